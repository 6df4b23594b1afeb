"""The streams of tests/test_flac_cpu.py (oracle round trips) and tests/test_flac_gpu.py (device decode): every case is a
list of rows ``(samples int16, blocksize, frame specs)`` for ``flac_oracle.encode``.  Built once per process."""
import functools

import numpy as np

import flac_oracle as fo

BLOCKSIZES = (16, 192, 4096)  # 16 is the format's minimum


def signal(n, seed, amp=12000):
    """A band-limited int16 signal with some noise: predictors leave small but non-trivial residuals."""
    rng = np.random.RandomState(seed)
    t = np.arange(n)
    x = amp * np.sin(2 * np.pi * t * (0.003 + 0.01 * rng.rand())) + 0.3 * amp * np.sin(2 * np.pi * t * 0.041 + rng.rand())
    x = x + rng.randint(-200, 201, size=n)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def lpc_spec(order, seed):
    rng = np.random.RandomState(100 + seed)
    if order == 1:
        return dict(type="lpc", coefs=[7], precision=4, shift=3)
    if order == 8:
        return dict(type="lpc", coefs=[int(c) for c in rng.randint(-900, 901, size=8)], precision=12, shift=10)
    return dict(type="lpc", coefs=[int(c) for c in rng.randint(-4000, 4001, size=order)], precision=15, shift=14)


SUBFRAME_TYPES = ["constant", "verbatim", "fixed0", "fixed1", "fixed2", "fixed3", "fixed4", "lpc1", "lpc8", "lpc32"]


def _lengths(bs):
    k = 2 if bs == 4096 else 3
    return ((k * bs, 0), (k * bs + 1, 1), (k * bs + 37, 37))


def subframe_rows(kind):
    """One stream per block size (16, 192, 4096) and total length (k bs, k bs + 1, k bs + 37): the short last frame takes
    the 8-bit explicit block-size code for + 1 and, forced, the 16-bit one for + 37.  The format bounds the predictor
    order by the block size: LPC 32 at block size 16 is written as LPC 16 (the largest the block admits)."""
    rows = []
    for bs in BLOCKSIZES:
        for n, extra in _lengths(bs):
            x = signal(n, seed=bs + n)
            if kind == "constant":
                x = np.repeat(signal(-(-n // bs), seed=n), bs)[:n]
                spec = dict(type="constant")
            elif kind == "verbatim":
                spec = dict(type="verbatim")
            elif kind.startswith("fixed"):
                spec = dict(type="fixed", order=int(kind[5:]))
            else:
                order = min(int(kind[3:]), bs)
                spec = lpc_spec(order, seed=bs)
            last = dict(spec)
            if extra == 37:
                last["bs_code"] = 7
            nfr = -(-n // bs)
            rows.append((x, bs, [spec] * (nfr - 1) + [last if n % bs else spec]))
    return rows


def accumulator_rows():
    """LPC order 32, precision 15, coefficients (-1)^j 16383, shift 14 over samples alternating -32768 / 32767: every
    product has one sign, the prediction sum is ~1.7e10 - a 32-bit accumulator gives wrong samples - and the residuals
    still fit 32 bits."""
    n = 2 * 192 + 37
    x = np.where(np.arange(n) % 2 == 0, -32768, 32767).astype(np.int16)
    spec = dict(type="lpc", coefs=[(-1) ** j * 16383 for j in range(32)], precision=15, shift=14, method=1, params=None)
    return [(x, 192, [spec])]


def residual_rows():
    rng = np.random.RandomState(5)
    rows = []
    # Rice parameter 0 and 14, Rice2 parameter 30
    rows.append((rng.randint(-1, 2, size=192 * 2 + 5).astype(np.int16), 192, [dict(type="fixed", order=0, params=0)]))
    rows.append((rng.randint(-32768, 32768, size=192 * 2).astype(np.int16), 192, [dict(type="fixed", order=0, params=14)]))
    rows.append((signal(192 + 37, 11), 192, [dict(type="fixed", order=2, method=1, params=30)]))
    # escape partitions: n = 0 (order 1 over a constant run: the residual is zero), 1 and 17
    rows.append((np.full(192 * 2, -1234, dtype=np.int16), 192, [dict(type="fixed", order=1, params=("esc", 0))]))
    rows.append((rng.randint(-1, 1, size=192 + 16).astype(np.int16), 192, [dict(type="fixed", order=0, params=("esc", 1))]))
    rows.append((rng.randint(-32768, 32768, size=192 * 2 + 1).astype(np.int16), 192,
                 [dict(type="fixed", order=1, method=1, params=("esc", 17))]))
    # partition order 0 and the maximum: 4096 samples in 16-sample partitions, Rice and escape partitions mixed
    x = signal(4096 * 2, 12)
    mixed = [None if p % 3 else ("esc", 17) for p in range(256)]
    mixed[5], mixed[6] = 0, 14
    rows.append((x, 4096, [dict(type="fixed", order=2, partition_order=8, params=mixed),
                           dict(type="fixed", order=3, partition_order=0)]))
    rows.append((signal(4096, 13), 4096, [dict(lpc_spec(8, 3), method=1, partition_order=8, params=None)]))
    # the predictor order equals the first partition's size: that partition carries no residual
    rows.append((signal(64 * 3, 14), 64, [dict(type="fixed", order=4, partition_order=4),
                                          dict(lpc_spec(8, 4), partition_order=3)]))
    rows.append((signal(16 * 4, 15), 16, [dict(lpc_spec(16, 5), partition_order=0)]))
    # a residual of 5000 under parameter 0: a unary run of 10,000 zero bits (and -5000: 9,999)
    x = np.zeros(192 * 2, dtype=np.int16)
    x[[7, 100, 200]] = 5000
    x[[50, 300]] = -5000
    rows.append((x, 192, [dict(type="fixed", order=0, params=0)]))
    return rows


def wasted_rows():
    rows = []
    for k in (1, 15):
        rng = np.random.RandomState(20 + k)
        lim = 1 << (15 - k)
        n = 192 * 2 + 37

        def draw(m):
            return (rng.randint(-lim, lim, size=m).astype(np.int64) << k).astype(np.int16)
        rows.append((np.repeat(draw(3), 192)[:n], 192, [dict(type="constant", wasted=k)]))
        rows.append((draw(n), 192, [dict(type="verbatim", wasted=k)]))
        rows.append((draw(n), 192, [dict(type="lpc", coefs=[3, -2, 1], precision=4, shift=2, wasted=k)]))
        rows.append((draw(n), 16, [dict(type="fixed", order=2, wasted=k), dict(type="fixed", order=0)]))
    return rows


def header_rows():
    """Every sample-rate code (parsed and ignored), the sample-size code "from STREAMINFO", the 16-bit explicit
    block size on full frames."""
    specs = [dict(type="fixed", order=1, sr_code=c, size_code=0 if c % 2 else 4) for c in range(15)]
    specs += [dict(type="verbatim", bs_code=7), dict(type="fixed", order=2, bs_code=6)]
    return [(signal(192 * len(specs) + 3, 30), 192, specs)]


def frame_number_rows():
    """2,049 frames of 16 samples: frame numbers coded in 1, 2 and 3 bytes, and a scan over many tiny frames."""
    return [(signal(16 * 2049, 31), 16, [dict(type="fixed", order=2), dict(type="verbatim"), dict(type="fixed", order=0)])]


FALSE_VALUE = 0x1234


def false_sync_row():
    """A VERBATIM frame whose samples spell a complete, valid CONSTANT frame of 192 samples of FALSE_VALUE (correct
    CRC-8 and CRC-16, frame number 1 - the number of the frame that really follows).  A VERBATIM payload without wasted
    bits is byte aligned (6 header bytes + 1 subframe byte), so any even-length byte string fits."""
    inner = fo.encode_frame(np.full(192, FALSE_VALUE), 1, dict(type="constant", sr_code=12))
    assert len(inner) % 2 == 0
    x = signal(192 * 3, 32)
    x[20:20 + len(inner) // 2] = np.frombuffer(inner, dtype=">i2")
    return (x, 192, [dict(type="verbatim")]), inner


def ragged_rows():
    return [(signal(1, 40), 16, None),                          # nothing but a 1-sample frame
            (signal(3 * 4096 + 37, 41), 4096, [lpc_spec(8, 6), dict(type="fixed", order=3)]),
            (signal(16 * 5 + 3, 42), 16, [dict(type="fixed", order=1)]),
            (signal(192 * 7, 43), 192, [dict(type="verbatim"), lpc_spec(32, 7)]),
            (signal(4096, 44), 4096, [dict(type="fixed", order=4, partition_order=4)])]


def unsupported_rows():
    """Frames outside the served subset, each in the middle of an otherwise fine stream."""
    ok = dict(type="fixed", order=1)
    lp = dict(type="lpc", coefs=[3, -2, 1], unchecked=True)
    return [(signal(192 * 3, 50), 192, [ok, dict(ok, channel_code=8), ok]),            # left / side stereo
            (signal(192 * 3, 51), 192, [ok, dict(lp, precision=4, shift=-1), ok]),     # negative shift
            (signal(192 * 3, 52), 192, [ok, dict(lp, precision=16, shift=2), ok]),     # precision code 1111
            (signal(192 * 3, 53), 192, [ok, dict(ok, size_code=6), ok])]               # 24-bit frames


@functools.lru_cache(maxsize=None)
def case(name):
    """-> rows [(samples, blocksize, specs)] of a named case."""
    if name in SUBFRAME_TYPES:
        return subframe_rows(name)
    return {"accumulator": accumulator_rows, "residual": residual_rows, "wasted": wasted_rows, "header": header_rows,
            "frame_numbers": frame_number_rows, "false_sync": lambda: [false_sync_row()[0]],
            "ragged": ragged_rows}[name]()


CASES = SUBFRAME_TYPES + ["accumulator", "residual", "wasted", "header", "frame_numbers", "false_sync", "ragged"]


@functools.lru_cache(maxsize=None)
def streams(name):
    """-> [(stream bytes, samples)] of a case, encoded once."""
    return [(fo.encode(x, bs, specs), x) for x, bs, specs in case(name)]
