"""float64 restatement of the G.711 transmission-codec stage (``air_g711_ragged``, include/air_hip.h), for the tests only.

The coding is CPython's ``audioop`` (ITU-T G.711: lin2ulaw / ulaw2lin / lin2alaw / alaw2lin at width 2); the two filters
are the definition's sums, evaluated with numpy in float64.  Nothing here is shared with the kernel."""
import audioop
import functools

import numpy as np

LAWS = ("ulaw", "alaw")
_ENC = (audioop.lin2ulaw, audioop.lin2alaw)
_DEC = (audioop.ulaw2lin, audioop.alaw2lin)


def encode(s16, law):
    """int16 array -> uint8 codes (law 0: mu-law, 1: A-law)."""
    s16 = np.ascontiguousarray(s16, dtype="<i2")
    return np.frombuffer(_ENC[law](s16.tobytes(), 2), dtype=np.uint8).reshape(s16.shape).copy()


def decode(codes, law):
    """uint8 codes -> int16."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    return np.frombuffer(_DEC[law](codes.tobytes(), 2), dtype="<i2").reshape(codes.shape).astype(np.int16)


@functools.lru_cache(maxsize=None)
def tables(law):
    """(codes of all 65 536 16-bit values in the order -32768 .. 32767, decoded values of the 256 codes)."""
    return encode(np.arange(-32768, 32768).astype(np.int16), law), decode(np.arange(256, dtype=np.uint8), law)


def step_at(code, law):
    """Quantiser step, in 16-bit units, of the segment that ``code`` lies in: the distance between neighbouring decoded
    levels there (mu-law 8 << seg; A-law 16 in segments 0 and 1, 16 << (seg - 1) above)."""
    code = np.asarray(code, dtype=np.int64)
    if law == 0:
        return 8 << (((~code) & 0x70) >> 4)
    seg = ((code ^ 0x55) & 0x70) >> 4
    return 16 << np.maximum(seg - 1, 0)


def quantise(u):
    """clamp(rint(u * 32768)), ties to even -> int16."""
    return np.clip(np.rint(np.asarray(u, dtype=np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def decimate(x, fir):
    """u[m] = sum_k fir[k] x[2 m + c - k], m in [0, ceil(L / 2)), x zero outside [0, L).  float64."""
    x, fir = np.asarray(x, dtype=np.float64), np.asarray(fir, dtype=np.float64)
    c = (len(fir) - 1) // 2
    full = np.convolve(x, fir)  # full[i] = sum_k fir[k] x[i - k]
    return full[c:c + len(x):2].copy()


def interpolate(v, fir, L):
    """y[n] = 2 sum_k fir[k] vup[n + c - k], vup[2 m] = v[m], zero elsewhere, n in [0, L).  float64."""
    v, fir = np.asarray(v, dtype=np.float64), np.asarray(fir, dtype=np.float64)
    c = (len(fir) - 1) // 2
    vup = np.zeros(2 * len(v))
    vup[::2] = v
    return 2.0 * np.convolve(vup, fir)[c:c + L]


def codec_row(x, fir, law, resample=True, normalize=True):
    """One utterance (L,) -> dict(u: the pre-rounding 8 kHz signal in 16-bit units, codes, y).  law < 0: unchanged."""
    x = np.asarray(x, dtype=np.float64)
    if law < 0:
        return dict(u=None, codes=np.zeros(0, dtype=np.uint8), y=x.copy())
    u = decimate(x, fir) if resample else x
    codes = encode(quantise(u), law)
    v = decode(codes, law).astype(np.float64) / 32768.0
    y = interpolate(v, fir, len(x)) if resample else v
    if normalize and np.abs(y).max() > 0:
        y = y * (np.abs(x).max() / np.abs(y).max())
    return dict(u=u * 32768.0, codes=codes, y=y)


def codec_definition(x, fir, law):
    """The literal double loops of the definition (no numpy.convolve), un-normalised: (codes, y).  Small inputs only."""
    L, K = len(x), len(fir)
    c, M = (K - 1) // 2, (len(x) + 1) // 2
    u = [sum(float(fir[k]) * float(x[2 * m + c - k]) for k in range(K) if 0 <= 2 * m + c - k < L) for m in range(M)]
    codes = encode(quantise(u), law)
    v = decode(codes, law).astype(np.float64) / 32768.0
    y = [2.0 * sum(float(fir[k]) * v[(n + c - k) // 2] for k in range(K)
                   if (n + c - k) % 2 == 0 and 0 <= (n + c - k) // 2 < M) for n in range(L)]
    return codes, np.array(y)
