"""CPU: the RawBoost oracle (tests/rawboost_oracle.py) against scipy.signal, the host side of ``RawBoostAugment`` against
the oracle's restatement of its draw order, and ``AugmentChain`` with and without the new stage."""
import numpy as np
import pytest
import torch

import rawboost_oracle as ro


# ------------------------------------------------------------------------------------------------------------ design
def _scipy_notch(bands, G):
    from scipy import signal
    b = np.ones(1)
    for fc, bw, c in bands:
        f1, f2 = fc - bw / 2, fc + bw / 2
        if f1 <= 0:
            f1 = 1 / 1000
        if f2 >= ro.FS / 2:
            f2 = ro.FS / 2 - 1 / 1000
        b = np.convolve(signal.firwin(int(c), [float(f1), float(f2)], window="hamming", fs=ro.FS), b)
    _, h = signal.freqz(b, 1, fs=ro.FS)
    return pow(10, G / 20) * b / np.amax(np.abs(h))


def _drawn_sets():
    """200 sets from the default ranges (odd and even c before the + 1; f1 <= 0 occurs: minF - maxBW / 2 < 0), then sets
    that force each clamp and the one-band / longest cascades."""
    rng = np.random.Generator(np.random.PCG64(5))
    sets = [(ro.draw_bands(rng, ro.DEFAULTS), ro.uniform(rng, -20.0, 0.0)) for _ in range(200)]
    sets += [([(30.0, 900.0, 11)], 0.0), ([(7990.0, 800.0, 101)], -3.0), ([(100.0, 1000.0, 101)] * 5, -12.0),
             ([(7800.0, 1000.0, 13), (40.0, 100.0, 11)], 0.0), ([(4000.0, 500.0, 1)], 0.0)]
    return sets


def test_design_equals_scipy_on_drawn_parameter_sets():
    sets = _drawn_sets()
    lo = sum(fc - bw / 2 <= 0 for bands, _ in sets for fc, bw, _ in bands)
    hi = sum(fc + bw / 2 >= ro.FS / 2 for bands, _ in sets for fc, bw, _ in bands)
    rng = np.random.Generator(np.random.PCG64(5))
    raw = [int(ro.uniform(rng, 10, 100)) for _ in range(50)]
    assert lo >= 2 and hi >= 2 and any(c % 2 == 0 for c in raw) and len(sets) >= 200
    worst = 0.0
    for bands, G in sets:
        assert all(int(c) % 2 == 1 for _, _, c in bands)
        got, info = ro.notch(bands, G)
        want = _scipy_notch(bands, G)
        assert got.shape == want.shape == (sum(int(c) for _, _, c in bands) - (len(bands) - 1),)
        bound = ro.design_bound(info, got.size)
        err = np.abs(got - want).max()
        worst = max(worst, err / bound)
        assert err <= bound, (bands, G, err, bound)
    print("design vs scipy: worst error / bound = %.3g" % worst)


def test_even_draw_becomes_odd():
    class Fixed:
        def __init__(self, v):
            self.v = list(v)

        def random(self):
            return self.v.pop(0)

    cfg = dict(ro.DEFAULTS, nBands=2)
    bands = ro.draw_bands(Fixed([0.5, 0.5, 0.0, 0.5, 0.5, 0.5 / 90]), cfg)  # c = int(10.0) = 10 -> 11; int(10.5) = 10 -> 11
    assert [c for _, _, c in bands] == [11, 11]
    bands = ro.draw_bands(Fixed([0.5, 0.5, 1.5 / 90, 0.5, 0.5, 89.9 / 90]), cfg)
    assert [c for _, _, c in bands] == [11, 99]


@pytest.mark.parametrize("taps", [11, 101, 501])
@pytest.mark.parametrize("L", [1, 5, 37, 400])
def test_centred_fir_equals_pad_lfilter_slice(L, taps):
    from scipy import signal
    rng = np.random.Generator(np.random.PCG64(L * 1000 + taps))
    b, x = rng.standard_normal(taps), rng.standard_normal(L)
    N = b.shape[0] + 1
    y = signal.lfilter(b, 1, np.pad(x, (0, N), "constant"))
    want = y[int(N / 2):int(y.shape[0] - N / 2)]
    got = ro.centred_fir(b, x)
    assert got.shape == want.shape == (L,)
    # both are sums of at most `taps` products of the same operands: (taps + 2) u64 sum |b| |x| each
    bound = 2 * (taps + 2) * ro.U64 * ro.centred_fir(np.abs(b), np.abs(x))
    assert np.all(np.abs(got - want) <= bound + 1e-300)


# ------------------------------------------------------------------------------------------------------- host tables
def test_layout_constants_match_the_library():
    from asvspoof2021_air_amd import _hip, augment, build
    build.build(verbose=False)
    lib = _hip.lib()
    assert lib.air_rawboost_row_doubles() == augment.RB_ROW == ro.ROW == 164
    assert lib.air_rawboost_tile() > 0 and lib.air_rawboost_tile() % 8 == 0
    assert lib.air_rawboost_ws_bytes(4, 9000) > 3 * 4 * 9000 * 4
    assert lib.air_rawboost_ws_bytes(0, 9000) == 0 and lib.air_rawboost_ws_bytes(4, augment.RB_MAXL + 1) == 0
    assert (augment.RB_KEY_TAG, augment.RB_MAXL) == (ro.KEY_TAG, ro.MAXL)
    assert augment.RB_DEFAULTS == ro.DEFAULTS


@pytest.mark.parametrize("config", [{}, dict(nBands=3, N_f=2, minG=-2.0, maxG=1.0, P=40.0, minCoeff=11, maxCoeff=11)])
def test_params_equal_the_restated_draw_order(config):
    from asvspoof2021_air_amd.augment import RawBoostAugment
    algos = (0, 1, 2, 3, 4, 5, 6, 7)
    aug = RawBoostAugment(algos=algos, p=0.8, seed=77, device="cpu", **config)
    rng = np.random.Generator(np.random.PCG64(77))
    cfg = dict(ro.DEFAULTS, **config)
    isd_base = ssi_base = 0
    for B in (9, 4, 9):
        idx = aug.draw(B)
        want_idx = rng.integers(0, len(algos), size=B).astype(np.int32)
        want_idx[rng.random(B) >= 0.8] = -1
        assert np.array_equal(idx, want_idx)
        got = aug.params(idx)
        want = ro.draw_table(rng, [algos[i] if i >= 0 else -1 for i in want_idx], cfg, 77, isd_base, ssi_base)
        assert got.dtype == np.float64 and got.shape == (B, ro.ROW)
        assert np.array_equal(got, want)
        isd_base += B * ro.MAXL
        ssi_base += B * (ro.MAXL // 4)
    assert aug.rng.bit_generator.state == rng.bit_generator.state


def test_table_entries_are_in_range():
    from asvspoof2021_air_amd.augment import RawBoostAugment
    aug = RawBoostAugment(algos=(3, 7), seed=3, device="cpu")
    t = aug.params(aug.draw(16))
    for row in t:
        assert 0 <= row[1] < 0.1 * 2 ** 32 and row[1] == np.floor(row[1]) and row[2] == 2.0
        for slot in range(ro.NF + (1 if row[0] == 3 else 0)):
            bands, G = ro.get_filter(row, slot)
            assert len(bands) == 5 and all(11 <= c <= 99 and c % 2 == 1 for _, _, c in bands)
            assert (G == 0.0) if slot in (0, ro.NF) else (-20.0 <= G <= -5.0)
        if row[0] == 7:
            assert not row[ro.HDR + ro.NF * ro.FREC:].any()  # no SSI filter


def test_a_refused_batch_does_not_advance_the_generator():
    from asvspoof2021_air_amd.augment import RawBoostAugment
    aug = RawBoostAugment(seed=5, device="cpu")
    state, bases = aug.rng.bit_generator.state, (aug.isd_base, aug.ssi_base)
    pcm = torch.zeros(3, 100)
    for bad in ([10, 0, 5], [10, 101, 5], [10, 20], [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError):
            aug(pcm, lengths=bad)
    assert aug.rng.bit_generator.state == state and (aug.isd_base, aug.ssi_base) == bases


def test_successive_calls_use_disjoint_counter_ranges():
    from asvspoof2021_air_amd.augment import RawBoostAugment
    aug = RawBoostAugment(algos=(3,), seed=9, device="cpu")
    spans = []
    for B in (64, 3, 64):
        t = aug.params(aug.draw(B))
        assert np.all(t[:, 3] == t[0, 3]) and np.all(t[:, 4] == t[0, 4])
        assert t[0, 6] != t[0, 7]  # the two stages draw under different keys
        spans.append(ro.counter_ranges(t, B))
    for kind in (0, 1):
        r = sorted(s[kind] for s in spans)
        assert all(r[i][1] <= r[i + 1][0] for i in range(2)), r
    # what a call touches lies inside what it reserves: B rows of Lcap <= 2^20 samples / ceil(Lcap / 4) quads
    assert 64 * ro.MAXL <= spans[0][0][1] - spans[0][0][0] and 64 * ((ro.MAXL + 3) // 4) <= spans[0][1][1] - spans[0][1][0]


def test_configurations_that_could_exceed_the_tap_limit_are_refused():
    from asvspoof2021_air_amd.augment import RawBoostAugment
    RawBoostAugment(device="cpu")  # the defaults: 5 * 101 - 4 = 501
    for bad in (dict(maxCoeff=104), dict(nBands=6), dict(nBands=9, maxCoeff=11), dict(N_f=6), dict(minCoeff=0), dict(nope=1)):
        with pytest.raises(ValueError):
            RawBoostAugment(device="cpu", **bad)
    with pytest.raises(ValueError):
        RawBoostAugment(algos=(8,), device="cpu")


# ------------------------------------------------------------------------------------------------------------- chain
def _stages():
    from asvspoof2021_air_amd.augment import ChannelAugment, CodecAugment
    return CodecAugment(p=0.7, seed=1, device="cpu"), ChannelAugment(irs=torch.zeros(4, 8), p=0.7, seed=2, device="cpu")


def test_chain_without_waveform_is_unchanged():
    from asvspoof2021_air_amd.augment import AugmentChain
    codec, dev = _stages()
    both = AugmentChain(codec, dev).prepare(6)
    assert both.dtype == torch.int64 and both.tolist() == [[0, 4], [2, 2], [2, 0], [0, 2], [1, 2], [1, 4]]
    codec, dev = _stages()
    one = AugmentChain(codec=codec).prepare(6)
    assert one.dtype == torch.int64 and one.tolist() == [0, 2, 2, 0, 1, 1]
    assert AugmentChain(device=dev).prepare(6).tolist() == [4, 2, 0, 2, 2, 4]
    with pytest.raises(ValueError, match="AugmentChain needs a codec stage, a device stage, or both"):
        AugmentChain()
    chain = AugmentChain(*_stages())
    chain.prepare(6)
    with pytest.raises(ValueError, match="prepared for a batch of 6, called with 5"):
        chain(torch.zeros(5, 10))


def test_chain_with_waveform_adds_its_column_in_front():
    from asvspoof2021_air_amd.augment import AugmentChain, RawBoostAugment
    codec, dev = _stages()
    wave = RawBoostAugment(algos=(3, 5, 7), p=0.6, seed=4, device="cpu")
    chain = AugmentChain(codec, dev, waveform=wave)
    assert chain.stages == [wave, codec, dev]
    labels = chain.prepare(6)
    assert labels.shape == (6, 3) and labels[:, 1:].tolist() == [[0, 4], [2, 2], [2, 0], [0, 2], [1, 2], [1, 4]]
    want = RawBoostAugment(algos=(3, 5, 7), p=0.6, seed=4, device="cpu").draw(6)
    assert labels[:, 0].tolist() == [int(i) + 1 if i >= 0 else 0 for i in want] and int(labels[:, 0].max()) <= 3
    alone = AugmentChain(waveform=RawBoostAugment(algos=(3, 5, 7), p=0.6, seed=4, device="cpu")).prepare(6)
    assert alone.shape == (6,) and alone.tolist() == labels[:, 0].tolist()
