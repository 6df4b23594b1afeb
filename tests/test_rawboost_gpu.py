"""GPU: RawBoost (``air_rawboost_design`` / ``air_rawboost_ragged`` through ``augment.rawboost``) against
tests/rawboost_oracle.py: the design, every algorithm on rows around the tile size, both branches of the peak rule, the
ragged layout and its determinism, and the augmenter in front of the train step.

Every bound is the one the oracle derives (its module docstring); the oracle is fed the device's own taps, the Philox
words of tests/philox_oracle.py and, for SSI, ``randn_ref``.  The observed maxima are printed as a fraction of the bound
(profiles/rawboost.md records them)."""
import functools

import numpy as np
import pytest
import torch

import rawboost_oracle as ro
from oracle.filler import fill_module_

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _tile():
    from asvspoof2021_air_amd import _hip
    return int(_hip.lib().air_rawboost_tile())


def _lengths():
    t = _tile()
    return [1, 37, t - 1, t, t + 1, 2 * t + 3]


def _cap(lengths):
    return (max(lengths) + 7) // 8 * 8


# Per row of the six-row batch: the filter configuration (11 taps up to the 501 maximum: rows 0 and 1 are shorter than
# half their cascade), the amplitude of the input and the LnL gain.  Rows 0 - 2 keep every peak the rule sees at or below
# 0.95 (amplitude 0.2: ISD at most triples a sample, LnL passes at most max|H| = 1 of x plus attenuated powers), rows 3 - 5
# push every one to 1.05 or more (amplitude 0.9 - 1, + 12 dB on the linear filter, half the samples open to ISD); both
# are asserted on the oracle's own peaks, which cannot depend on the kernel.
ROWS = [
    dict(cfg=dict(nBands=1, minCoeff=11, maxCoeff=11), amp=0.2),
    dict(cfg=dict(minCoeff=101, maxCoeff=101), amp=0.2),
    dict(cfg=dict(), amp=0.2),
    dict(cfg=dict(minG=12.0, maxG=12.0, P=50.0, nBands=3), amp=1.0),
    dict(cfg=dict(minCoeff=101, maxCoeff=101, minG=12.0, maxG=12.0, P=50.0), amp=1.0),
    dict(cfg=dict(minG=12.0, maxG=12.0, P=50.0, SNRmin=0.0, SNRmax=5.0), amp=0.9),
]
SEED = 41


def _table(algos, rows, isd_base=5 << 20, ssi_base=(1 << 33) - 700):
    """Host table, row b drawn with its own configuration (the SSI base makes the counters cross 2^32 inside the call)."""
    rng = np.random.Generator(np.random.PCG64([SEED, len(algos)] + [a + 1 for a in algos]))
    return np.concatenate([ro.draw_table(rng, [a], dict(ro.DEFAULTS, **rows[b]["cfg"]), SEED, isd_base, ssi_base)
                           for b, a in enumerate(algos)])


def _pcm(lengths, cap, rows, dtype, fill="zero", seed=3):
    """(B, cap) host array: row b uniform in [-amp, amp] over its length; behind it zero or the worst value of the type."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = np.zeros((len(lengths), cap), dtype=np.float32)
    for b, n in enumerate(lengths):
        x[b, :n] = rng.uniform(-rows[b]["amp"], rows[b]["amp"], n).astype(np.float32)
    if dtype == "i16":
        x = np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)
    if fill != "zero":
        for b, n in enumerate(lengths):
            x[b, n:] = np.nan if dtype == "f32" else -32768
    return x


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_taps(table):
    """Per row the six cascades the device designed: lists of float32 arrays (empty: unused slot)."""
    from asvspoof2021_air_amd.augment import rawboost_design
    taps, lens = rawboost_design(_dev(table))
    taps, lens = taps.cpu().numpy(), lens.cpu().numpy()
    return [[taps[b, s, :lens[b, s]].copy() for s in range(ro.FILTERS)] for b in range(table.shape[0])], taps, lens


# ------------------------------------------------------------------------------------------------------------ design
def test_design_equals_the_oracle():
    algos = [3, 3, 3, 3, 3, 3, 1, -1]
    rows = ROWS + [dict(cfg=dict(maxF=300.0, maxBW=1000.0, minBW=900.0)), dict(cfg=dict())]
    rows[5] = dict(cfg=dict(minF=7700.0, minBW=900.0))  # every band clamps at fs / 2; row 6 would clamp at 0 but is ISD only
    rows[2] = dict(cfg=dict(maxF=300.0, minBW=900.0))   # every band clamps at 0
    table = _table(algos, rows)
    per_row, taps, lens = _device_taps(table)
    worst, sizes = 0.0, set()
    for b, a in enumerate(algos):
        for s in range(ro.FILTERS):
            bands, G = ro.get_filter(table[b], s)
            if a != 3:
                assert lens[b, s] == 0 and not taps[b, s].any()
                continue
            want, info = ro.notch(bands, G)
            assert lens[b, s] == want.size and not taps[b, s, want.size:].any()
            sizes.add(want.size)
            bound = ro.U * np.abs(want) + ro.design_bound(info, want.size, ro.DEV_ULP)
            err = np.abs(per_row[b][s].astype(np.float64) - want)
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (b, s, float((err / bound).max()))
    assert min(sizes) == 11 and max(sizes) == 501
    f1 = [fc - bw / 2 for fc, bw, _ in ro.get_filter(table[2], 0)[0]]
    f2 = [fc + bw / 2 for fc, bw, _ in ro.get_filter(table[5], 0)[0]]
    assert max(f1) <= 0 and min(f2) >= ro.FS / 2  # both clamps were exercised
    print("design: worst |taps - oracle| / bound = %.3f" % worst)


def test_design_refuses_what_the_call_would():
    from asvspoof2021_air_amd.augment import rawboost_design
    table = _table([0, 0, 0], ROWS[:3])
    table[0, ro.HDR + 4] = 12            # an even tap count
    table[1, ro.HDR + 1] = 9             # more bands than the table holds
    table[2, ro.HDR + 2: ro.HDR + 2 + 15] = [1000.0, 200.0, 201.0] * 5  # 5 * 201 - 4 = 1001 taps
    taps, lens = rawboost_design(_dev(table))
    assert lens[:, 0].tolist() == [0, 0, 0] and not bool(taps[:, 0].any())
    assert all(int(n) > 0 for n in lens[:, 1].tolist())


# ------------------------------------------------------------------------------------------------- algorithms, N0
@functools.lru_cache(maxsize=None)
def _run(algo, dtype, single):
    """One call and its per-row references.  single: the dense call on one row of exactly one tile."""
    from asvspoof2021_air_amd.augment import rawboost
    if single:
        lengths, rows, algos = [_tile()], [ROWS[4]], [algo]
    else:
        lengths, rows = _lengths(), ROWS
        algos = [algo] * 6
        algos[algo % 6] = -1
    cap = _cap(lengths)
    table, x = _table(algos, rows), _pcm(lengths, cap, rows, dtype)
    y = rawboost(_dev(x), _dev(table), lengths=None if single else _dev(np.array(lengths, dtype=np.int32))).cpu().numpy()
    per_row, _, _ = _device_taps(table)
    refs = [ro.row_reference(x[b, :n], b, cap, table[b], per_row[b]) for b, n in enumerate(lengths)]
    return dict(x=x, y=y, refs=refs, lengths=lengths, algos=algos, table=table)


@pytest.mark.parametrize("single", [False, True], ids=["B6", "B1"])
@pytest.mark.parametrize("dtype", ["f32", "i16"])
@pytest.mark.parametrize("algo", range(8))
def test_algorithm_equals_the_oracle(algo, dtype, single):
    c = _run(algo, dtype, single)
    worst, peaks = 0.0, []
    for b, n in enumerate(c["lengths"]):
        ref, got = c["refs"][b], c["y"][b]
        assert not got[n:].any()
        if c["algos"][b] < 0:
            assert np.array_equal(got[:n], ro.to_f32(c["x"][b, :n]))  # copied (converted, for int16)
            continue
        err = np.abs(got[:n].astype(np.float64) - ref["y"])
        bound = ref["err"] + ro.U * np.abs(ref["y"])  # (the value itself is an fp32 number)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (b, n, int(np.argmax(err / np.maximum(bound, 1e-300))), float(err.max()))
        peaks += [(b, p) for p in ref["peaks"]]
        if algo == 1 and ref["peaks"][0] <= 1.0:  # ISD alone below the peak rule: the selection shows bit for bit
            x32 = ro.to_f32(c["x"][b, :n])
            assert not np.any((got[:n] != x32) & ~ref["sel"])
            moved = np.abs(ref["y"] - x32) > np.spacing(np.abs(x32))
            assert np.all((got[:n] != x32)[ref["sel"] & moved])
    # the peak rule: every peak the oracle sees is clear of 1, and a six-row batch shows both branches
    assert all(p <= 0.95 or p >= 1.05 for _, p in peaks), peaks
    if not single and algo != 2:
        assert any(p <= 0.95 for _, p in peaks) and any(p >= 1.05 for _, p in peaks), peaks
    print("algo %d %s %s: worst error / bound = %.3f" % (algo, dtype, "B1" if single else "B6", worst))


def test_isd_selection_rate_and_ssi_level():
    """What the two noise stages are for, on the long high-level row: about beta of the samples move, and the noise
    sits at the drawn SNR."""
    c = _run(1, "f32", False)
    b, n = 5, c["lengths"][5]
    sel = c["refs"][b]["sel"]
    rate = c["table"][b, 1] / 2.0 ** 32
    assert abs(sel.mean() - rate) <= 4.0 * np.sqrt(rate * (1 - rate) / n)
    c = _run(2, "f32", False)
    x = ro.to_f32(c["x"][b, :n]).astype(np.float64)
    noise = c["y"][b, :n].astype(np.float64) - x
    snr = 20.0 * np.log10(np.linalg.norm(x) / np.linalg.norm(noise))
    assert abs(snr - c["table"][b, 5]) <= 1e-3


# ------------------------------------------------------------------------------------------- layout and determinism
MIXED = [3, 7, 5, -1, 6, 0]


@pytest.mark.parametrize("dtype", ["f32", "i16"])
def test_layout_and_determinism(dtype):
    from asvspoof2021_air_amd.augment import rawboost
    lengths = _lengths()
    cap = _cap(lengths)
    table = _table(MIXED, ROWS)
    ld, td = _dev(np.array(lengths, dtype=np.int32)), _dev(table)
    x = _pcm(lengths, cap, ROWS, dtype)
    y = rawboost(_dev(x), td, lengths=ld)
    again = rawboost(_dev(x), td, lengths=ld)
    assert torch.equal(y, again)  # a call repeats its bits
    worst = rawboost(_dev(_pcm(lengths, cap, ROWS, dtype, fill="worst")), td, lengths=ld)
    assert torch.equal(y, worst)  # nothing at or behind L_b is read
    out = torch.full((6, cap), 7.0, device="cuda")
    assert rawboost(_dev(x), td, lengths=ld, out=out) is out and torch.equal(out, y)
    y = y.cpu().numpy()
    assert np.isfinite(y).all()
    for b, n in enumerate(lengths):
        assert not y[b, n:].any()
        if MIXED[b] < 0:
            assert np.array_equal(y[b, :n], ro.to_f32(x[b, :n]))
            continue
        # the dense call on the utterance alone, its table row carrying the row's own counter bases
        row = table[b:b + 1].copy()
        row[0, 3] += b * cap
        row[0, 4] += b * ((cap + 3) // 4)
        alone = rawboost(_dev(x[b:b + 1, :n]), _dev(row)).cpu().numpy()
        assert np.array_equal(alone[0], y[b, :n]), (b, n)
        assert np.any(y[b, :n] != ro.to_f32(x[b, :n])) or n == 1  # the row was augmented


def test_host_lengths_and_bad_arguments():
    from asvspoof2021_air_amd import _hip
    from asvspoof2021_air_amd.augment import rawboost
    lengths = _lengths()
    cap = _cap(lengths)
    table, x = _dev(_table(MIXED, ROWS)), _dev(_pcm(lengths, cap, ROWS, "f32"))
    assert torch.equal(rawboost(x, table, lengths=lengths), rawboost(x, table, lengths=_dev(np.array(lengths, dtype=np.int32))))
    with pytest.raises(ValueError):
        rawboost(x, table, lengths=[1, 2, 3, 4, 5, cap + 1])
    with pytest.raises(ValueError):
        rawboost(x, table[:5])
    with pytest.raises(_hip.AirError):
        rawboost(x, table, out=x)
    with pytest.raises(_hip.AirError):
        rawboost(x.cpu(), table)


# ----------------------------------------------------------------------------------------------------------- trainer
B, CAP = 4, 9300
LENS = [[9300, 159, 6000, 4481], [4480, 9300, 2049, 9299]]


def _trainer(graph, augment, feat_len=48, seed=4242):
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.resnet import ResNet
    from asvspoof2021_air_amd.train import Trainer
    m = ResNet(3, 256, resnet_type="18", nclasses=2)
    fill_module_(m)
    m = m.cuda()
    m._noise_seed = seed
    lossm = AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)
    fill_module_(lossm)
    tr = Trainer(m, loss_module=lossm, feat_len=feat_len, augment=augment)
    if graph:
        tr.enable_graph(segments=False)
    else:
        m.overlap_wgrad = False  # the capture is one chain; same launches eagerly
    return m, tr


def _batches():
    rows = [dict(amp=0.5)] * B
    out = []
    for i in range(2):
        pcm = _dev(_pcm(LENS[i], CAP, rows, "i16" if i else "f32", seed=500 + i))
        out.append((pcm, ((torch.arange(B) + i) % 3 != 0).long().cuda(), _dev(np.array(LENS[i], dtype=np.int32))))
    return out


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
def test_trainer_steps_eager_and_replayed_are_bit_equal(ragged):
    """Four steps each way: the replaying trainer runs two eagerly, captures on the third and replays the fourth; the
    augmenter runs ahead of the captured region either way and draws from the same seed."""
    from asvspoof2021_air_amd.augment import RawBoostAugment
    batches = _batches()
    ends = []
    for graph in (False, True):
        aug = RawBoostAugment(algos=(0, 1, 2, 3, 4, 5, 6, 7), p=0.8, seed=11)
        m, tr = _trainer(graph, aug)
        losses = []
        for i in range(4):
            pcm, lab, ln = batches[i % 2]
            if ragged:
                losses.append(tr.step(pcm, lab, lengths=ln)[0].item())
            else:
                losses.append(tr.step(pcm if pcm.dtype == torch.float32 else pcm.float() / 32768.0, lab)[0].item())
        torch.cuda.synchronize()
        if graph:
            assert tr._graph is not None
        ends.append((losses, m.arena().flat.clone(), aug.rng.bit_generator.state, (aug.isd_base, aug.ssi_base)))
    (l0, w0, r0, b0), (l1, w1, r1, b1) = ends
    assert all(np.isfinite(l0)) and l0 == l1
    assert torch.equal(w0, w1) and r0 == r1 and b0 == b1 and b0[0] == 4 * B * ro.MAXL


def test_augmenter_equals_the_function_form_on_its_own_table():
    from asvspoof2021_air_amd.augment import RawBoostAugment, rawboost
    pcm, _, ln = _batches()[1]
    a, b = RawBoostAugment(algos=(3, 6), p=0.7, seed=8), RawBoostAugment(algos=(3, 6), p=0.7, seed=8)
    got = a(pcm, lengths=ln)
    idx = b.draw(B)
    want = rawboost(pcm, _dev(b.params(idx)), lengths=ln)
    assert torch.equal(got, want) and got.dtype == torch.float32
    assert torch.equal(a(pcm, idx=np.array([-1] * B), lengths=ln)[0, :LENS[1][0]], pcm[0, :LENS[1][0]].float() / 32768.0)


def test_adversarial_step_takes_the_chains_labels():
    from asvspoof2021_air_amd.adversarial import AdversarialTrainer
    from asvspoof2021_air_amd.augment import AugmentChain, CodecAugment, RawBoostAugment
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.resnet import ResNet
    chain = AugmentChain(waveform=RawBoostAugment(algos=(3, 5, 7), p=0.7, seed=3), codec=CodecAugment(p=0.7, seed=4), device=None)
    pcm, lab, ln = _batches()[0]
    am = ResNet(3, 256, resnet_type="18", nclasses=2)
    fill_module_(am)
    am.set_attention_noise(None)
    lossm = AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)
    fill_module_(lossm)
    atr = AdversarialTrainer(am, (4, 3), loss_module=lossm, feat_len=48, augment=chain)
    channels = chain.prepare(B)
    assert channels.shape == (B, 2) and int(channels[:, 0].max()) <= 3 and int(channels[:, 1].max()) <= 2
    loss, _ = atr.step(pcm, lab, channels=channels, lengths=ln)
    assert bool(torch.isfinite(loss).all()) and chain._prepared is None
