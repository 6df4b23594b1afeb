"""GPU: the STFT and Melspec front-ends (csrc/spectral.hip through feature_extraction.STFT / Melspec), their Dataset and
Trainer wiring.

Error bound.  Power-domain outputs are measured with ``spectral_oracle.frame_rel_err``: max |y - y64| over that frame's
largest fp64 value, all-zero frames compared for equality.  e_ref is the worst such error of the fixture's fp32 baseline
(the reference's own STFT on the CPU; the fp32 restatement of the mel spectrogram) against the fp64 oracle, and a kernel
must stay within 4 x e_ref: its FFT is another factorisation (16 x 16 complex + the real-FFT untangle) with two more
roundings per bin than a library rfft.  Against the fp32 baseline itself the bound is 5 x e_ref (triangle inequality).
Measured on an MI355X: see ``test_dense_vs_oracle``'s output and profiles/spectral_frontends.md.

Everything that is data movement - layouts, pad modes, crops, ragged rows, int16 input - is held bit for bit."""
import numpy as np
import pytest
import torch

import spectral_oracle as so
from oracle import lfcc as o_lfcc
from oracle import pad as o_pad
from oracle.filler import fill_module_, synth_pcm

pytestmark = pytest.mark.gpu

MARGIN = 4.0
KINDS = ["stft", "mel_constant", "mel_reflect"]
HOP = {"stft": 160, "mel_constant": 128, "mel_reflect": 128}
DIM = {"stft": 257, "mel_constant": 128, "mel_reflect": 128}


def make(kind, **kw):
    from asvspoof2021_air_amd.feature_extraction import STFT, Melspec
    if kind == "stft":
        m = STFT(320, 160, 512, 16000, **kw).cuda()
        m.mutate_input = False
        return m
    return Melspec(kind[4:]).cuda()


def dense(m, x):
    """(B, T, D) of either front-end."""
    return m.forward_frames(x) if hasattr(m, "forward_frames") else m(x)


def oracle64(kind, x, **kw):
    x = x.cpu().numpy()
    return so.stft_power(x, **kw) if kind == "stft" else so.mel_power(x, kind[4:])


@pytest.fixture(scope="module")
def e_ref(golden):
    """Worst error of the fixture's fp32 baselines against the fp64 oracle, per front-end (computed once)."""
    return so.baseline_errors(golden("spectral.npz"))


def dense_shapes(kind):
    """The T = 1 / 2 boundary, one tile of 32 frames and one frame into the second, three tiles with B > 1."""
    hop = HOP[kind]
    ls = [1, 159, 160, 161] + ([127, 128, 257] if kind != "stft" else [])
    shapes = [(1, L) for L in ls] + [(2, 32 * hop - 1), (2, 32 * hop), (3, 64 * hop + 1)]
    return [s for s in shapes if kind != "mel_reflect" or s[1] >= 257]  # (reflect needs 257 samples)


# ---------------------------------------------------------------------------- dense, against the oracle and the fixture
@pytest.mark.parametrize("kind", KINDS)
def test_dense_vs_oracle(kind, e_ref):
    m = make(kind)
    bound = MARGIN * e_ref[kind]
    worst = 0.0
    for i, (B, L) in enumerate(dense_shapes(kind)):
        x = synth_pcm(B, L, seed=800 + i)
        xg = x.cuda()
        y = dense(m, xg)
        assert y.shape == (B, 1 + L // HOP[kind], DIM[kind]) and y.is_contiguous() and y.dtype == torch.float32
        assert torch.equal(xg.cpu(), x)  # mutate_input False / Melspec: the waveform is left alone
        err = so.frame_rel_err(y.cpu().numpy(), oracle64(kind, x))
        print("%s (%d, %d): kernel vs fp64 %.3g (bound %.3g = %g x e_ref %.3g)" % (kind, B, L, err, bound, MARGIN, e_ref[kind]))
        worst = max(worst, err)
    assert worst <= bound, (kind, worst, bound)


@pytest.mark.parametrize("kind", KINDS)
def test_dense_vs_fixture(kind, golden, e_ref):
    g = golden("spectral.npz")
    m = make(kind)
    e = e_ref[kind]
    for tag, x in so.golden_cases(g):
        key = ("stft" if kind == "stft" else kind) + tag
        if key not in g.files:
            continue
        y = dense(m, x.cuda()).cpu().numpy()
        assert y.shape == g[key].shape
        e64, e32 = so.frame_rel_err(y, oracle64(kind, x)), so.frame_rel_err(y, g[key].astype(np.float64))
        print("%s case %s: kernel vs fp64 %.3g, vs the fp32 baseline %.3g" % (kind, tag, e64, e32))
        assert e64 <= MARGIN * e and e32 <= (MARGIN + 1.0) * e, (kind, tag, e64, e32, e)
        if tag == "_sil":
            assert not y.any()


def test_stft_without_emphasis_vs_oracle(e_ref):
    m = make("stft", with_emphasis=False)
    x = synth_pcm(2, 32 * 160 + 7, seed=820)
    err = so.frame_rel_err(m(x.cuda()).cpu().numpy(), so.stft_power(x.numpy(), with_emphasis=False))
    print("stft, no pre-emphasis: kernel vs fp64 %.3g" % err)
    assert err <= MARGIN * e_ref["stft"]


def test_stft_mutates_its_input_like_the_reference(golden):
    from asvspoof2021_air_amd.feature_extraction import STFT
    g = golden("spectral.npz")
    m = STFT(320, 160, 512, 16000).cuda()
    assert m.mutate_input
    x = synth_pcm(2, 4481, seed=int(g["seed0"]) + 3)
    xg = x.cuda()
    y = m(xg)
    want = o_lfcc.pre_emphasis_(x.numpy().copy())
    assert np.array_equal(xg.cpu().numpy(), want) and np.array_equal(want[:, :64], g["xmut3"])
    m.mutate_input = False
    xg2 = x.cuda()
    assert torch.equal(m(xg2), y) and torch.equal(xg2.cpu(), x)
    # no pre-emphasis: nothing to mutate
    m2 = STFT(320, 160, 512, 16000, with_emphasis=False).cuda()
    xg3 = x.cuda()
    m2(xg3)
    assert torch.equal(xg3.cpu(), x)


def test_melspec_forward_is_the_reference_layout():
    from asvspoof2021_air_amd.feature_extraction import Melspec
    m = Melspec().cuda()
    x = synth_pcm(3, 4000, seed=830).cuda()
    fr = m.forward_frames(x)
    bt = m.forward_batch(x)
    assert bt.shape == (3, 128, 32) and bt.is_contiguous() and torch.equal(bt, fr.transpose(1, 2))
    one = m(x)  # reads x[0] only (feature_extraction.py:175)
    assert one.shape == (128, 32) and torch.equal(one, bt[0])
    with pytest.raises(ValueError, match="257"):
        m.forward_batch(x[:, :256].contiguous())
    assert Melspec("constant").cuda().forward_batch(x[:, :256].contiguous()).shape == (3, 128, 3)


# ---------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("kind", KINDS)
def test_zero_input_int16_and_padded_layout_are_exact(kind):
    m = make(kind)
    hop = HOP[kind]
    for B, L in ((1, 300), (2, 32 * hop + 5)):
        assert not dense(m, torch.zeros(B, L).cuda()).any()
        assert not m.forward_padded(torch.zeros(B, L, dtype=torch.int16).cuda(), 40, None, "zero").any()
        s = (synth_pcm(B, L, seed=840 + B) * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
        xf = (s.float() / 32768.0).cuda()
        y = dense(m, xf)
        assert y.abs().max() > 0
        assert torch.equal(dense(m, s.cuda()), y)
        T = 1 + L // hop
        p = m.forward_padded(xf, T)
        assert p.shape == (B, DIM[kind], T) and p.is_contiguous() and torch.equal(p, y.transpose(1, 2))
        assert torch.equal(m.forward_padded(s.cuda(), T), p)


# ---------------------------------------------------------------------------- padded
def _want_padded(y, feat_len, padding, start):
    """oracle.pad on the dense (B, T, D) output -> (B, D, feat_len)."""
    rows = []
    for b in range(y.shape[0]):
        f = y[b:b + 1].cpu()
        T = f.shape[1]
        if T > feat_len:
            st = min(max(int(start[b]), 0), T - feat_len) if start is not None else 0
            f = f[:, st:st + feat_len]
        elif T < feat_len:
            f = o_pad.repeat_pad(f, feat_len) if padding == "repeat" else o_pad.zero_pad(f, feat_len)
        rows.append(f)
    return o_pad.to_model_input(torch.stack(rows))[:, 0]


@pytest.mark.parametrize("kind", KINDS)
def test_padded_equals_pad_of_dense(kind):
    m = make(kind)
    hop = HOP[kind]
    x = synth_pcm(2, 1600, seed=850).cuda()  # T = 11 / 13 into 48 frames
    y = dense(m, x)
    for padding in ("repeat", "zero"):
        got = m.forward_padded(x, 48, None, padding)
        assert got.shape == (2, DIM[kind], 48) and got.is_contiguous()
        assert torch.equal(got.cpu(), _want_padded(y, 48, padding, None)), padding
    x = synth_pcm(2, 9599, seed=851).cuda()  # T = 60 / 75 > 32: chopped, two or three tiles
    y = dense(m, x)
    for start in ([0, 7], [-5, 10 ** 6], None):
        st = None if start is None else torch.tensor(start, dtype=torch.int32).cuda()
        for padding in ("repeat", "zero"):
            assert torch.equal(m.forward_padded(x, 32, st, padding).cpu(), _want_padded(y, 32, padding, start)), (start, padding)
    T = 1 + 9599 // hop
    assert torch.equal(m.forward_padded(x, T, torch.tensor([3, 4], dtype=torch.int32).cuda(), "zero"), y.transpose(1, 2))
    for call in (lambda: m.forward_padded(x, 32, None, "silence"), lambda: m.forward_ragged(x, [9599, 9000], 32, None, "silence")):
        with pytest.raises(NotImplementedError, match="LFCC"):
            call()
    with pytest.raises(ValueError, match="Padding should be zero or repeat!"):
        m.forward_padded(x, 32, None, "edge")


# ---------------------------------------------------------------------------- ragged
LCAP, FEAT_LEN = 8000, 40
LENGTHS = {"stft": [1, 159, 160, 5121, 8000], "mel_constant": [1, 159, 160, 5121, 8000],
           "mel_reflect": [257, 383, 384, 5121, 8000]}  # (reflect: host-side lengths below 257 are refused)


def _ragged_batch(kind, dtype):
    lengths = LENGTHS[kind]
    x = synth_pcm(len(lengths), LCAP, seed=860)
    if dtype == torch.int16:
        x = (x * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
    for b, n in enumerate(lengths):
        x[b, n:] = float("nan") if dtype == torch.float32 else 32767
    return x.cuda(), lengths


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("kind", KINDS)
def test_ragged_rows_equal_each_utterance_alone(kind, dtype):
    m = make(kind)
    x, lengths = _ragged_batch(kind, dtype)
    keep = x.clone()
    ld = torch.tensor(lengths, dtype=torch.int32).cuda()
    for padding in ("repeat", "zero"):
        for start in (None, [0, 0, 0, 1, 7], [0, 0, 0, -3, 10 ** 6]):
            st = None if start is None else torch.tensor(start, dtype=torch.int32).cuda()
            want = torch.stack([m.forward_padded(x[b:b + 1, :n].contiguous(), FEAT_LEN, None if st is None else st[b:b + 1],
                                                 padding)[0] for b, n in enumerate(lengths)])
            assert bool(torch.isfinite(want).all())
            for given in (ld, lengths):
                got = m.forward_ragged(x, given, FEAT_LEN, st if given is ld else start, padding)
                assert got.shape == (len(lengths), DIM[kind], FEAT_LEN) and got.is_contiguous()
                for b in range(len(lengths)):
                    assert torch.equal(got[b], want[b]), (padding, start, b, lengths[b])
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(x.view(bits), keep.view(bits))
    if dtype == torch.float32:
        # a chopped row writes only its clamped window: the rows are what the dense output holds there
        y = dense(m, x[4:5].contiguous())
        T = y.shape[1]
        got = m.forward_ragged(x, ld, FEAT_LEN, torch.tensor([0, 0, 0, 0, 10 ** 6], dtype=torch.int32).cuda())
        assert torch.equal(got[4], y[0, T - FEAT_LEN:].t())


@pytest.mark.parametrize("kind", KINDS)
def test_ragged_lengths_are_checked_on_the_host_and_clamped_on_the_device(kind):
    from asvspoof2021_air_amd import _hip
    m = make(kind)
    lengths = LENGTHS[kind]
    x = synth_pcm(len(lengths), LCAP, seed=861).cuda()
    for bad in ([0] + lengths[1:], lengths[:-1] + [LCAP + 1], lengths[:-1], [float(v) for v in lengths]):
        with pytest.raises(ValueError):
            m.forward_ragged(x, bad, FEAT_LEN)
    with pytest.raises(ValueError):
        m.forward_ragged(x, torch.tensor(lengths[:-1], dtype=torch.int32).cuda(), FEAT_LEN)
    with pytest.raises(_hip.AirError):
        m.forward_ragged(x.cpu(), lengths, FEAT_LEN)
    want = m.forward_ragged(x, lengths, FEAT_LEN)
    over = torch.tensor(lengths[:-1] + [LCAP + 5], dtype=torch.int32).cuda()
    assert torch.equal(m.forward_ragged(x, over, FEAT_LEN), want)
    if kind == "mel_reflect":
        with pytest.raises(ValueError, match="257"):
            m.forward_ragged(x, [256] + lengths[1:], FEAT_LEN)
        with pytest.raises(ValueError, match="257"):
            m.forward_padded(x[:, :256].contiguous(), FEAT_LEN)
        # device-side lengths are used as they are: the reflected indices are clamped into the row
        short = torch.tensor([-3, 1, 2, 100, 256], dtype=torch.int32).cuda()
        assert bool(torch.isfinite(m.forward_ragged(x, short, FEAT_LEN)).all())
    else:
        under = torch.tensor([-3] + lengths[1:], dtype=torch.int32).cuda()
        assert torch.equal(m.forward_ragged(x, under, FEAT_LEN), m.forward_ragged(x, [1] + lengths[1:], FEAT_LEN))


# ---------------------------------------------------------------------------- dataset
ITEM_LENGTHS = [1600, 3000, 9599]  # T = 11, 19, 60 (STFT) / 13, 24, 75 (Melspec) against feat_len 48: two padded, one chopped


def _items():
    wav = synth_pcm(3, max(ITEM_LENGTHS), seed=870)
    return [("%05d_LA_T_%07d_%s_%s" % (i, 1000000 + i, "A%02d" % (1 + i) if i % 2 else "-", "spoof" if i % 2 else "bonafide"),
             wav[i, :n].clone()) for i, n in enumerate(ITEM_LENGTHS)]


@pytest.mark.parametrize("feature,dim", [("STFT", 257), ("Melspec", 128), ("LFCC", 60)])
def test_dataset_items_come_from_the_chosen_front_end(feature, dim):
    from asvspoof2021_air_amd import dataset as air_ds
    from asvspoof2021_air_amd.feature_extraction import LFCC, STFT, Melspec
    items = _items()
    m = {"STFT": lambda: STFT(320, 160, 512, 16000), "Melspec": Melspec, "LFCC": lambda: LFCC(320, 160, 512, 16000, 20)}[feature]().cuda()
    m.mutate_input = False
    ds = air_ds.ASVspoof2019("LA", None, feature=feature, source=air_ds.PCMSource(items), feat_len=48)
    assert type(ds.frontend) is type(m)
    want = []
    for i, (_, wav) in enumerate(items):
        np.random.seed(11 + i)
        feat, name, tag, label = ds[i]
        assert feat.shape == (1, 48, dim) and label == i % 2
        T = 1 + wav.shape[0] // m.fs
        np.random.seed(11 + i)
        st = torch.tensor([np.random.randint(T - 48)], dtype=torch.int32).cuda() if T > 48 else None
        want.append(m.forward_padded(wav.cuda().unsqueeze(0), 48, st).transpose(1, 2))
        assert torch.equal(feat, want[-1]), i
    # the batched path: one launch per length, the crop offsets drawn in item order
    ds2 = air_ds.ASVspoof2019("LA", None, feature=feature, source=air_ds.PCMSource(items), feat_len=48, return_pcm=True)
    np.random.seed(13)
    batch = ds2.collate_fn([ds2[i] for i in range(3)])
    assert batch[0].shape == (3, 1, 48, dim)
    np.random.seed(13)
    T = 1 + ITEM_LENGTHS[2] // m.fs
    st = torch.tensor([np.random.randint(T - 48)], dtype=torch.int32).cuda()
    assert torch.equal(batch[0][0], want[0]) and torch.equal(batch[0][1], want[1])
    assert torch.equal(batch[0][2], m.forward_padded(items[2][1].cuda().unsqueeze(0), 48, st).transpose(1, 2))
    # without pad / chop: the plain (1, T, D) features
    ds3 = air_ds.ASVspoof2019("LA", None, feature=feature, source=air_ds.PCMSource(items), pad_chop=False)
    assert ds3[0][0].shape == (1, 1 + 1600 // m.fs, dim)


def test_dataset_refuses_a_feature_without_a_front_end():
    from asvspoof2021_air_amd import dataset as air_ds
    with pytest.raises(ValueError, match="CQCC"):
        air_ds.ASVspoof2019("LA", None, feature="CQCC", source=air_ds.PCMSource(_items()), feat_len=48)
    with pytest.raises(ValueError, match="CQCC"):
        air_ds.ASVspoof2021LA_aug(feature="CQCC", ori_source=air_ds.PCMSource(_items()), aug_source=air_ds.PCMSource([]))


# ---------------------------------------------------------------------------- trainer
def _res2net():
    from asvspoof2021_air_amd.res2net import Res2Net, SEBottle2neck
    return fill_module_(Res2Net(SEBottle2neck, [3, 4, 6, 3], baseWidth=26, scale=4, num_classes=2)).cuda()


@pytest.mark.parametrize("kind", ["stft", "mel_reflect"])
def test_trainer_features_come_from_the_given_front_end(kind):
    from asvspoof2021_air_amd.resnet import ResNet
    from asvspoof2021_air_amd.train import Trainer
    fe = make(kind)
    tr = Trainer(ResNet(3, 256, resnet_type="18", nclasses=2), frontend=fe, feat_len=64)  # (features only: no model runs)
    assert tr.lfcc is fe
    pcm = synth_pcm(2, 8000, seed=880).cuda()
    f = tr.features(pcm)
    assert f.shape == (2, 1, DIM[kind], 64) and torch.equal(f[:, 0], fe.forward_padded(pcm, 64))
    ln = torch.tensor([8000, 3000], dtype=torch.int32).cuda()
    st = torch.tensor([2, 0], dtype=torch.int32).cuda()
    assert torch.equal(tr.features(pcm, st, ln)[:, 0], fe.forward_ragged(pcm, ln, 64, st))
    assert tr._graph_key(pcm, torch.zeros(2), False) != Trainer(ResNet(3, 256, resnet_type="18", nclasses=2), feat_len=64)._graph_key(
        pcm, torch.zeros(2), False)


def test_trainer_step_on_stft_features():
    """One train step of SE-Res2Net-50 on the 257-bin spectrogram made inside ``step`` equals ``step_features`` on the
    features made separately, from a second model filled alike."""
    from asvspoof2021_air_amd.feature_extraction import STFT
    from asvspoof2021_air_amd.train import Trainer
    pcm = synth_pcm(2, 8000, seed=881).cuda()
    labels = torch.tensor([0, 1]).cuda()
    tr1 = Trainer(_res2net(), add_loss=None, frontend=STFT(320, 160, 512, 16000), feat_len=64)
    tr2 = Trainer(_res2net(), add_loss=None, frontend=STFT(320, 160, 512, 16000), feat_len=64)
    l1 = tr1.step(pcm, labels)[0]
    l2 = tr2.step_features(tr2.features(pcm), labels)[0]
    torch.cuda.synchronize()
    assert np.isfinite(float(l1)) and float(l1) == float(l2)
    assert torch.equal(tr1.model.arena().flat, tr2.model.arena().flat)


def test_trainer_replays_and_scores_on_stft_features():
    """The captured step holds the given front-end: hipGraph replay of three steps equals the eager steps bit for bit, and
    ``score`` reads the same features."""
    from asvspoof2021_air_amd.feature_extraction import STFT
    from asvspoof2021_air_amd.train import Trainer
    pcm = synth_pcm(2, 8000, seed=882).cuda()
    labels = torch.tensor([1, 0]).cuda()
    runs = []
    for graph in (False, True):
        tr = Trainer(_res2net(), add_loss=None, frontend=STFT(320, 160, 512, 16000), feat_len=64)
        if graph:
            tr.enable_graph(True)
        losses = [float(tr.step(pcm, labels)[0]) for _ in range(4)]  # replay: two eager steps, the capture, one replay
        torch.cuda.synchronize()
        if graph:
            assert tr._graph is not None and "STFT" in tr._graph["key"]
        runs.append((losses, tr.model.arena().flat.clone()))
    assert all(np.isfinite(runs[0][0])) and runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert tr.score(pcm).shape == (2,)


# ---------------------------------------------------------------------------- one spectrum for LFCC and STFT
@pytest.mark.parametrize("emph", [True, False])
def test_lfcc_is_filterbank_log_dct_of_the_stft_kernels_spectrum(emph):
    """LFCC and STFT run the same pipeline up to the power spectrum (csrc/air_spec512.h): the static cepstra of the LFCC
    kernel are DCT(log10(P @ lfcc_fb + eps)) of the power P the STFT kernel writes for the same input, taken on the host in
    fp64 with the module's own ``lfcc_fb`` and ``l_dct.weight``.  Shapes: the tile edges of the two kernels (28 written
    frames per LFCC tile, 32 per STFT tile); white noise of amplitude 0.1, so that no filter sums near zero.  Tolerance:
    the one ``test_lfcc_gpu.py::test_lfcc_vs_oracle_shapes`` holds LFCC to against its oracle."""
    from asvspoof2021_air_amd.feature_extraction import LFCC, STFT
    tol = 3e-5
    lfcc = LFCC(320, 160, 512, 16000, 20, with_emphasis=emph, with_delta=False).cuda()
    stft = STFT(320, 160, 512, 16000, with_emphasis=emph).cuda()
    lfcc.mutate_input = stft.mutate_input = False
    fb, dct = lfcc.lfcc_fb.double().cpu(), lfcc.l_dct.weight.double().cpu()
    for L in (159, 28 * 160 - 1, 28 * 160, 32 * 160 - 1, 32 * 160, 64 * 160 + 1):
        x = (0.1 * torch.randn(2, L, generator=torch.Generator().manual_seed(900 + L))).cuda()
        got = lfcc(x)
        power = stft(x).double().cpu()
        want = torch.log10(power @ fb + torch.finfo(torch.float32).eps) @ dct.t()
        assert got.shape == want.shape == (2, 1 + L // 160, 20)
        err = float((got.double().cpu() - want).abs().max())
        print("emphasis %s, (2, %d): LFCC vs DCT(log10(STFT @ fb + eps)) %.3g (bound %.3g)" % (emph, L, err, tol))
        assert err <= tol, (emph, L, err)
