"""GPU: the IR channel augmentation on ragged batches (``air_ir_convolve_ragged`` through ``augment.ir_convolve(...,
lengths=)``) and the ragged train step with ``augment=ChannelAugment(...)``.

Two yardsticks.  The dense kernel, itself held to oracle/channel.py in tests/test_augment.py: row b of a ragged batch must
be, BIT FOR BIT, what the dense call gives for that utterance alone - both entry points run the same kernel bodies, the
row's length only moves the staging clamp and the store, so a differing bit is a bug.  And the oracle itself, per row."""
import functools

import numpy as np
import pytest
import torch

from oracle import channel as o_channel
from oracle.filler import fill_module_, synth_pcm

pytestmark = pytest.mark.gpu

LCAP = 9300
# around the direct form's block (2048 outputs), one overlap-save block (3072) and one pair of them (6144); 1 and the capacity
LENGTHS = [1, 777, 2048, 2049, 3072, 3073, 6144, 6145, 9300]
IDX = [1, 3, -1, 0, 2, -1, 0, 3, 1]  # -1: pass-through rows (a short and a long one)
# 37 and 2500 taps: direct form (2500: three tap chunks, more taps than most rows have samples); 128 and 1024: overlap-save
TAPS = (37, 128, 1024, 2500)


def _bank(H, n=4):
    rng = np.random.default_rng(LCAP + H)
    return torch.from_numpy((rng.standard_normal((n, H)) * np.exp(-np.arange(H) / max(H / 6.0, 1.0))).astype(np.float32))


def _pcm(lengths, cap, dtype=torch.float32, tail="zero", seed=9):
    """(B, cap) on the GPU; beyond its length a row is zero, or the worst value of its type."""
    x = synth_pcm(len(lengths), cap, seed=seed)
    if dtype == torch.int16:
        x = (x * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
    fill = 0 if tail == "zero" else (float("nan") if dtype == torch.float32 else 32767)
    for b, n in enumerate(lengths):
        x[b, n:] = fill
    return x.cuda()


@functools.lru_cache(maxsize=None)
def _case(H):
    """Inputs and the ragged results for one tap count, computed once: {normalize: (B, LCAP) on the host}."""
    from asvspoof2021_air_amd.augment import ir_convolve
    x, irs = _pcm(LENGTHS, LCAP), _bank(H).cuda()
    idx = torch.tensor(IDX, dtype=torch.int32).cuda()
    ld = torch.tensor(LENGTHS, dtype=torch.int32).cuda()
    keep = x.clone()
    got = {nz: ir_convolve(x, irs, idx, nz, lengths=ld) for nz in (False, True)}
    assert torch.equal(x, keep)  # the input is left as it was
    for y in got.values():
        assert y.dtype == torch.float32 and y.shape == (len(LENGTHS), LCAP) and y.is_contiguous()
    return dict(x=x, irs=irs, idx=idx, ld=ld, got={nz: y.cpu() for nz, y in got.items()})


@pytest.mark.parametrize("H", TAPS)
def test_ragged_rows_equal_the_dense_call_on_each_utterance_alone(H):
    from asvspoof2021_air_amd.augment import ir_convolve
    c = _case(H)
    for normalize in (False, True):
        got = c["got"][normalize]
        for b, n in enumerate(LENGTHS):
            alone = ir_convolve(c["x"][b:b + 1, :n].contiguous(), c["irs"], c["idx"][b:b + 1], normalize)[0].cpu()
            assert torch.equal(got[b, :n], alone), (H, normalize, b, n, float((got[b, :n] - alone).abs().max()))
            assert int(torch.count_nonzero(got[b, n:])) == 0, (H, normalize, b, n)
            if IDX[b] < 0:
                assert torch.equal(got[b, :n], c["x"][b, :n].cpu())  # untouched


@pytest.mark.parametrize("H", TAPS)
def test_ragged_rows_vs_oracle(H):
    """Each row against oracle/channel.py on that utterance alone, to the bound of tests/test_augment.py (2e-6 of the row's
    output scale, times sqrt(H) / 8 for long responses); normalised rows keep their own input peak."""
    c = _case(H)
    x, irs = c["x"].cpu().numpy(), c["irs"].cpu().numpy()
    for normalize in (False, True):
        got = c["got"][normalize].double().numpy()
        for b, n in enumerate(LENGTHS):
            want = o_channel.ir_convolve(x[b:b + 1, :n], irs, IDX[b:b + 1], normalize)[0]
            scale = np.abs(want).max()
            err = np.abs(got[b, :n] - want).max()
            print("H %d normalize %d row %d L %d: max |err| %.3g, scale %.3g" % (H, normalize, b, n, err, scale))
            assert err <= 2e-6 * scale * max(1.0, np.sqrt(H) / 8), (H, normalize, b, n, err, scale)
            assert not got[b, n:].any()
            if normalize and IDX[b] >= 0:
                px = np.abs(x[b, :n].astype(np.float64)).max()
                assert abs(np.abs(got[b, :n]).max() - px) <= 1e-6 * px, (H, b, n)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("H", TAPS)
def test_ragged_tail_is_never_read(H, dtype):
    """What lies behind an utterance's length (NaN / full scale) reaches no output; the input is left as it was."""
    from asvspoof2021_air_amd.augment import ir_convolve
    c = _case(H)
    clean, dirty = _pcm(LENGTHS, LCAP, dtype), _pcm(LENGTHS, LCAP, dtype, tail="worst")
    assert not torch.equal(clean.float().nan_to_num(7.0), dirty.float().nan_to_num(7.0))
    keep = dirty.clone()
    for normalize in (False, True):
        a = ir_convolve(clean, c["irs"], c["idx"], normalize, lengths=c["ld"])
        b = ir_convolve(dirty, c["irs"], c["idx"], normalize, lengths=c["ld"])
        assert bool(torch.isfinite(b).all())
        assert torch.equal(a, b)
        if dtype == torch.float32:
            assert torch.equal(a.cpu(), c["got"][normalize])
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(dirty.view(bits), keep.view(bits))


@pytest.mark.parametrize("H", TAPS)
def test_ragged_int16_equals_fp32_on_the_converted_samples(H):
    from asvspoof2021_air_amd.augment import ir_convolve
    c = _case(H)
    x16 = _pcm(LENGTHS, LCAP, torch.int16)
    xf = x16.float() / 32768.0  # exact
    for normalize in (False, True):
        a = ir_convolve(x16, c["irs"], c["idx"], normalize, lengths=c["ld"])
        b = ir_convolve(xf, c["irs"], c["idx"], normalize, lengths=c["ld"])
        assert a.dtype == torch.float32 and torch.equal(a, b), (H, normalize, float((a - b).abs().max()))
        for r in (2, 5):  # pass-through rows: the converted samples, the tail zero
            assert torch.equal(a[r, :LENGTHS[r]], xf[r, :LENGTHS[r]]) and int(torch.count_nonzero(a[r, LENGTHS[r]:])) == 0


def test_ragged_fft_form_equals_direct_form():
    """Option IR_FFT on a ragged batch: both routes serve it and agree to fp32 FFT rounding (4e-6 of the output scale,
    tests/test_augment.py::test_fft_form_equals_direct_form); pass-through rows are bit-identical in both."""
    from asvspoof2021_air_amd import _hip
    from asvspoof2021_air_amd.augment import ir_convolve
    cap, H = 7000, 300
    lengths = [min(n, cap) for n in LENGTHS]
    x = _pcm(lengths, cap, seed=3)
    rng = np.random.default_rng(cap)
    irs = torch.from_numpy((rng.standard_normal((4, H)) * np.exp(-np.arange(H) / (H / 6.0))).astype(np.float32)).cuda()
    idx = torch.tensor(IDX, dtype=torch.int32).cuda()
    ld = torch.tensor(lengths, dtype=torch.int32).cuda()
    out = {}
    for mode in (0, 1):
        old = _hip.set_option("IR_FFT", mode)
        try:
            out[mode] = [ir_convolve(x, irs, idx, nz, lengths=ld).cpu() for nz in (False, True)]
        finally:
            _hip.set_option("IR_FFT", old)
    for a, b in zip(out[1], out[0]):
        scale = float(b.abs().max())
        print("FFT vs direct: max |diff| %.3g, scale %.3g" % (float((a - b).abs().max()), scale))
        assert not torch.equal(a, b)  # (two routes did run)
        assert float((a - b).abs().max()) <= 4e-6 * scale
        for r, n in enumerate(lengths):
            assert int(torch.count_nonzero(a[r, n:])) == 0 and int(torch.count_nonzero(b[r, n:])) == 0
            if IDX[r] < 0:
                assert torch.equal(a[r], x[r].cpu()) and torch.equal(b[r], x[r].cpu())


def test_ragged_lengths_validation():
    """Host lengths are checked before anything is launched: ``out`` stays as it was."""
    from asvspoof2021_air_amd.augment import ChannelAugment, ir_convolve
    c = _case(37)
    out = torch.full((len(LENGTHS), LCAP), 7.0, device="cuda")
    for bad in (LENGTHS[:-1],                               # wrong count
                [0] + LENGTHS[1:],                          # a length of 0
                LENGTHS[:-1] + [LCAP + 1],                  # above the capacity
                [float(n) for n in LENGTHS],                # float lengths
                torch.tensor(LENGTHS, dtype=torch.float32)):
        with pytest.raises(ValueError):
            ir_convolve(c["x"], c["irs"], c["idx"], True, out=out, lengths=bad)
    with pytest.raises(ValueError):
        ir_convolve(c["x"], c["irs"], c["idx"], True, out=out, lengths=c["ld"][:-1])  # a device tensor of the wrong count
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    aug = ChannelAugment(irs=c["irs"], p=0.5, seed=1)
    state = aug.rng.bit_generator.state
    with pytest.raises(ValueError):
        aug(c["x"], lengths=[0] + LENGTHS[1:])
    assert aug.rng.bit_generator.state == state  # a refused batch draws nothing
    # host lists, host tensors and device tensors agree; ``out`` is used
    want = c["got"][True]
    assert torch.equal(ir_convolve(c["x"], c["irs"], c["idx"], True, lengths=LENGTHS).cpu(), want)
    assert torch.equal(ir_convolve(c["x"], c["irs"], c["idx"], True, lengths=torch.tensor(LENGTHS)).cpu(), want)
    assert ir_convolve(c["x"], c["irs"], c["idx"], True, out=out, lengths=c["ld"]) is out and torch.equal(out.cpu(), want)


# ---------------------------------------------------------------------------- trainer
B, CAP = 4, 32000  # T up to 201 > feat_len 96
LENS = [[32000, 159, 20000, 15359], [4480, 32000, 16000, 31999], [25000, 12000, 32000, 300]]
STARTS = [[60, 0, 11, 0], [0, 105, 3, 1], [33, 0, 7, 0]]  # non-zero on every long row (T_b > 96)


def _trainer(graph, augment=None, feat_len=96, seed=4242):
    """The model, head and seeds of the ragged replay test of tests/test_lfcc_ragged_gpu.py."""
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.resnet import ResNet
    from asvspoof2021_air_amd.train import Trainer
    m = ResNet(3, 256, resnet_type="18", nclasses=2)
    fill_module_(m)
    m = m.cuda()
    m._noise_seed = seed  # device noise ON: the replay has to draw what the eager step draws
    lossm = AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)
    fill_module_(lossm)
    tr = Trainer(m, loss_module=lossm, feat_len=feat_len, augment=augment)
    if graph:
        tr.enable_graph(segments=False)
    else:
        m.overlap_wgrad = False  # the capture is one chain; same launches eagerly
    return m, tr


def _batches():
    """Three ragged batches; the second one arrives as 16-bit PCM."""
    out = []
    for i in range(3):
        pcm = _pcm(LENS[i], CAP, torch.int16 if i == 1 else torch.float32, seed=500 + i)
        out.append((pcm, ((torch.arange(B) + i) % 3 != 0).long().cuda(),
                    torch.tensor(STARTS[i], dtype=torch.int32).cuda(), torch.tensor(LENS[i], dtype=torch.int32).cuda()))
    return out


def test_ragged_step_with_augment_equals_the_hand_augmented_step_eager_and_replayed():
    """Trainer(augment=ChannelAugment) stepping on ragged batches == a trainer without augment stepping on the batches
    augmented by hand with the same seed, eagerly and on hipGraph replay: ONE ragged capture of fp32 (B, Lcap) serves
    every set of lengths and both input dtypes."""
    from asvspoof2021_air_amd.augment import ChannelAugment
    batches = _batches()
    ends = []
    for mode in ("hand", "eager", "graph"):
        aug = ChannelAugment(p=0.5, seed=1)
        m, tr = _trainer(mode == "graph", None if mode == "hand" else aug)
        losses, capture, drawn = [], None, []
        for i in range(5):  # two eager warm-up steps, the capture on batch 2, then batches 0 and 1 on replay
            pcm, lab, st, ln = batches[i % 3]
            if mode == "hand":
                pcm = aug(pcm, lengths=ln)
                assert pcm.dtype == torch.float32 and int(torch.count_nonzero(pcm[1, ln[1]:])) == 0
            losses.append(tr.step(pcm, lab, start=st, lengths=ln)[0].item())
            if mode == "graph" and i == 2:
                capture = tr._graph
                assert capture is not None and "ragged" in capture["key"]
                assert capture["pcm"].dtype == torch.float32 and capture["pcm"].shape == (B, CAP)
        torch.cuda.synchronize()
        if mode == "graph":
            assert tr._graph is capture and len(capture["graphs"]) == 1  # one capture, one graph object
            assert capture["lengths"].tolist() == LENS[1] and capture["start"].tolist() == STARTS[1]
        else:
            assert tr._graph is None
        ends.append((losses, m.arena().flat.clone(), tr.loss.center.detach().clone(), int(m._noise_ctr.item()),
                     aug.rng.bit_generator.state))
    (l0, w0, c0, k0, r0), (l1, w1, c1, k1, r1), (l2, w2, c2, k2, r2) = ends
    assert all(np.isfinite(l0)) and l0 == l1 == l2
    assert torch.equal(w0, w1) and torch.equal(c0, c1) and k0 == k1 > 0 and r0 == r1
    assert torch.equal(w0, w2) and torch.equal(c0, c2) and k0 == k2 and r0 == r2


def test_features_eval_and_score_do_not_augment_and_the_adversarial_step_takes_lengths():
    from asvspoof2021_air_amd.adversarial import AdversarialTrainer
    from asvspoof2021_air_amd.augment import ChannelAugment
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.resnet import ResNet
    pcm, lab, st, ln = _batches()[0]
    m, tr = _trainer(False)
    m.set_attention_noise(None)  # (the per-call noise off: two calls on the same features give the same scores)
    want = (tr.features(pcm, st, ln), tr.eval_batch(pcm, lab, start=st, lengths=ln), tr.score(pcm, start=st, lengths=ln))
    tr.augment = ChannelAugment(p=0.5, seed=1)
    state = tr.augment.rng.bit_generator.state
    got = (tr.features(pcm, st, ln), tr.eval_batch(pcm, lab, start=st, lengths=ln), tr.score(pcm, start=st, lengths=ln))
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    assert torch.equal(got[1][0], want[1][0]) and torch.equal(got[1][1], want[1][1])
    assert tr.augment.rng.bit_generator.state == state  # as without lengths: only step augments

    # AdversarialTrainer.step(..., channels=, lengths=): its front-end sees the batch augmented over each row's own samples
    am = ResNet(3, 256, resnet_type="18", nclasses=2)
    fill_module_(am)
    am.set_attention_noise(None)
    lossm = AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)
    fill_module_(lossm)
    atr = AdversarialTrainer(am, 5, loss_module=lossm, feat_len=96, augment=ChannelAugment(p=0.5, seed=1))
    seen = []
    features = atr.features
    atr.features = lambda *a, **k: seen.append(features(*a, **k)) or seen[-1]
    loss, _ = atr.step(pcm, lab, channels=torch.tensor([0, 3, 1, 4]).cuda(), start=st, lengths=ln.tolist())
    assert bool(torch.isfinite(loss).all()) and len(seen) == 1
    hand = ChannelAugment(p=0.5, seed=1)(pcm, lengths=ln)
    assert not torch.equal(hand, pcm)
    assert torch.equal(seen[0], features(hand, st, ln))
    atr.augment = lambda x: x  # an augment that is not told the lengths is still refused
    with pytest.raises(NotImplementedError):
        atr.step(pcm, lab, channels=torch.tensor([0, 3, 1, 4]).cuda(), lengths=ln)
