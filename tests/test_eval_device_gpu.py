"""GPU: the device EER / min t-DCF (csrc/eval_metrics.hip), Trainer.evaluate and end-synchronised scoring against the
host code they replace.  Every comparison is ``==`` on float64 values and on indices: the device sorts integer keys
and counts, and the two fp64 divisions per curve point are correctly rounded on both sides, so there is no tolerance
to choose - a result is the host's or an error.

Sizes: 1 + 1 and 2 + 1 trials; 2^k - 1, 2^k, 2^k + 1 for k = 8, 10, 12, 13, 14, 16 (the sort pads to a power of two
with sentinels; a workgroup sorts 4096 = 2^12 keys in LDS, the scan walks blocks of 4096 curve points); 71,237 (the
ASVspoof 2019 LA evaluation set); 2^20 (the limit)."""
import numpy as np
import pytest
import torch

from oracle.filler import fill_module_, synth_feat, synth_pcm

pytestmark = pytest.mark.gpu

KINDS = ("normal", "ties", "equal", "separable", "inverted", "zeros", "inf", "denormal")
POW_SIZES = [2 ** k + d for k in (8, 10, 12, 13, 14, 16) for d in (-1, 0, 1)]
SIZES = [2, 3] + POW_SIZES + [71237]
LIMIT = 1 << 20


def make_labels(n, mix, rng):
    """0 = bona fide, 1 = spoof, shuffled; ``mix``: "1:9" (about), "1:rest" (one bona fide), "rest:1" (one spoof)."""
    if n == 2:
        n_tar = 1
    elif n == 3:
        n_tar = 2
    else:
        n_tar = {"1:9": max(1, n // 10), "1:rest": 1, "rest:1": n - 1}[mix]
    lab = np.ones(n, dtype=np.int64)
    lab[:n_tar] = 0
    rng.shuffle(lab)
    return lab


def make_scores(kind, lab, rng):
    n = lab.size
    x = rng.normal(0.0, 1.0, n)
    sign = np.where(lab == 0, 1.0, -1.0)
    if kind == "normal":
        s = x + sign
    elif kind == "ties":
        s = np.round(2.0 * (x + sign))
    elif kind == "equal":
        s = np.full(n, 0.5)
    elif kind == "separable":
        s = sign * (2.0 + np.abs(x))
    elif kind == "inverted":
        s = x - sign
    elif kind == "zeros":
        s = rng.choice(np.array([-0.0, 0.0, -0.0, 0.0, -1.0, 1.0]), n)
    elif kind == "inf":
        s = x + sign
        s[rng.random(n) < 0.05] = np.inf
        s[rng.random(n) < 0.05] = -np.inf
    elif kind == "denormal":
        s = rng.integers(-6, 7, n).astype(np.float64) * 2.0 ** -149 * np.where(rng.random(n) < 0.5, 1.0, 4096.0)
    s = s.astype(np.float32)
    if kind == "denormal":
        assert np.any((s != 0) & (np.abs(s) < np.finfo(np.float32).tiny))
    return s


def host_eer(s, lab, negate=False):
    from asvspoof2021_air_amd.eval_metrics import compute_eer
    s = s.astype(np.float64)
    s = -s if negate else s
    return compute_eer(s[lab == 0], s[lab != 0])


def dev(s, lab):
    return torch.from_numpy(s).cuda(), torch.from_numpy(lab).cuda()


def check_eer(s, lab, tag):
    from asvspoof2021_air_amd import eval_metrics as em
    ds, dl = dev(s, lab)
    pend = [em.compute_eer_device(ds, dl), em.compute_eer_device(ds, dl, negate=True), em.eer_both_polarities_device(ds, dl)]
    want = [host_eer(s, lab), host_eer(s, lab, True)]
    got = [p.result() for p in pend]
    assert got[0] == want[0], (tag, "as given", got[0], want[0])
    assert got[1] == want[1], (tag, "negated", got[1], want[1])
    assert got[2] == em.eer_both_polarities(s.astype(np.float64), lab) == min(want[0][0], want[1][0]), (tag, "both")


def test_sizes_straddle_the_sort_block():
    """The sizes above were chosen for a 4096-key LDS block: a library built with another block needs its size +- 1."""
    from asvspoof2021_air_amd import _hip, ops
    block = _hip.lib().air_eval_sort_block()
    assert {block - 1, block, block + 1} <= set(SIZES)
    assert _hip.lib().air_eval_max_trials() == ops.EVAL_MAX_TRIALS == LIMIT


@pytest.mark.parametrize("n", SIZES)
def test_eer_equals_host(n):
    for i, kind in enumerate(KINDS):
        rng = np.random.default_rng(1000 * n + i)
        lab = make_labels(n, "1:9", rng)
        check_eer(make_scores(kind, lab, rng), lab, (kind, n))


@pytest.mark.parametrize("mix", ["1:rest", "rest:1"])
@pytest.mark.parametrize("n", SIZES[2:])
def test_eer_equals_host_lopsided_classes(n, mix):
    for i, kind in enumerate(("normal", "ties", "zeros")):
        rng = np.random.default_rng(77 * n + i)
        lab = make_labels(n, mix, rng)
        check_eer(make_scores(kind, lab, rng), lab, (kind, n, mix))


@pytest.mark.parametrize("kind, mix", [("normal", "1:9"), ("ties", "1:9"), ("ties", "1:rest"), ("normal", "rest:1")])
def test_eer_equals_host_at_the_limit(kind, mix):
    rng = np.random.default_rng(20)
    lab = make_labels(LIMIT, mix, rng)
    check_eer(make_scores(kind, lab, rng), lab, (kind, LIMIT, mix))


@pytest.mark.parametrize("n", [1, 2, 4095, 4096, 4097, 8193, 71237])
def test_sorted_keys_equal_numpy_sort(n):
    """The sort alone: the device's keys are np.sort of the host's keys; the whole chain's record counts the classes."""
    from asvspoof2021_air_amd import ops
    rng = np.random.default_rng(n)
    lab = rng.integers(0, 2, n).astype(np.int64) * rng.integers(1, 9, n)  # any nonzero label is a spoof
    s = make_scores("ties" if n % 2 else "normal", np.minimum(lab, 1), rng)
    s[::7] = -0.0
    for negate in (False, True):
        for ldt in (torch.int64, torch.int32):
            ds, dl = torch.from_numpy(s).cuda(), torch.from_numpy(lab).cuda().to(ldt)
            keys = ops.eval_sorted_keys(ds, dl, negate=negate)
            v = (-s if negate else s) + np.float32(0.0)  # -0.0 -> +0.0
            u = v.view(np.uint32).astype(np.uint64)
            o = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
            want = np.sort((o << np.uint64(9)) | ((lab != 0).astype(np.uint64) << np.uint64(8)))
            assert np.array_equal(keys.cpu().numpy().view(np.uint64), want), (n, negate, ldt)
            rec = torch.empty(ops.EVAL_RECORD_WORDS, dtype=torch.int32, device="cuda")
            ops.eval_det_min(ds, dl, rec, torch.empty(ops.eval_workspace_bytes(n), dtype=torch.uint8, device="cuda"), negate=negate)
            assert rec.cpu().numpy().view(np.uint32)[:4].tolist() == [int((lab == 0).sum()), int((lab != 0).sum()), 0, 0]


@pytest.fixture(scope="module")
def asv(golden):
    from asvspoof2021_air_amd.eval_metrics import asvspoof19_cost_model
    return tuple(golden("tdcf.npz")["asv_rates"]) + (asvspoof19_cost_model(),)


@pytest.mark.parametrize("n", [3, 255, 1025, 4096, 4097, 8193, 16385, 65537, 71237])
def test_min_tdcf_equals_host(n, asv):
    from asvspoof2021_air_amd import eval_metrics as em
    for i, (kind, mix) in enumerate((("normal", "1:9"), ("ties", "1:9"), ("separable", "1:9"), ("inverted", "rest:1"),
                                     ("denormal", "1:rest"), ("zeros", "1:9"))):
        rng = np.random.default_rng(31 * n + i)
        lab = make_labels(n, mix, rng)
        s = make_scores(kind, lab, rng)
        if np.unique(s).size < 3:
            continue
        ds, dl = dev(s, lab)
        for negate in (False, True):
            h = (-s if negate else s).astype(np.float64)
            curve, _ = em.compute_tDCF(h[lab == 0], h[lab != 0], *asv)
            k = int(np.argmin(curve))
            got = em.min_tdcf_device(ds, dl, *asv, negate=negate).result()
            assert got == (curve[k], k), (kind, n, mix, negate, got, (curve[k], k))


def test_min_tdcf_on_the_fixture_scores(golden, asv):
    from asvspoof2021_air_amd import eval_metrics as em
    g = golden("tdcf.npz")
    s = np.concatenate((g["bona_cm"], g["spoof_cm"])).astype(np.float32)
    lab = np.concatenate((np.zeros(g["bona_cm"].size, np.int64), np.ones(g["spoof_cm"].size, np.int64)))
    ds, dl = dev(s, lab)
    for tag, negate in (("pos", False), ("neg", True)):
        assert em.min_tdcf_device(ds, dl, *asv, negate=negate).result() == (float(g["min_" + tag]), int(g["argmin_" + tag]))
        assert em.compute_eer_device(ds, dl, negate=negate).result() == tuple(g["eer_" + tag])


def test_errors(asv):
    from asvspoof2021_air_amd import eval_metrics as em
    rng = np.random.default_rng(5)
    lab = make_labels(5000, "1:9", rng)
    s = make_scores("normal", lab, rng)
    bad = s.copy()
    bad[4321] = np.nan
    for fn in (em.compute_eer_device, em.eer_both_polarities_device, lambda a, b: em.min_tdcf_device(a, b, *asv)):
        with pytest.raises(ValueError):
            fn(*dev(bad, lab)).result()
        for only in (0, 1):  # an empty class
            with pytest.raises(ValueError):
                fn(*dev(s, np.full_like(lab, only))).result()
        with pytest.raises(ValueError):
            fn(torch.zeros(LIMIT + 1, device="cuda"), torch.zeros(LIMIT + 1, dtype=torch.int64, device="cuda"))
    for kind in ("inf", "equal"):  # compute_tDCF refuses +-inf and fewer than three distinct scores
        with pytest.raises(ValueError):
            em.min_tdcf_device(*dev(make_scores(kind, lab, rng), lab), *asv).result()
    two = np.where(rng.random(lab.size) < 0.5, -0.0, 1.0).astype(np.float32)
    two[::2] = np.abs(two[::2])  # {-0.0, +0.0, 1.0}: two distinct scores
    with pytest.raises(ValueError):
        em.min_tdcf_device(*dev(two, lab), *asv).result()
    with pytest.raises(ValueError):  # priors that do not sum to one are refused before anything is enqueued
        em.min_tdcf_device(*dev(s, lab), asv[0], asv[1], asv[2], dict(asv[3], Ptar=0.5))
    with pytest.raises(ValueError):
        em.compute_eer_device(torch.from_numpy(s), torch.from_numpy(lab))  # host tensors: compute_eer is the host path
    assert em.compute_eer_device(*dev(s, lab)).result() == host_eer(s, lab)


def test_both_polarities_replay_in_a_graph():
    """After one warm-up call the both-polarities metric is captured in a single-stream graph and replayed on three
    score sets copied into its static input: nothing inside synchronises or allocates outside the capture's pool."""
    from asvspoof2021_air_amd import eval_metrics as em
    n = 10007
    rng = np.random.default_rng(9)
    sets = []
    for kind, mix in (("normal", "1:9"), ("ties", "rest:1"), ("inverted", "1:9")):
        lab = make_labels(n, mix, rng)
        sets.append((make_scores(kind, lab, rng), lab))
    ss, sl = dev(*sets[0])
    assert em.eer_both_polarities_device(ss, sl).result() == em.eer_both_polarities(sets[0][0].astype(np.float64), sets[0][1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pending = em.eer_both_polarities_device(ss, sl)
    for s, lab in reversed(sets):
        ss.copy_(torch.from_numpy(s))
        sl.copy_(torch.from_numpy(lab))
        graph.replay()
        assert pending.result(refresh=True) == em.eer_both_polarities(s.astype(np.float64), lab)


# ------------------------------------------------------------------ Trainer.evaluate
def _model(kind):
    if kind == "resnet":
        from asvspoof2021_air_amd.resnet import ResNet
        m = ResNet(3, 256, resnet_type="18", nclasses=2)
        fill_module_(m)
        m.set_attention_noise(None)  # two passes see the same arithmetic
        return m
    from asvspoof2021_air_amd.ecapa_tdnn import Bottle2neck, Res2Net2
    m = Res2Net2(Bottle2neck, C=512, model_scale=8, nOut=2, n_mels=60)
    fill_module_(m)
    return m


@pytest.mark.parametrize("head", ["ang_iso", None])
@pytest.mark.parametrize("kind", ["ecapa", "resnet"])
def test_evaluate_equals_the_per_batch_loop(tmp_path, kind, head):
    from asvspoof2021_air_amd import eval_metrics as em
    from asvspoof2021_air_amd.train import Trainer
    tr = Trainer(_model(kind), feat_len=128, ecapa=(kind == "ecapa"), add_loss=head)
    if tr.loss is not None:
        fill_module_(tr.loss)
    B = 4
    batches = [(synth_pcm(B, 16000, seed=500 + i).cuda(), ((torch.arange(B) + i) % 3 != 0).long().cuda()) for i in range(6)]
    # the loop as the reference writes it (main_train.py:526-575, :662-671): .item() per batch
    losses, scores, labels = [], [], []
    for pcm, lab in batches:
        loss, score = tr.eval_batch(pcm, lab)
        losses.append(loss.item())
        scores.append(score.cpu().numpy())
        labels.append(lab.cpu().numpy())
    want_loss = np.nanmean(losses)
    want_eer = em.eer_both_polarities(np.concatenate(scores), np.concatenate(labels))
    tr.set_out_fold(str(tmp_path / "loop"))
    tr.log_eval(3, losses, want_eer, name="dev_loss.log")
    want_line = (tmp_path / "loop" / "dev_loss.log").read_text()

    tr.set_out_fold(str(tmp_path / "pass"))
    for given in (batches, iter(batches)):  # preallocated from len(), and grown by device-side copies
        out = tr.evaluate(given, epoch_num=3, log="dev_loss.log")
        assert out.loss == want_loss and out.eer == want_eer and out.min_tdcf is None
        assert np.array_equal(out.scores.cpu().numpy(), np.concatenate(scores))
        assert np.array_equal(out.labels.cpu().numpy(), np.concatenate(labels))
    assert (tmp_path / "pass" / "dev_loss.log").read_text() == want_line * 2
    assert tr.evaluate(batches, capacity=5).eer == want_eer  # a capacity that is outgrown
    assert not (tmp_path / "pass" / "test_loss.log").exists()
    with pytest.raises(ValueError):
        tr.evaluate(batches, log="train_loss.log")


def test_evaluate_with_tdcf(golden):
    """min t-DCF of the pass: the polarity with the lower EER (evaluate_tDCF_asvspoof19.py:53-67), the host port's value."""
    from asvspoof2021_air_amd import eval_metrics as em
    from asvspoof2021_air_amd.train import Trainer
    tr = Trainer(_model("resnet"), feat_len=128)
    fill_module_(tr.loss)
    rates = tuple(golden("tdcf.npz")["asv_rates"])
    batches = [(synth_pcm(4, 16000, seed=600 + i).cuda(), ((torch.arange(4) + i) % 3 != 0).long().cuda()) for i in range(6)]
    out = tr.evaluate(batches, tdcf=rates + (em.asvspoof19_cost_model(),))
    s, lab = out.scores.cpu().numpy().astype(np.float64), out.labels.cpu().numpy()
    eers = [em.compute_eer(sg * s[lab == 0], sg * s[lab == 1])[0] for sg in (1.0, -1.0)]
    sg = 1.0 if eers[0] < eers[1] else -1.0
    curve, _ = em.compute_tDCF(sg * s[lab == 0], sg * s[lab == 1], *rates, em.asvspoof19_cost_model())
    assert out.min_tdcf == curve[np.argmin(curve)]
    assert out.eer == min(eers)
    with pytest.raises(ValueError):  # refused before the pass
        tr.evaluate(batches, tdcf=(rates[0], rates[1], None, em.asvspoof19_cost_model()))


# ------------------------------------------------------------------ test_on_dataset(sync="end")
@pytest.mark.parametrize("bs", [1, 3])
@pytest.mark.parametrize("task", ["19eval", "LA"])
def test_end_synchronised_scoring_writes_the_same_bytes(tmp_path, task, bs):
    from asvspoof2021_air_amd.generate_score import test_on_dataset
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    model = _model("resnet").cuda()
    lossm = AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)
    fill_module_(lossm)
    lossm = lossm.cuda()
    n = 7
    feats = synth_feat((n, 1, 96, 60), seed=11)
    names = ["LA_E_%07d" % (1000 + i) for i in range(n)]
    labels = torch.tensor([i % 3 == 0 for i in range(n)]).long()
    tags = torch.zeros(n)
    if "19" in task:
        data = [(feats[i:i + bs], names[i:i + bs], tags[i:i + bs], labels[i:i + bs]) for i in range(0, n, bs)]
    else:
        data = [(feats[i:i + bs], names[i:i + bs]) for i in range(0, n, bs)]
    for j, kw in enumerate((dict(), dict(keep_dataset_labels=True), dict(use_graph=True))):
        fa, fb = tmp_path / ("batch%d.txt" % j), tmp_path / ("end%d.txt" % j)
        assert test_on_dataset(model, data, str(fa), lossm, "ocsoftmax", task=task, **kw) == n
        assert test_on_dataset(model, iter(data), str(fb), lossm, "ocsoftmax", task=task, sync="end", **kw) == n
        assert fa.read_bytes() == fb.read_bytes() and len(fa.read_text().splitlines()) == n
    with pytest.raises(ValueError):
        test_on_dataset(model, data, str(tmp_path / "x.txt"), lossm, "ocsoftmax", task=task, sync="never")
