"""GPU: csrc/score_fusion.hip (ops.score_fuse) against the numpy oracle tests/fusion_oracle.py, which
tests/test_score_fusion_cpu.py pins to the reference's pandas results; score_fusion.fuse_device against the recorded
reference and the host metrics; the ensemble scoring pass against test_on_dataset per model and the file-based fusion.
Every comparison is on bits and bytes: the kernel performs the oracle's float32 operations one by one."""
import ctypes

import numpy as np
import pytest
import torch

import fusion_oracle as fo
from oracle.filler import fill_module_, synth_feat, synth_pcm

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 16)
NS = (1, 63, 64, 65, 257, 4097)  # a wave and its neighbours, a block (256) + 1, 16 blocks + 1: a ragged last block


def draw(K, L, seed):
    """Scores of mixed sign and widely different magnitude, with -0.0, +-inf and NaN among them."""
    rng = np.random.default_rng(seed)
    s = (rng.normal(size=(K, L)) * 10.0 ** rng.uniform(-3, 6, (K, L))).astype(np.float32)
    flat = s.reshape(-1)
    for v, every in ((-0.0, 11), (np.inf, 53), (-np.inf, 59), (np.nan, 31)):
        flat[rng.integers(0, every)::every] = v
    return s


def draw_index(K, L, N, seed):
    """Permuted rows with absent entries; trial 0 (and every 97th) is absent from every system."""
    rng = np.random.default_rng(seed)
    index = np.full((K, N), -1, dtype=np.int32)
    for k in range(K):
        n_have = min(L, N)
        trials = rng.permutation(N)[:n_have]
        index[k, trials] = rng.permutation(L)[:n_have]
        index[k, rng.random(N) < 0.15] = -1
    index[:, ::97] = -1
    return index


def run(scores, index, weights, mode, want_counts=True):
    from asvspoof2021_air_amd import ops
    N = scores.shape[1] if index is None else index.shape[1]
    counts = torch.full((N,), -7, dtype=torch.int32, device="cuda") if want_counts else None
    out = ops.score_fuse(scores, None if index is None else torch.from_numpy(index).cuda(),
                         None if weights is None else torch.from_numpy(weights).cuda(), mode, n_present=counts)
    return out.cpu().numpy(), None if counts is None else counts.cpu().numpy()


@pytest.mark.parametrize("K", KS)
def test_kernel_equals_the_oracle(K):
    for N in NS:
        host = draw(K, N, 100 * K + N)
        dev = torch.from_numpy(host).cuda()
        wide = torch.full((K, N + 37), 123.0, device="cuda")  # rows of a wider buffer: a row stride that is not N
        wide[:, :N] = dev
        weights = (np.random.default_rng(N).uniform(0.05, 1.0, K)).astype(np.float32)
        index = draw_index(K, N, N + 5, 7 * K + N)
        assert (index >= 0).any() or N == 1
        for mode in ("sum", "mean"):
            for w in (None, weights):
                for given in (dev, wide[:, :N]):
                    for ix in (None, index):
                        want, want_n = fo.fuse(host, ix, w, mode)
                        got, got_n = run(given, ix, w, mode)
                        tag = (K, N, mode, w is not None, given is not dev, ix is not None)
                        assert fo.same_bits(got, fo.bits(want)), tag
                        assert np.array_equal(got_n.astype(np.uint32), want_n), tag
                if N == 65:
                    got, none = run(dev, None, w, mode, want_counts=False)
                    assert none is None and fo.same_bits(got, fo.bits(fo.fuse(host, None, w, mode)[0]))
        want, want_n = fo.fuse(host, index, None, "sum")
        assert np.isnan(want[0]) and want_n[0] == 0  # the all-absent trial: NaN, count 0


def test_kernel_on_the_fixture(golden, tmp_path):
    """The reference's own inputs through the gather path: the recorded pandas bits, cancellation rows, the NaN that is
    skipped and the -inf included."""
    from asvspoof2021_air_amd import score_fusion as sf
    g = golden("fusion.npz")
    frames = [sf.read_file(p) for p in fo.fixture_inputs(g, tmp_path)]
    matrix, index, keys, _ = sf.align(frames)
    rows = np.zeros((3, max(len(f) for f in frames)), dtype=np.float32)
    for k, f in enumerate(frames):
        rows[k, :len(f)] = f.score
    weights = np.asarray(sf.cal_weight(g["eers"].tolist()), dtype=np.float64).astype(np.float32)
    aligned = np.where(index >= 0, np.arange(index.shape[1], dtype=np.int32), -1).astype(np.int32)
    for method, mode, w in (("avg", "sum", None), ("wght", "mean", weights)):
        want_rows, want = fo.fixture_rows(g, method)
        assert keys == want_rows
        assert fo.same_bits(run(torch.from_numpy(rows).cuda(), index, w, mode)[0], want), method
        assert fo.same_bits(run(torch.from_numpy(matrix).cuda(), aligned, w, mode)[0], want), method
    pick = np.array([r[0].startswith("ZZ_CANCEL") for r in keys])
    assert pick.sum() == 48


def test_refusals_leave_out_untouched():
    from asvspoof2021_air_amd import _hip, ops
    L = _hip.lib()
    assert L.air_score_fuse_max_systems() >= 16 and ops.score_fuse_max_systems() == L.air_score_fuse_max_systems()
    K, N = 3, 100
    buf = torch.arange(K * N + N, dtype=torch.float32, device="cuda")
    scores, out = buf[:K * N], buf[K * N:]
    before = buf.cpu().numpy().copy()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    null = ctypes.c_void_p(0)

    def call(scores_p=p(scores), stride=N, K=K, N=N, mode=0, out_p=p(out)):
        return L.air_score_fuse(scores_p, ctypes.c_int64(stride), null, null, ctypes.c_int(K), ctypes.c_int64(N),
                                ctypes.c_int(mode), out_p, null, _hip.stream())

    assert call(K=0) == -1 and call(N=-1) == -1 and call(mode=2) == -1
    assert call(K=L.air_score_fuse_max_systems() + 1) == -2
    assert call(scores_p=null) == -1 and call(out_p=null) == -1
    assert call(stride=N - 1) == -1  # rows that overlap each other
    assert call(out_p=p(scores[2 * N + 50:])) == -1 and call(out_p=p(scores)) == -1  # out inside the rows
    assert call(N=0) == 0 and call(N=0, scores_p=null, out_p=null) == 0
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), before)
    assert call() == 0  # (and the same call is accepted when out lies behind the rows)
    assert np.array_equal(out.cpu().numpy(), before[:N] + before[N:2 * N] + before[2 * N:3 * N])
    with pytest.raises(_hip.AirError):
        ops.score_fuse(torch.zeros(2, 4))
    with pytest.raises(ValueError):
        ops.score_fuse(torch.zeros(L.air_score_fuse_max_systems() + 1, 4, device="cuda"))
    with pytest.raises(ValueError):
        ops.score_fuse(torch.zeros(2, 4, device="cuda"), mode="max")
    assert ops.score_fuse(torch.zeros(2, 0, device="cuda")).numel() == 0


def test_weights_are_device_data_of_a_captured_graph():
    from asvspoof2021_air_amd import ops
    host = draw(3, 1000, 5)
    dev = torch.from_numpy(host).cuda()
    weights = torch.ones(3, device="cuda")
    out = torch.empty(1000, device="cuda")
    ops.score_fuse(dev, None, weights, "mean", out=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.score_fuse(dev, None, weights, "mean", out=out)
    for w in ([0.2, 0.3, 0.5], [1.0, 1e-5, 0.25]):
        weights.copy_(torch.tensor(w))
        graph.replay()
        assert fo.same_bits(out.cpu().numpy(), fo.bits(fo.fuse(host, None, np.array(w, dtype=np.float32), "mean")[0]))


# ------------------------------------------------------------------ fuse_device
@pytest.fixture(scope="module")
def fixture_on_device(golden, tmp_path_factory):
    """The fixture for fuse_device: system k's row is its file's scores in file order.  The one NaN score (file B, trial
    ZZ_NAN_000) is left out of its file: pandas neither sums nor counts it, so the fused frame is the recorded one bit
    for bit, and the device chain - like compute_tDCF - refuses a system whose own scores hold a NaN."""
    from asvspoof2021_air_amd import score_fusion as sf
    g = golden("fusion.npz")
    frames = [sf.read_file(p) for p in fo.fixture_inputs(g, tmp_path_factory.mktemp("fusion_gpu"))]
    kept = []
    for f in frames:
        ok = ~np.isnan(f.score)
        kept.append(sf.ScoreFrame(*([c for c, o in zip(col, ok) if o] for col in (f.fname, f.sysid, f.key)), f.score[ok]))
    assert sum(len(f) for f in kept) == sum(len(f) for f in frames) - 1
    matrix, index, keys, labels = sf.align(kept)
    rows = np.zeros((3, max(len(f) for f in kept)), dtype=np.float32)
    for k, f in enumerate(kept):
        rows[k, :len(f)] = f.score
    return g, kept, torch.from_numpy(rows).cuda(), index, keys, labels


def test_fuse_device_on_the_fixture(fixture_on_device, monkeypatch):
    from asvspoof2021_air_amd import eval_metrics as em, score_fusion as sf
    g, frames, rows, index, keys, labels = fixture_on_device
    dev_labels = torch.from_numpy(labels).cuda()
    host_eers = []
    for f in frames:
        lab = np.array([sf.LABELS[k] for k in f.key])
        s = f.score.astype(np.float64)
        host_eers.append((em.compute_eer(s[lab == 0], s[lab == 1])[0], em.compute_eer(-s[lab == 0], -s[lab == 1])[0]))
    copies = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **kw: (copies.append(t.numel()), real_cpu(t, *a, **kw))[1])
    for method, eers, n_copies in (("avg", None, 1), ("wght", g["eers"].tolist(), 1), ("wght", None, 2)):
        del copies[:]
        res = sf.fuse_device(rows, dev_labels, method, eers, index=index)
        assert len(copies) == n_copies, (method, eers, copies)  # the device-to-host copies fuse_device documents
        assert res.system_eers == host_eers
        fused = real_cpu(res.scores).numpy()
        if eers is not None or method == "avg":
            assert keys == fo.fixture_rows(g, method)[0]
            assert fo.same_bits(fused, g[method + "_bits"])
            assert res.eer == float(g[method + "_eer"])
        else:  # the weights from the systems' own EERs: the host port on the same inputs
            assert res.weights == sf.cal_weight([min(e) for e in host_eers])
            want = sf.weighted_fuse(frames, [min(e) for e in host_eers])
            assert fo.same_bits(fused, fo.bits(want.score)) and res.eer == sf.fused_eer(want.rows(), want.score)
        assert res.eer == em.eer_both_polarities(fused.astype(np.float64), labels) == min(res.eers)
        assert res.min_tdcf is None and res.by_group is None


def test_fuse_device_by_group_and_tdcf(fixture_on_device, golden):
    from asvspoof2021_air_amd import eval_metrics as em, score_fusion as sf
    g, frames, rows, index, keys, labels = fixture_on_device
    sysids = sorted({r[1] for r in keys if r[2] == "spoof"})
    groups = np.array([-1 if r[2] == "bonafide" else sysids.index(r[1]) for r in keys], dtype=np.int64)
    res = sf.fuse_device(rows, torch.from_numpy(labels).cuda(), "avg", index=index, groups=torch.from_numpy(groups).cuda(),
                         n_groups=len(sysids))
    fused = res.scores.cpu().numpy().astype(np.float64)
    want = em.eer_both_polarities_by_group(fused, labels, groups, len(sysids))
    assert len(sysids) > 3 and [None if b is None else b["eer"] for b in res.by_group] == want
    assert res.eer == float(g["avg_eer"])
    # min t-DCF: compute_tDCF refuses the fixture's -inf, so the finite trials alone, aligned
    rates = tuple(golden("tdcf.npz")["asv_rates"])
    finite = np.isfinite(fused) & (index >= 0).all(axis=0)
    matrix = sf.align(frames)[0][:, finite]
    lab = labels[finite]
    res = sf.fuse_device(torch.from_numpy(matrix).cuda(), torch.from_numpy(lab).cuda(), "avg",
                         tdcf=rates + (em.asvspoof19_cost_model(),))
    s = res.scores.cpu().numpy().astype(np.float64)
    assert np.array_equal(s, fused[finite])
    sg = 1.0 if res.eers[0] < res.eers[1] else -1.0
    curve, _ = em.compute_tDCF(sg * s[lab == 0], sg * s[lab == 1], *rates, em.asvspoof19_cost_model())
    assert res.min_tdcf == curve[np.argmin(curve)]


def test_fuse_device_limits(fixture_on_device):
    from asvspoof2021_air_amd import _hip, ops, score_fusion as sf
    g, frames, rows, index, keys, labels = fixture_on_device
    dev_labels = torch.from_numpy(labels).cuda()
    with pytest.raises(_hip.AirError):
        sf.fuse_device(rows.cpu(), dev_labels)
    with pytest.raises(_hip.AirError):
        sf.fuse_device(rows, torch.from_numpy(labels), index=index)
    lost = index.copy()
    lost[:, 17] = -1
    with pytest.raises(ValueError, match="absent from every system"):
        sf.fuse_device(rows, dev_labels, index=lost)
    with pytest.raises(ValueError):
        sf.fuse_device(rows, dev_labels, "max", index=index)
    with pytest.raises(ValueError):
        sf.fuse_device(rows, dev_labels, "wght", [0.1, 0.2], index=index)
    n = ops.EVAL_MAX_TRIALS + 1
    with pytest.raises(ValueError):
        sf.fuse_device(torch.zeros(2, n, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda"))


# ------------------------------------------------------------------ the ensemble pass
@pytest.fixture(scope="module")
def ensemble():
    """Two systems without forward randomness: an eval-mode ECAPA scored by softmax and a ResNet-18 without attention
    noise scored by its OC-softmax head."""
    from asvspoof2021_air_amd.ecapa_tdnn import Bottle2neck, Res2Net2
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.resnet import ResNet
    ecapa = fill_module_(Res2Net2(Bottle2neck, C=512, model_scale=8, nOut=2, n_mels=60)).cuda().eval()
    resnet = fill_module_(ResNet(3, 256, resnet_type="18", nclasses=2))
    resnet.set_attention_noise(None)
    resnet = resnet.cuda().eval()
    lossm = fill_module_(AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)).cuda()
    return dict(models=[ecapa, resnet], loss_models=[None, lossm], add_loss=[None, "ocsoftmax"], ecapa=[True, False])


@pytest.mark.parametrize("method", ["avg", "wght"])
def test_ensemble_pass_writes_the_files_of_the_single_passes(tmp_path, ensemble, method):
    from asvspoof2021_air_amd import score_fusion as sf
    from asvspoof2021_air_amd.generate_score import test_on_dataset, test_on_dataset_ensemble
    B, n_batches, T = 4, 3, 128
    n = B * n_batches
    feats = synth_feat((n, 1, T, 60), seed=21)
    names = ["LA_E_%07d" % (5000 - 7 * i) for i in range(n)]  # not in sorted order
    labels = torch.tensor([i % 3 == 0 for i in range(n)]).long()
    tags = torch.zeros(n)
    data = [(feats[i:i + B], names[i:i + B], tags[i:i + B], labels[i:i + B]) for i in range(0, n, B)]
    singles = []
    for k in range(2):
        singles.append(str(tmp_path / ("single%d.txt" % k)))
        assert test_on_dataset(ensemble["models"][k], data, singles[k], ensemble["loss_models"][k], ensemble["add_loss"][k],
                               task="19eval", ecapa=ensemble["ecapa"][k], keep_dataset_labels=True, sync="end") == n
    files = [str(tmp_path / ("ens%d.txt" % k)) for k in range(2)]
    fused_file = str(tmp_path / "fused" / "scores.txt")
    eers = [0.3, 0.1] if method == "wght" else None
    lines, res = test_on_dataset_ensemble(fused_file=fused_file, method=method, eers=eers, loader=iter(data), score_files=files,
                                          task="19eval", keep_dataset_labels=True, **ensemble)
    assert lines == n
    for a, b in zip(singles, files):
        assert open(a, "rb").read() == open(b, "rb").read() and len(open(a).readlines()) == n
    assert open(singles[0], "rb").read() != open(singles[1], "rb").read()
    want = sf.avg_fuse(singles, str(tmp_path / "host_")) if method == "avg" else sf.weighted_fuse(singles, eers, str(tmp_path / "host_"))
    assert open(fused_file, "rb").read() == open(str(tmp_path / "host_") + sf.OUTPUT_NAME, "rb").read()
    assert fo.same_bits(res.scores.cpu().numpy()[np.argsort(names)], fo.bits(want.score))
    assert res.eer == sf.fused_eer(want.rows(), want.score)
    # without the true keys: the reference's all-bonafide files, no result; the 2021 layout has nothing to join on
    lines, res = test_on_dataset_ensemble(loader=data, score_files=files, fused_file=fused_file, method=method, eers=eers,
                                          task="19eval", **ensemble)
    assert (lines, res) == (n, None) and open(fused_file).read().count(" - bonafide ") == n
    with pytest.raises(ValueError):
        test_on_dataset_ensemble(loader=[d[:2] for d in data], score_files=files, fused_file=fused_file, task="LA", **ensemble)
    with pytest.raises(ValueError):
        test_on_dataset_ensemble(loader=data, score_files=files[:1], **ensemble)


def test_score_pcm_ensemble_rows_equal_score_pcm(ensemble):
    from asvspoof2021_air_amd.generate_score import score_pcm, score_pcm_ensemble
    pcm = synth_pcm(4, 16000, seed=33).cuda()
    got = score_pcm_ensemble(ensemble["models"], ensemble["loss_models"], pcm, feat_len=128, ecapa=ensemble["ecapa"],
                             add_loss=ensemble["add_loss"])
    assert got.shape == (2, 4)
    for k in range(2):
        want = score_pcm(ensemble["models"][k], ensemble["loss_models"][k], pcm, feat_len=128, ecapa=ensemble["ecapa"][k],
                         add_loss=ensemble["add_loss"][k])
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), want.float().cpu().numpy().view(np.uint32))
