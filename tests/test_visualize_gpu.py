"""GPU: the embedding projections of csrc/embed_vis.hip (PCA, pairwise distances, perplexity bisection, joint
distribution, t-SNE gradient / KL / descent / stop rules) against the fp64 oracle tests/tsne_oracle.py, the embeddings
out of Trainer.evaluate(keep_feats=True), and the figure of visualize.py.

TOLERANCES.  Every comparison is kernel against fp64 oracle, and its bound is FOUR TIMES the distance of the oracle's own
fp32 restatement (the same numpy statement with every array and scalar in fp32) from the fp64 oracle ON THE TEST'S INPUT,
taken here on the CPU by ``bound()`` - never a figure of the kernel's.  The factor is there because the kernel's
summation order differs from numpy's.  Distances measured for the inputs below (profiles/embedding_vis.md has the
table; "rel" = relative to the largest reference magnitude):
    squared distances      9e-9 .. 1.6e-7 rel                  -> bound 3.6e-8 .. 6.3e-7 rel
    beta                   8e-7 .. 5.4e-5 rel                  -> bound 3.4e-6 .. 2.1e-4 rel
    conditional P          1.2e-6 .. 5.3e-6 absolute           -> bound 4.8e-6 .. 2.1e-5 (rows sums: 1.1e-7 .. 1.7e-7)
    joint P                4.1e-9 .. 3.7e-8 absolute, its sum 4.7e-10 .. 1.9e-9
    gradient               1.0e-7 .. 5.3e-7 rel, KL 5e-10 .. 1.0e-7 rel; N = 2 with exaggeration 1: 0 (p = q exactly)
    descent (5 iterations) y 4.7e-7 rel, update 1.0e-6 rel, KL 5.7e-9 rel; gains: no entry differs
    switch (3 + 3)         y 1.1e-6 rel, update 7.8e-7 rel, KL 1.0e-7 rel
    PCA                    mean 2.8e-8 .. 6.7e-7 rel, Gram 4.1e-9 .. 3.3e-7 rel, ratio 1.8e-9 .. 7.2e-8 absolute,
                           components 8e-9 .. 8.2e-8 absolute, projection 1.4e-7 .. 1.9e-6 rel
The entropy bound is scikit-learn's 1e-5 nats plus the restatement's own entropy error (the fp64 entropy of its fp32
row against the entropy it stopped at), 2.5e-7 .. 2.4e-6 nats, over the rows whose bisection converges: on the input
with duplicates and an outlier scikit-learn itself runs out of its 100 steps on some rows (the outlier's distances are
all but equal in fp32), which are compared with the oracle like any other but have no entropy to meet."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsne_oracle as o  # noqa: E402
from oracle.filler import fill_module_, synth_pcm  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def bound(name, ref64, ref32):
    """4 x the largest distance of the fp32 restatement from the fp64 oracle (printed: the test log carries the figure)."""
    ref64, ref32 = np.asarray(ref64, dtype=F64), np.asarray(ref32, dtype=F64)
    d = float(np.abs(ref32 - ref64).max()) if ref64.size else 0.0
    scale = float(np.abs(ref64).max()) if ref64.size else 0.0
    print("%s: restatement distance %.3g (%.3g of the largest magnitude %.3g) -> bound %.3g" % (
        name, d, d / scale if scale else 0.0, scale, 4 * d))
    return 4.0 * d


def close(name, got, ref64, ref32):
    got = np.asarray(got, dtype=F64)
    b = bound(name, ref64, ref32)
    err = float(np.abs(got - np.asarray(ref64, dtype=F64)).max()) if got.size else 0.0
    print("%s: kernel distance %.3g" % (name, err))
    assert err <= b, "%s: kernel %.3g from the fp64 oracle, bound %.3g" % (name, err, b)


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def host(t):
    return t.detach().cpu().numpy()


def rows(n, d, seed, offset=0.0):
    return (np.random.RandomState(seed).randn(n, d) + offset).astype(F32)


# ------------------------------------------------------------------ pairwise squared distances
# every tile edge (64 x 64 tiles, 16 features per stage, 4-wide vector loads): N in {2, 63, 64, 65, 193, 257},
# D in {1, 20, 256} and 7 (no multiple of the vector width)
@pytest.mark.parametrize("N,D", [(2, 1), (63, 20), (64, 256), (65, 7), (193, 20), (257, 256), (193, 1), (257, 7)])
def test_sqdist_against_fp64(N, D):
    from asvspoof2021_air_amd import ops
    x = rows(N, D, 10 * N + D)
    got = host(ops.pairwise_sqdist(dev(x)))
    close("sqdist N=%d D=%d" % (N, D), got, o.sqdist(x), o.sqdist(x, F32))
    assert np.array_equal(got, got.T) and np.all(np.diag(got) == 0)


def test_sqdist_offset_cluster_and_identical_rows():
    """A unit cluster at offset 100: |x|^2 ~ 10^4 D, where the expansion |x_i|^2 + |x_j|^2 - 2 x_i.x_j would keep 3
    digits; three identical rows: exact zeros."""
    from asvspoof2021_air_amd import ops
    x = rows(193, 20, 5, offset=100.0)
    x[7] = x[50] = x[192]
    got = host(ops.pairwise_sqdist(dev(x)))
    close("sqdist offset 100", got, o.sqdist(x), o.sqdist(x, F32))
    expanded = (x.astype(F32) ** 2).sum(1)[:, None] + (x ** 2).sum(1)[None, :] - 2 * (x @ x.T)
    assert np.abs(expanded - o.sqdist(x)).max() > 100 * np.abs(got - o.sqdist(x)).max()  # (what the kernel avoids)
    for a in (7, 50, 192):
        for b in (7, 50, 192):
            assert got[a, b] == 0.0
    assert np.array_equal(got, got.T) and np.all(np.diag(got) == 0)


# ------------------------------------------------------------------ affinities and the joint distribution
@functools.lru_cache(maxsize=None)
def affinity_case(N, perplexity, hard):
    """(fp32 distances, fp64 oracle (cond, beta, err), fp32 restatement (cond, beta, err)).  hard: three identical
    rows and one outlier at 1e4."""
    x, _ = o.clusters(N, 16, seed=N)
    if hard:
        x[1] = x[0]
        x[2] = x[0]
        x[-1] = 1e4
    d = o.sqdist(x).astype(F32)
    return d, o.binary_search_perplexity(d, perplexity), o.binary_search_perplexity(d, perplexity, F32)


def entropy64(p):
    p = np.asarray(p, dtype=F64)
    p = p / p.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.where(p > 0, p * np.log(p), 0.0).sum(axis=1)


@pytest.mark.parametrize("N,perplexity,hard", [(193, 5.0, False), (193, 40.0, False), (48, 40.0, False),
                                               (193, 40.0, True), (48, 5.0, True)])
def test_affinities(N, perplexity, hard):
    from asvspoof2021_air_amd import ops
    d, (c64, b64, e64), (c32, b32, e32) = affinity_case(N, perplexity, hard)
    cond, beta = ops.tsne_affinities(dev(d), perplexity)
    cond, beta = host(cond), host(beta)
    assert np.all(np.isfinite(cond)) and np.all(np.isfinite(beta)) and np.all(np.diag(cond) == 0)
    tag = "N=%d perplexity=%g%s" % (N, perplexity, " hard" if hard else "")
    close("beta " + tag, beta, b64, b32)
    close("conditional P " + tag, cond, c64, c32)
    # rows sum to 1: the fp32 rounding of N entries, bounded by the restatement's own row sums
    close("row sums " + tag, cond.astype(F64).sum(1), c64.sum(1), c32.astype(F64).sum(1))
    # the entropy of the device's row, in fp64 on the host, against log(perplexity): scikit-learn's 1e-5 plus the
    # restatement's entropy error - the fp64 entropy of its fp32 row against the entropy it stopped at
    target = np.log(perplexity)
    converged = (np.abs(e64) <= o.PERPLEXITY_TOLERANCE) & (np.abs(e32) <= F32(o.PERPLEXITY_TOLERANCE))
    assert converged.all() if not hard else converged.sum() >= N - 8  # (scikit-learn's own 100 steps run out on a few)
    restated = float(np.abs(entropy64(c32) - (e32.astype(F64) + target))[converged].max())
    print("entropy %s: restatement error %.3g -> bound %.3g" % (tag, restated, 1e-5 + restated))
    assert np.abs(entropy64(cond) - target)[converged].max() <= 1e-5 + restated


@pytest.mark.parametrize("N,perplexity,hard", [(193, 40.0, False), (193, 40.0, True), (2, 1.0, False), (65, 5.0, False)])
def test_joint(N, perplexity, hard):
    from asvspoof2021_air_amd import ops
    if N == 2:  # no bisection to speak of: any conditional matrix serves
        c64 = np.array([[0.0, 1.0], [1.0, 0.0]])
        c32 = c64.astype(F32)
    else:
        _, (c64, _, _), (c32, _, _) = affinity_case(N, perplexity, hard)
    cond = c64.astype(F32)  # the kernel's input: the oracle's conditional, rounded
    P = host(ops.tsne_joint(dev(cond)))
    tag = "N=%d%s" % (N, " hard" if hard else "")
    assert np.array_equal(P, P.T) and np.all(np.diag(P) == 0) and np.all(np.isfinite(P))
    close("joint P " + tag, P, o.joint(c64), o.joint(c32, F32))
    close("sum of P " + tag, [P.astype(F64).sum()], [o.joint(c64).sum()], [o.joint(c32, F32).astype(F64).sum()])
    off = ~np.eye(N, dtype=bool)
    assert P[off].min() >= F32(o.EPS)


# ------------------------------------------------------------------ gradient and KL at fixed embeddings
@functools.lru_cache(maxsize=None)
def joint_case(N):
    if N == 2:
        return np.array([[0.0, 0.5], [0.5, 0.0]])
    x, _ = o.clusters(N, 16, seed=N)
    d = o.sqdist(x).astype(F32)
    return o.joint(o.binary_search_perplexity(d, min(40.0, (N - 1) / 3.0))[0]).astype(F32).astype(F64)


def embedding(N, scale):
    y = np.random.RandomState(N).randn(N, 2)
    if scale == "init":
        return (y * 1e-4).astype(F32)
    if scale == "unit":
        return y.astype(F32)
    y = y * 50.0  # two far points: n_ij / Z falls below eps, q sits at its floor
    y[0] = (3e9, -2e9)
    y[-1] = (-4e9, 1e9)
    return y.astype(F32)


@pytest.mark.parametrize("exaggeration", [1.0, 40.0])
@pytest.mark.parametrize("scale", ["init", "unit", "far"])
@pytest.mark.parametrize("N", [2, 193, 257])
def test_gradient_and_kl(N, scale, exaggeration):
    from asvspoof2021_air_amd import ops
    P, y = joint_case(N), embedding(N, scale)
    kl64, g64, _ = o.kl_grad(P, y, exaggeration)
    kl32, g32, _ = o.kl_grad(P, y, exaggeration, F32)
    if scale == "far" and N > 2:
        n = 1.0 / (1.0 + o.sqdist(y))
        assert (n / (n.sum() - N) < o.EPS).sum() >= 2  # the floor is reached
    grad, status = ops.tsne_gradient_kl(dev(P), dev(y), exaggeration)
    tag = "N=%d %s e=%g" % (N, scale, exaggeration)
    close("gradient " + tag, host(grad), g64, g32)
    close("KL " + tag, [ops.tsne_read_status(status)["kl"]], [kl64], [kl32])


# ------------------------------------------------------------------ descent, switch, stop rules, determinism
@functools.lru_cache(maxsize=None)
def fixture_case(N):
    """The fixture's input with the oracle's joint (as the fp32 matrix the kernel is given) and PCA start."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "visualize.npz"))
    x = g["x_%d" % N]
    P = o.joint(o.binary_search_perplexity(o.sqdist(x).astype(F32), 40.0)[0]).astype(F32)
    return g, x, P, g["y_%d" % N][0].astype(F32)


def run_device(P, y0, **kw):
    """tsne_run on device copies: (y, update, gains, status dict)."""
    from asvspoof2021_air_amd import ops
    y = dev(y0).clone()
    update, gains = torch.empty_like(y), torch.empty_like(y)
    status = ops.tsne_new_status("cuda")
    ops.tsne_run(dev(P), y, update, gains, status, **kw)
    return host(y), host(update), host(gains), ops.tsne_read_status(status)


def test_descent_five_iterations():
    """tests/test_visualize_cpu.py checks on the CPU that the fp32 restatement makes the sign decisions of fp64 on this
    input over these five iterations: no entry of ``gains`` may differ here either."""
    g, x, P, y0 = fixture_case(192)
    kw = dict(max_iter=5, learning_rate=50.0, early_exaggeration=40.0)
    r64 = o.descent(P.astype(F64), y0, **kw)
    r32 = o.descent(P.astype(F64), y0, dtype=F32, **kw)
    assert np.abs(r32["gains"] - r64["gains"]).max() <= 1e-6  # (the choice of input, re-checked)
    y, update, gains, st = run_device(P, y0, **kw)
    close("descent y", y, r64["y"], r32["y"])
    close("descent update", update, r64["update"], r32["update"])
    assert np.abs(gains - r64["gains"]).max() <= 1e-6  # same decisions: other sequences differ by several per cent
    assert st["n_iter"] == 4 and not st["stopped"]
    close("descent KL", [st["kl"]], [r64["kl"]], [r32["kl"]])


def test_switch_resets_update_gains_and_exaggeration():
    g, x, P, y0 = fixture_case(96)
    kw = dict(max_iter=6, exploration_iter=3, learning_rate=50.0, early_exaggeration=40.0)
    r64 = o.descent(P.astype(F64), y0, **kw)
    r32 = o.descent(P.astype(F64), y0, dtype=F32, **kw)
    y, update, gains, st = run_device(P, y0, **kw)
    close("switch y", y, r64["y"], r32["y"])
    close("switch update", update, r64["update"], r32["update"])
    assert np.abs(gains - r64["gains"]).max() <= 1e-6 and np.abs(r32["gains"] - r64["gains"]).max() <= 1e-6
    assert gains.max() <= 1.0 + 0.2 * 3 + 1e-6  # three iterations since gains = 1 (six without the reset: up to 2.2)
    close("switch KL", [st["kl"]], [r64["kl"]], [r32["kl"]])  # exaggeration 1 at the end
    assert st["n_iter"] == 5


@pytest.mark.parametrize("rule", ["grad_norm", "no_progress"])
def test_stop_rules(rule):
    g, x, P, y0 = fixture_case(96)
    kw = dict(exploration_iter=2, n_iter_check=2, learning_rate=50.0, early_exaggeration=40.0)
    kw.update(dict(min_grad_norm=1e30) if rule == "grad_norm" else dict(n_iter_without_progress=0))
    want = o.descent(P.astype(F64), y0, max_iter=40, **kw)
    assert want["stopped"] and (want["n_iter"] == 3 if rule == "grad_norm" else 3 < want["n_iter"] < 39)
    y, update, gains, st = run_device(P, y0, max_iter=40, **kw)
    assert st["stopped"] == 1 and st["n_iter"] == want["n_iter"] and st["reason"] == (2 if rule == "grad_norm" else 1)
    # bit-equal to the run that ends at that iteration: the launches of iterations n_iter + 1 .. 39 changed nothing
    y2, update2, gains2, st2 = run_device(P, y0, max_iter=want["n_iter"] + 1, **kw)
    assert np.array_equal(y, y2) and np.array_equal(update, update2) and np.array_equal(gains, gains2)
    assert st["kl"] == st2["kl"] and st2["n_iter"] == want["n_iter"]


def test_tsne_device_is_deterministic_and_checks_arguments():
    from asvspoof2021_air_amd import visualize
    g, x, P, y0 = fixture_case(96)
    X = dev(x)
    runs = [visualize.tsne_device(X, max_iter=60, exploration_iter=20, n_iter_check=10) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and runs[0][2] == runs[1][2] == 59
    y, kl, n_iter = visualize.tsne_device(X, max_iter=60, exploration_iter=20, n_iter_check=10, init=dev(y0))
    assert tuple(y.shape) == (96, 2) and np.isfinite(kl)
    with pytest.raises(ValueError):
        visualize.tsne_device(X, perplexity=96.0)
    with pytest.raises(ValueError):
        visualize.tsne_device(X, init=dev(y0[:5]))


def test_end_to_end_full_schedule():
    """N = 192, three clusters, the default schedule (1000 iterations, PCA start, learning rate "auto").  Trajectories
    diverge after some 20 iterations whatever the arithmetic, so the end is held to the fixture's eight fp64 oracle
    runs from starts 1e-7 apart: a final KL no higher than their largest plus their own spread, and nearest embedded
    neighbours of the own cluster as often as in the worst of them."""
    from asvspoof2021_air_amd import visualize
    g, x, P, y0 = fixture_case(192)
    y, kl, n_iter = visualize.tsne_device(dev(x))
    kls, purity = g["spread_kl_192"], g["spread_nn_192"]
    print("end to end: device KL %.6f after iteration %d; oracle runs %.6f .. %.6f" % (kl, n_iter, kls.min(), kls.max()))
    assert np.isfinite(host(y)).all() and n_iter <= 999
    assert kl <= kls.max() + (kls.max() - kls.min())
    assert o.nn_purity(host(y).astype(F64), g["labels_192"]) >= purity.min()


# ------------------------------------------------------------------ PCA
def pca_input(N, D, seed):
    """Offset 100 from the origin, leading standard deviations 8 and 4 (then 1): the components are well separated."""
    rng = np.random.RandomState(seed)
    x = rng.randn(N, D)
    x[:, 0] *= 8.0
    if D > 1:
        x[:, 1] *= 4.0
    q, _ = np.linalg.qr(rng.randn(D, D))
    return (x @ q + 100.0).astype(F32)


@pytest.mark.parametrize("N,D", [(3, 2), (3, 20), (193, 2), (193, 20), (193, 256), (3, 256)])
def test_pca_against_fp64(N, D):
    from asvspoof2021_air_amd import ops, visualize
    x = pca_input(N, D, 100 * N + D)
    p64, c64, m64, r64, g64 = o.pca(x, 2)
    p32, c32, m32, r32, g32 = o.pca(x, 2, F32)
    mean, gram = ops.pca_gram(dev(x))
    tag = "N=%d D=%d" % (N, D)
    close("PCA mean " + tag, host(mean), m64, m32)
    close("PCA Gram " + tag, host(gram), g64, g32)
    assert np.array_equal(host(gram), host(gram).T)
    res = visualize.pca_device(dev(x), 2)
    close("PCA ratio " + tag, res.explained_variance_ratio, r64, r32)
    comps = host(res.components).astype(F64)
    top = np.argmax(np.abs(comps), axis=1)
    assert np.all(comps[np.arange(2), top] > 0)  # the sign rule
    if N > 3:  # (at N = 3 the second component of 2 centred points' span is defined; the third direction is not needed)
        close("PCA components " + tag, comps, c64, c32)
    close("PCA projection " + tag, host(res.projection), p64, p32)


@pytest.mark.parametrize("N", [96, 192])
def test_pca_against_sklearn_fixture(N):
    """The projection against scikit-learn's own PCA(2).fit_transform: the kernel's bound to the fp64 oracle plus
    scikit-learn's own distance from it (its result is fp32 arithmetic of the fp32 input)."""
    from asvspoof2021_air_amd import visualize
    g, x, P, y0 = fixture_case(N)
    p64, _, _, r64, _ = o.pca(x, 2)
    p32, _, _, r32, _ = o.pca(x, 2, F32)
    res = visualize.pca_device(dev(x), 2)
    sk = float(np.abs(g["pca_%d" % N] - p64).max())
    b = bound("PCA projection N=%d" % N, p64, p32)
    assert np.abs(host(res.projection) - g["pca_%d" % N]).max() <= b + sk
    assert np.abs(res.explained_variance_ratio - g["pca_ratio_%d" % N]).max() <= bound("ratio", r64, r32) + np.abs(
        g["pca_ratio_%d" % N] - r64).max()


# ------------------------------------------------------------------ embeddings out of the dev / eval pass
def test_evaluate_keep_feats():
    from asvspoof2021_air_amd.resnet import ResNet
    from asvspoof2021_air_amd.train import Trainer
    from asvspoof2021_air_amd import visualize
    model = ResNet(3, 256, resnet_type="18", nclasses=2)
    fill_module_(model)
    model.set_attention_noise(None)
    tr = Trainer(model, feat_len=96)
    fill_module_(tr.loss)
    B = 4
    batches = [(synth_pcm(B, 8000, seed=40 + i).cuda(), ((torch.arange(B) + i) % 3 != 0).long().cuda()) for i in range(3)]
    lengths = torch.tensor([8000, 3000, 7000, 500], dtype=torch.int32).cuda()
    batches[1] = batches[1] + (None, lengths)  # a ragged batch: row b holds lengths[b] samples
    plain = tr.evaluate(batches)
    assert plain.feats is None
    for given in (batches, iter(batches)):  # preallocated from len(), and grown by device-side copies
        out = tr.evaluate(given, keep_feats=True)
        loss, eer, min_tdcf, scores, labels = out  # five fields, as before
        assert (loss, eer, min_tdcf) == (plain.loss, plain.eer, plain.min_tdcf)
        assert torch.equal(scores, plain.scores) and torch.equal(labels, plain.labels)
        assert out.feats.dtype == torch.float32 and tuple(out.feats.shape) == (3 * B, 256)
        tr.model.eval()
        with torch.no_grad():
            for i, batch in enumerate(batches):
                want = tr.model(tr.features(batch[0], None, batch[3] if len(batch) > 3 else None))[0]
                assert torch.equal(out.feats[i * B:(i + 1) * B], want.float())
    feats, labels = visualize.get_features(tr, batches)
    assert torch.equal(feats, out.feats) and torch.equal(labels, plain.labels)


# ------------------------------------------------------------------ the figure
def test_embed_dev_and_eval_and_the_figure(tmp_path):
    from asvspoof2021_air_amd import visualize
    xd, ld = o.clusters(150, 16, seed=1)
    xe, le = o.clusters(130, 16, seed=2)
    center = np.zeros((1, 16), F32)
    kw = dict(k=64, perplexity=20.0, max_iter=40, exploration_iter=20, n_iter_check=10)
    e = visualize.embed_dev_and_eval(dev(xd), ld % 2, dev(xe), le % 2, center, **kw)
    assert [tuple(b.shape) for b in e[:6]] == [(1, 2), (64, 2), (64, 2), (1, 2), (64, 2), (64, 2)]
    assert e.explained_variance_ratio.shape == (2,) and np.isfinite(e.kl_divergence) and e.n_iter == 39
    # the centre row comes first: its PCA projection is that of row 0 of the stack [center; dev; eval]
    ind_dev, ind_eval = visualize.sample_indices(150, 130, 64)
    stack = np.concatenate((center, xd[ind_dev.numpy()], xe[ind_eval.numpy()]))
    want = host(visualize.pca_device(dev(stack), 2).projection)
    assert np.array_equal(host(e.center_pca), want[:1]) and np.array_equal(host(e.feat_pca_eval), want[65:])
    pytest.importorskip("matplotlib")
    out = tmp_path / "fig"
    state = np.random.get_state()[1].copy()
    visualize.visualize_dev_and_eval(xd, ld % 2, None, dev(xe), torch.from_numpy(le % 2), None, center, 88, str(out), **kw)
    assert (out / "_vis_feat.pdf").stat().st_size > 1000
    assert np.array_equal(np.random.get_state()[1], state) and os.environ.get("PYTHONHASHSEED") != "668"
