"""CPU: the numpy oracle of the embedding projections (tests/tsne_oracle.py) against scikit-learn's recorded outputs
(tests/golden/visualize.npz) and, where scikit-learn imports, against its private functions directly; the index draws of
the reference's figure; the argument checks of the device entry points (no GPU needed: they refuse before any launch)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsne_oracle as o  # noqa: E402

SIZES = (96, 192)
PERPLEXITY, EXAGGERATION = 40.0, 40.0


@pytest.fixture(scope="module")
def g(golden):
    return golden("visualize.npz")


@pytest.fixture(scope="module")
def joint(g):
    out = {}
    for N in SIZES:
        D = o.sqdist(g["x_%d" % N]).astype(np.float32)
        out[N] = o.joint(o.binary_search_perplexity(D, PERPLEXITY)[0])
    return out


@pytest.mark.parametrize("N", SIZES)
def test_oracle_inputs_are_the_fixtures(g, N):
    X, labels = o.clusters(N, 16, seed=N)
    assert np.array_equal(X, g["x_%d" % N]) and np.array_equal(labels, g["labels_%d" % N])


@pytest.mark.parametrize("N", SIZES)
def test_oracle_joint_matches_sklearn(g, joint, N):
    # the issue's figure for this comparison: 2.2e-16 absolute, the floor itself
    assert np.abs(o.condensed(joint[N]) - g["p_%d" % N]).max() <= 2.3e-16
    assert np.array_equal(joint[N], joint[N].T) and np.all(np.diag(joint[N]) == 0)


@pytest.mark.parametrize("N", SIZES)
def test_oracle_kl_and_gradient_match_sklearn(g, joint, N):
    ys, kls, grads = g["y_%d" % N], g["kl_%d" % N], g["grad_%d" % N]
    for a in range(3):
        for b, ex in enumerate((1.0, EXAGGERATION)):
            kl, grad, _ = o.kl_grad(joint[N], ys[a], ex)
            assert abs(kl - kls[a, b]) <= 1e-12 * max(1.0, abs(kls[a, b]))
            scale = np.abs(grads[a, b]).max()
            assert np.abs(grad - grads[a, b]).max() <= 1e-12 * scale  # (measured: 1e-15 of the scale)


@pytest.mark.parametrize("N", SIZES)
def test_oracle_pca_matches_sklearn(g, N):
    proj, comps, mean, ratio, gram = o.pca(g["x_%d" % N], 2)
    want = g["pca_%d" % N]  # scikit-learn's fp32 result of fp32 input
    assert np.abs(proj - want).max() <= 2e-5 * np.abs(want).max()
    assert np.abs(ratio - g["pca_ratio_%d" % N]).max() <= 1e-6
    top = np.argmax(np.abs(comps), axis=1)
    assert np.all(comps[np.arange(2), top] > 0)
    assert np.abs(o.pca_init(g["x_%d" % N]) - g["y_%d" % N][0]).max() <= 1e-18 + 1e-12 * 1e-4


@pytest.mark.parametrize("N", SIZES)
def test_oracle_descent_reproduces_the_recorded_iterates(g, joint, N):
    """The descent with gains, momentum and exaggeration: five iterations from the PCA start land on the recorded
    embedding; the fp32 restatement makes the same sign decisions (gains) over these five iterations - the input of the
    GPU descent test is chosen by this."""
    lr = max(N / EXAGGERATION / 4.0, 50.0)
    y0 = g["y_%d" % N][0]
    r = o.descent(joint[N], y0, max_iter=5, learning_rate=lr, early_exaggeration=EXAGGERATION)
    assert np.allclose(r["y"], g["y_%d" % N][1], rtol=1e-9, atol=0)
    r32 = o.descent(joint[N], y0, max_iter=5, learning_rate=lr, early_exaggeration=EXAGGERATION, dtype=np.float32)
    # (gains are products of 0.8 and sums of 0.2: two different decision sequences differ by several per cent, the
    # same sequence in fp32 and fp64 by rounding)
    assert np.abs(r32["gains"] - r["gains"]).max() <= 1e-6


def test_oracle_switch_and_stop_rules(g, joint):
    N = 96
    P, y0 = joint[N], g["y_%d" % N][0]
    trace = []
    o.descent(P, y0, max_iter=6, exploration_iter=3, learning_rate=50.0, early_exaggeration=EXAGGERATION, trace=trace)
    # iteration 3 starts from update = 0 and gains = 1: its update is -lr * gains * grad with gains in {0.8} only
    assert np.all(trace[3][3] == 0.8)
    kw = dict(exploration_iter=2, n_iter_check=2, learning_rate=50.0, early_exaggeration=EXAGGERATION, max_iter=40)
    r = o.descent(P, y0, min_grad_norm=1e30, **kw)
    assert r["stopped"] and r["n_iter"] == 3
    # the no-progress rule: the KL first fails to improve at the check behind iteration 13, in fp64 and in fp32 alike -
    # the GPU test of the rule uses this input
    r = o.descent(P, y0, n_iter_without_progress=0, **kw)
    r32 = o.descent(P, y0, n_iter_without_progress=0, dtype=np.float32, **kw)
    assert r["stopped"] and r32["stopped"] and r["n_iter"] == r32["n_iter"] == 13


def test_oracle_end_of_run_within_spread_of_sklearn(g):
    for N in SIZES:
        kls = g["spread_kl_%d" % N]
        assert kls.min() - (kls.max() - kls.min()) <= float(g["sk_kl_%d" % N]) <= kls.max() + (kls.max() - kls.min())
        assert np.all(g["spread_nn_%d" % N] == 1.0)


def test_oracle_matches_sklearn_private_functions_directly(g, joint):
    _t_sne = pytest.importorskip("sklearn.manifold._t_sne")
    _utils = pytest.importorskip("sklearn.manifold._utils")
    N = 96
    X = g["x_%d" % N]
    D = o.sqdist(X).astype(np.float32)
    cond, beta, _ = o.binary_search_perplexity(D, PERPLEXITY)
    assert np.abs(cond - _utils._binary_search_perplexity(D, PERPLEXITY, 0)).max() <= 1e-15
    # duplicates and an outlier at 1e4 stay finite; the outlier's joint row mass is 1 / N
    Xo = X.copy()
    Xo[1] = Xo[0]
    Xo[2] = Xo[0]
    Xo[-1] = 1e4
    Do = o.sqdist(Xo).astype(np.float32)
    co = o.binary_search_perplexity(Do, PERPLEXITY)[0]
    sk = _utils._binary_search_perplexity(Do, PERPLEXITY, 0)
    assert np.all(np.isfinite(sk)) and np.abs(co - sk).max() <= 1e-15
    Po = o.joint(co)
    assert np.abs(o.condensed(Po) - _t_sne._joint_probabilities(Do, PERPLEXITY, 0)).max() <= 2.3e-16
    # (its conditional row sums to 1 and nobody's row reaches it: (1 + 0) / 2N)
    assert abs(Po[-1].sum() - 0.5 / N) <= 1e-3 / N
    kl, grad, _ = o.kl_grad(joint[N], g["y_%d" % N][1], EXAGGERATION)
    kl_sk, grad_sk = _t_sne._kl_divergence(g["y_%d" % N][1].ravel().copy(), g["p_%d" % N] * EXAGGERATION, 1.0, N, 2)
    assert abs(kl - kl_sk) <= 1e-12 * abs(kl_sk) and np.abs(grad.ravel() - grad_sk).max() <= 1e-12 * np.abs(grad_sk).max()


def test_sample_indices_match_the_reference_sequence(g):
    from asvspoof2021_air_amd.visualize import sample_indices
    n_dev, n_eval, k = (int(v) for v in g["sample_args"])
    before = torch.get_rng_state()
    ind_dev, ind_eval = sample_indices(n_dev, n_eval, k)
    assert torch.equal(torch.get_rng_state(), before)  # the caller's generator is untouched
    assert np.array_equal(ind_dev.numpy(), g["ind_dev"]) and np.array_equal(ind_eval.numpy(), g["ind_eval"])
    # the reference's lines (visualize.py:18-21) restated: one seeded global stream, two draws
    with torch.random.fork_rng():
        torch.manual_seed(888)
        want_dev = torch.randperm(n_dev)[:k]
        want_eval = torch.randperm(n_eval)[:k]
    assert torch.equal(ind_dev, want_dev) and torch.equal(ind_eval, want_eval)
    assert len(sample_indices(10, 5000, 5000)[0]) == 10


def test_argument_checks():
    from asvspoof2021_air_amd import _hip, build, ops, visualize
    build.build(verbose=False)
    L = _hip.lib()
    max_n, max_d, max_k = ops.vis_limits()
    assert max_n >= 16384 and max_d >= 1024
    assert ops.tsne_ws_bytes(1) == 0 and ops.tsne_ws_bytes(max_n + 1) == 0 and ops.tsne_ws_bytes(2) > 0
    assert ops.tsne_ws_bytes(max_n) > ops.tsne_ws_bytes(10003) > 0
    assert ops.pca_ws_bytes(1, 16) == 0 and ops.pca_ws_bytes(max_n + 1, 16) == 0 and ops.pca_ws_bytes(16, max_d + 1) == 0
    assert ops.pca_ws_bytes(max_n, max_d) > 0 and ops.pca_ws_bytes(3, 1) > 0
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    for n, d in ((1, 16), (max_n + 1, 16), (16, max_d + 1)):  # refused ahead of any launch: no pointer is touched
        assert L.air_pca_gram(one, n, d, one, one, one, ctypes.c_size_t(1 << 40), null) == -2
        assert L.air_pairwise_sqdist(one, n, d, one, null) == -2
    assert L.air_tsne_affinities(one, 1, ctypes.c_float(5.0), ctypes.c_void_p(32), one, null) == -2
    assert L.air_tsne_joint(one, max_n + 1, one, ctypes.c_size_t(1 << 40), null) == -2
    assert L.air_tsne_joint(one, 64, one, ctypes.c_size_t(8), null) == -4  # AIR_EWORKSPACE
    x = torch.zeros(100, 8)
    for call in (lambda: visualize.pca_device(x), lambda: visualize.tsne_device(x, perplexity=5.0),
                 lambda: ops.pairwise_sqdist(x), lambda: ops.tsne_affinities(torch.zeros(8, 8), 3.0),
                 lambda: ops.tsne_joint(torch.zeros(8, 8)), lambda: ops.pca_gram(x),
                 lambda: visualize.embed_dev_and_eval(x, None, x, None, torch.zeros(1, 8))):
        with pytest.raises(_hip.AirError):
            call()
    with pytest.raises(ValueError):
        visualize.tsne_device(torch.zeros(40, 8), perplexity=40.0)
    with pytest.raises(ValueError):
        visualize.tsne_device(torch.zeros(30, 8))  # the default perplexity, 40
