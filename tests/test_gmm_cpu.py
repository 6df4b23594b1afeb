"""CPU: the GMM oracle (tests/gmm_oracle.py) pinned to scikit-learn's GaussianMixture(covariance_type="diag") from a
given initialisation; sklearn round trips of gmm.DiagGMM; host-side refusals; the workspace's growth per frame."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import gmm_oracle as go

REG = 1e-6


def _cases():
    lf = go.lfcc_like(600, 20, seed=3)
    sp = go.separable(500, 3, 4, seed=5)
    return {"lfcc_like": (lf, go.init_from_data(lf, 4, seed=1, reg_covar=REG)),
            "separable": (sp, go.init_from_data(sp, 4, seed=2, reg_covar=REG))}


CASES = _cases()


def _sklearn_fit(x, init, max_iter, tol):
    mixture = pytest.importorskip("sklearn.mixture")
    w, mu, var = init
    gm = mixture.GaussianMixture(n_components=len(w), covariance_type="diag", reg_covar=REG, tol=tol, max_iter=max_iter,
                                 weights_init=w, means_init=mu, precisions_init=1.0 / var)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # ConvergenceWarning at tol = 0
        gm.fit(x.astype(np.float64))
    return gm


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_iteration_matches_sklearn_within_the_derived_bound(name):
    """One EM step from the same parameters: both are roundings of the same exact step (go.params_bound each)."""
    x, init = CASES[name]
    gm = _sklearn_fit(x, init, 1, 0.0)
    o = go.fit(x, *init, reg_covar=REG, max_iter=1, tol=0.0)
    dw, dmu, dvar, dlb = go.params_bound(x, *init, REG)
    assert gm.n_iter_ == o["n_iter"] == 1
    for got, want, bound, what in ((gm.weights_, o["w"], dw, "w"), (gm.means_, o["mu"], dmu, "mu"),
                                   (gm.covariances_, o["var"], dvar, "var")):
        err = np.abs(got - want)
        print(name, what, "max err / bound", float((err / (go.BOTH * bound)).max()))
        assert np.all(err <= go.BOTH * bound), what
    assert abs(gm.lower_bound_ - o["lower_bound"]) <= go.BOTH * dlb
    ll = gm.score_samples(x.astype(np.float64))
    want = go.score_samples(x, o["w"], o["mu"], o["var"])
    assert np.all(np.abs(ll - want) <= go.BOTH * go.lse_bound(x, o["w"], o["mu"], o["var"]))


# Ten iterations: a bound cannot be pushed through ten data-dependent steps, so what follows is an ALLOWANCE, argued and
# not derived.  Each step adds at most its own one-step bound and the EM map carries the earlier ones on; the allowance
# is the ten one-step bounds at the final parameters times 16, the margin the GPU fit test takes over a
# summation-order change (tests/test_gmm_gpu.py).  The printed ratios sit about three orders inside it.
@pytest.mark.parametrize("name", sorted(CASES))
def test_ten_iterations_match_sklearn(name):
    x, init = CASES[name]
    gm = _sklearn_fit(x, init, 10, 0.0)
    o = go.fit(x, *init, reg_covar=REG, max_iter=10, tol=0.0)
    assert gm.n_iter_ == o["n_iter"] == 10 and not o["converged"]
    dw, dmu, dvar, dlb = go.params_bound(x, o["w"], o["mu"], o["var"], REG)
    for got, want, bound, what in ((gm.weights_, o["w"], dw, "w"), (gm.means_, o["mu"], dmu, "mu"),
                                   (gm.covariances_, o["var"], dvar, "var")):
        err = np.abs(got - want)
        print(name, what, "max err / allowance", float((err / (160 * go.BOTH * bound)).max()),
              "max relative", float((err / np.abs(want)).max()))
        assert np.all(err <= 160 * go.BOTH * bound), what
    assert abs(gm.lower_bound_ - o["lower_bound"]) <= 160 * go.BOTH * dlb


@pytest.mark.parametrize("name", sorted(CASES))
def test_stop_rule_matches_sklearn(name):
    x, init = CASES[name]
    gm = _sklearn_fit(x, init, 100, 1e-3)
    o = go.fit(x, *init, reg_covar=REG, max_iter=100, tol=1e-3)
    change = np.abs(np.diff([-np.inf] + o["bounds"]))
    assert np.all(np.abs(change - 1e-3) > 1e-6)  # the comparison does not hinge on rounding
    assert (gm.n_iter_, gm.converged_) == (o["n_iter"], o["converged"]) and o["converged"]
    assert abs(gm.lower_bound_ - o["lower_bound"]) <= 1e-9


def test_sklearn_round_trip():
    mixture = pytest.importorskip("sklearn.mixture")
    from asvspoof2021_air_amd import DiagGMM, GMMBackend  # exported from the package
    assert GMMBackend is not None
    x, init = CASES["lfcc_like"]
    gm = _sklearn_fit(x, init, 3, 0.0)
    m = DiagGMM.from_sklearn(gm, device="cpu")
    assert (m.n_components, m.n_features, m.reg_covar) == (4, 20, REG)
    assert m.weights_.dtype == torch.float64 and np.array_equal(m.means_.numpy(), gm.means_)
    back = m.to_sklearn()
    assert isinstance(back, mixture.GaussianMixture) and back.covariance_type == "diag"
    for a in ("weights_", "means_", "covariances_"):
        assert np.array_equal(getattr(back, a), getattr(gm, a))
    x64 = x.astype(np.float64)
    assert np.allclose(back.score_samples(x64), gm.score_samples(x64), rtol=0, atol=1e-9)  # usable as fitted
    assert np.array_equal(back.predict(x64), gm.predict(x64))
    assert (back.n_iter_, back.converged_, back.lower_bound_) == (gm.n_iter_, gm.converged_, gm.lower_bound_)
    state = m.state_dict()
    m2 = DiagGMM(4, 20, device="cpu").load_state_dict(state)
    assert torch.equal(m2.covariances_, m.covariances_) and m2.n_iter_ == 3
    full = mixture.GaussianMixture(n_components=2, covariance_type="full").fit(x64[:, :3])
    with pytest.raises(ValueError):
        DiagGMM.from_sklearn(full, device="cpu")


def test_host_side_refusals():
    from asvspoof2021_air_amd import _hip, build, gmm
    build.build(verbose=False)
    L = _hip.lib()
    for K, D in ((0, 60), (1025, 60), (512, 0), (512, 129)):
        with pytest.raises(ValueError):
            gmm.DiagGMM(K, D, device="cpu")
        assert L.air_gmm_ws_bytes(ctypes.c_int64(1024), K, D) == 0
        assert L.air_gmm_params_doubles(K, D) == 0 and L.air_gmm_stats_doubles(K, D) == 0
    assert L.air_gmm_stats_doubles(512, 60) == 512 + 2 * 512 * 60 + 2
    # the C entry points refuse before any HIP call (no GPU here): host buffers stand in for the pointers
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    n0, st = ctypes.c_void_p(0), ctypes.c_void_p(0)
    acc = lambda lay, B, T, K, D: L.air_gmm_accumulate(p, lay, B, T, n0, p, K, D, p, p, ctypes.c_size_t(1 << 30), st)
    lik = lambda lay, B, T, K, D: L.air_gmm_loglik(p, lay, B, T, n0, p, K, D, p, p, p, ctypes.c_size_t(1 << 30), st)
    for f in (acc, lik):
        assert f(0, 1, 8, 1025, 60) == -2 and f(0, 1, 8, 0, 60) == -2 and f(1, 1, 8, 4, 129) == -2  # AIR_EUNSUPPORTED
        assert f(2, 1, 8, 4, 60) == -1 and f(-1, 1, 8, 4, 60) == -1 and f(0, 0, 8, 4, 60) == -1    # AIR_EINVAL
        assert f(0, 2, 1 << 30, 4, 60) == -2                                                      # B * Tcap = 2^31
    assert L.air_gmm_accumulate(p, 0, 1, 4096, n0, p, 4, 60, p, p, ctypes.c_size_t(16), st) == -4  # AIR_EWORKSPACE
    assert L.air_gmm_prepare(p, p, p, 2000, 60, p, st) == -2
    assert L.air_gmm_mstep(p, 4, 200, ctypes.c_double(1e-6), p, p, p, p, st) == -2
    # the Python layer: layouts, CPU tensors, shapes
    m = gmm.DiagGMM(4, 3, device="cpu").set_params(np.full(4, 0.25), np.zeros((4, 3)), np.ones((4, 3)))
    with pytest.raises(ValueError):
        m.accumulate(torch.zeros(8, 3), layout="dtb")
    with pytest.raises(_hip.AirError):
        m.accumulate(torch.zeros(8, 3))
    with pytest.raises(ValueError):
        m.set_params(np.full(3, 1 / 3), np.zeros((4, 3)), np.ones((4, 3)))
    with pytest.raises(RuntimeError):
        gmm.DiagGMM(4, 3, device="cpu").state_dict()


def test_workspace_grows_by_at_most_16_bytes_per_frame():
    from asvspoof2021_air_amd import build, gmm
    build.build(verbose=False)
    N, K, D = 1 << 20, 512, 60
    a, b = gmm.ws_bytes(N, K, D), gmm.ws_bytes(2 * N, K, D)
    assert 0 < a < b and b - a <= 16 * N
    assert gmm.ws_bytes(1 << 31, K, D) == 0 and gmm.ws_bytes(0, K, D) == 0
    assert gmm.frame_tile() >= 16 and gmm.frame_tile() % 16 == 0
