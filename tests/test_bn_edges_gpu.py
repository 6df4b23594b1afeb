"""GPU: the fp32 BatchNorm kernels (csrc/norm_act.hip) and the two convolution epilogues that feed them (csrc/conv_wino4.hip)
against the fp64 oracle of tests/bn_edges_oracle.py, per channel, on inputs whose channels sit at the conditioning edges:
|mean| >> std, variance 0, an outlier as the shift, variance << eps, squares ~ 1e12, exact sums.

* The bounds are the oracle's, derived from the summation structure (see its docstring), never measured on a kernel.
  tests/test_bn_edges_cpu.py shows that the kernels' arithmetic, emulated, stays inside them and that the same sums
  WITHOUT the shift K miss the variance bound on classes 1 and 2 by four orders of magnitude and more.
* Every bounded assertion prints max error / bound per class (pytest -s), so the margin is on record.
* The ReLU mask of the backward is taken from the STORED forward output: one element masked differently in forward and
  backward moves dbeta by that element's |g|, orders of magnitude above dbeta's bound; with a gradient of ones the
  count of passed elements must match exactly.
* The variance itself is read through the running variance at momentum 1, which is the unbiased variance and nothing
  else."""
import functools

import numpy as np
import pytest
import torch

import bn_edges_oracle as bo

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def ops():
    from asvspoof2021_air_amd import ops
    return ops


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def N_(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(shape):
    return bo.case(shape)


def held(what, got, want, bound, axis=1):
    g = N_(got) if torch.is_tensor(got) else got
    assert np.isfinite(g).all(), what + ": not finite"
    rs = bo.ratios(g, want, bound, axis)
    print(bo.fmt(what, rs))
    assert bo.worst(rs) <= 1.0, "%s: max error / bound per class %s" % (what, rs)


def gpu_stats(ops, d, momentum=bo.MOMENTUM):
    rm, rv = G(d["rm"]), G(d["rv"])
    out = ops.bn_stats(G(d["x"]), G(d["gamma"]), G(d["beta"]), rm, rv, bo.EPS, momentum)
    return out + (rm, rv)


# ---- statistics from x -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", bo.SHAPES)
def test_statistics_from_x(ops, shape):
    d = case(shape)
    C = shape[1]
    mean, invstd, scale, shift, rm, rv = gpu_stats(ops, d)
    st = bo.stats(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"])
    held("mean", mean, st["mean"], st["mean_bound"], 0)
    held("invstd", invstd, st["invstd"], st["invstd_bound"], 0)
    held("running mean", rm, st["running_mean"], st["running_mean_bound"], 0)
    held("running var", rv, st["running_var"], st["running_var_bound"], 0)
    co = bo.coeffs(N_(mean), N_(invstd), d["gamma"], d["beta"])
    held("scale", scale, co["scale"], co["scale_bound"], 0)
    held("shift", shift, co["shift"], co["shift_bound"], 0)
    # momentum 1: the running statistics are the mean and the unbiased variance themselves
    mean1, _, _, _, rm1, rv1 = gpu_stats(ops, d, momentum=1.0)
    s1 = bo.stats(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], momentum=1.0)
    held("variance (running var, momentum 1)", rv1, s1["running_var"], s1["running_var_bound"], 0)
    held("mean (running mean, momentum 1)", rm1, s1["running_mean"], s1["running_mean_bound"], 0)
    assert torch.equal(mean1, mean)
    # exact classes
    m7, _, unb7 = bo.exact_alternating(shape)
    mean, invstd, rm1, rv1 = N_(mean), N_(invstd), N_(rm1), N_(rv1)
    for c in range(C):
        if c % 8 == 3:  # the shifted data is exactly zero
            assert mean[c] == F32(3.25) and invstd[c] == bo.invstd_of_zero_variance(), (c, mean[c], invstd[c])
        if c % 8 == 7:
            assert mean[c] == F32(m7) and rm1[c] == F32(m7) and rv1[c] == F32(unb7), (c, mean[c], rv1[c], m7, unb7)
    if shape == (1, 8, 1, 1):
        # N = 1: variance 0, and the kernel's N > 1 ? ... : var guard leaves running_var = (1 - momentum) rv exactly
        # (PyTorch refuses N = 1 in training mode: this pins the kernel's documented convention)
        assert np.array_equal(mean, d["x"].reshape(-1))
        assert (invstd == bo.invstd_of_zero_variance()).all()
        assert (rv1 == 0).all()
        assert np.array_equal(N_(rv), (F32(1) - F32(bo.MOMENTUM)) * d["rv"])
        for t in (scale, shift, rm, rv):
            assert bool(torch.isfinite(t).all())


# ---- apply -----------------------------------------------------------------------------------------------------
EVAL_MEAN = np.array([0.0, 1000.0, -1e4, 3.25, 0.0, 0.0, 0.0, 0.0], F32)
EVAL_VAR = np.array([1.0, 0.01, 1.0, 0.0, 1.0, 1e-12, 1e12, 1.0], F32)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", bo.SHAPES)
def test_apply(ops, shape, relu):
    d = case(shape)
    C = shape[1]
    x = G(d["x"])
    _, _, scale, shift, _, _ = gpu_stats(ops, d)
    a = bo.apply(d["x"], N_(scale), N_(shift), relu)
    held("apply, batch statistics (relu=%s)" % relu, ops.bn_apply(x, scale, shift, relu), a["y"], a["y_bound"])
    # evaluation mode: coefficients from running statistics of the classes' own means and variances
    rm, rv = np.tile(EVAL_MEAN, C // 8), np.tile(EVAL_VAR, C // 8)
    sc, sh = ops.bn_eval_coeffs(G(d["gamma"]), G(d["beta"]), G(rm), G(rv), bo.EPS)
    ec = bo.eval_coeffs(d["gamma"], d["beta"], rm, rv)
    held("eval scale", sc, ec["scale"], ec["scale_bound"], 0)
    held("eval shift", sh, ec["shift"], ec["shift_bound"], 0)
    a = bo.apply(d["x"], N_(sc), N_(sh), relu)
    held("apply, running statistics (relu=%s)" % relu, ops.bn_apply(x, sc, sh, relu), a["y"], a["y_bound"])


# ---- backward, own pass ----------------------------------------------------------------------------------------
def passed_by_the_forward(ops, x, scale, shift):
    """The mask the backward must rebuild: where the stored relu(batchnorm(x)) is positive."""
    return ops.bn_apply(x, scale, shift, True) > 0


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", bo.SHAPES)
def test_backward_own_pass(ops, shape, relu):
    d = case(shape)
    x, dy, gamma, beta = G(d["x"]), G(d["dy"]), G(d["gamma"]), G(d["beta"])
    mean, invstd, scale, shift, _, _ = gpu_stats(ops, d)
    mask = passed_by_the_forward(ops, x, scale, shift) if relu else None
    dx, dgamma, dbeta = ops.bn_bwd(x, dy, mean, invstd, gamma, beta, relu)
    b = bo.bwd(d["x"], d["dy"], N_(mean), N_(invstd), d["gamma"], d["beta"], None if mask is None else N_(mask))
    held("dbeta (relu=%s)" % relu, dbeta, b["dbeta"], b["dbeta_bound"], 0)
    held("dgamma (relu=%s)" % relu, dgamma, b["dgamma"], b["dgamma_bound"], 0)
    held("dx (relu=%s)" % relu, dx, b["dx"], b["dx_bound"])
    acc = G(d["base"]).clone()
    dx2, dg2, db2 = ops.bn_bwd(x, dy, mean, invstd, gamma, beta, relu, dx=acc, accumulate=True)
    assert dx2 is acc and torch.equal(dg2, dgamma) and torch.equal(db2, dbeta)
    b2 = bo.bwd(d["x"], d["dy"], N_(mean), N_(invstd), d["gamma"], d["beta"], None if mask is None else N_(mask), d["base"])
    held("dx, accumulate (relu=%s)" % relu, dx2, b2["dx"], b2["dx_bound"])
    if relu:
        # a gradient of ones: dbeta counts the elements the backward passes - exactly (integers below 2^24)
        _, _, cnt = ops.bn_bwd(x, torch.ones_like(x), mean, invstd, gamma, beta, True)
        want = mask.sum(dim=[i for i in range(x.dim()) if i != 1]).float()
        assert torch.equal(cnt, want), "the backward passes %s elements per channel, the forward stored %s positive" % (
            cnt.tolist(), want.tolist())


# ---- statistics from the conv epilogue -------------------------------------------------------------------------
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("cfg", bo.CONV_STATS)
def test_statistics_from_the_conv_epilogue(ops, cfg, split):
    from asvspoof2021_air_amd import _hip
    B, Cin, H, W, Cout = cfg
    d = bo.conv_stats_case(cfg)
    gamma, beta = G(d["gamma"]), G(d["beta"])
    with _hip.options(WINO4_SPLIT=split):
        y, rec = ops.conv2d_fwd(G(d["x"]), G(d["w"]), 1, 1, residual=G(d["res"]), stats=True)
    assert rec is not None
    rm0, rv0, rm1, rv1 = G(d["rm"]), G(d["rv"]), G(d["rm"]), G(d["rv"])
    own = ops.bn_stats(y, gamma, beta, rm0, rv0)
    fused = ops.bn_stats(y, gamma, beta, rm1, rv1, stats_in=rec)
    yn = N_(y)
    K = bo.record_shift(N_(rec.view(torch.float32)), Cout)
    so = bo.stats(yn, d["gamma"], d["beta"], d["rm"], d["rv"])
    sf = bo.stats(yn, d["gamma"], d["beta"], d["rm"], d["rv"], K=K)
    print("records' shift K against the mean, in deviations, worst per class: " + " ".join(
        "%d:%.3g" % (k, max(abs(K[c] - sf["mean"][c]) * sf["invstd"][c] for c in range(k, Cout, 8))) for k in range(8)))
    for name, got, st, r_m, r_v in (("own pass", own, so, rm0, rv0), ("records", fused, sf, rm1, rv1)):
        held(name + ": mean", got[0], st["mean"], st["mean_bound"], 0)
        held(name + ": invstd", got[1], st["invstd"], st["invstd_bound"], 0)
        held(name + ": running mean", r_m, st["running_mean"], st["running_mean_bound"], 0)
        held(name + ": running var", r_v, st["running_var"], st["running_var_bound"], 0)
        co = bo.coeffs(N_(got[0]), N_(got[1]), d["gamma"], d["beta"])
        held(name + ": scale", got[2], co["scale"], co["scale_bound"], 0)
        held(name + ": shift", got[3], co["shift"], co["shift_bound"], 0)
    for i, k in ((0, "mean"), (1, "invstd")):
        held("records against own pass: " + k, fused[i], N_(own[i]).astype(np.float64), so[k + "_bound"] + sf[k + "_bound"], 0)
    held("records against own pass: running var", rv1, N_(rv0).astype(np.float64),
         so["running_var_bound"] + sf["running_var_bound"], 0)
    # the variance itself, through momentum 1
    rm2, rv2 = G(d["rm"]), G(d["rv"])
    ops.bn_stats(y, gamma, beta, rm2, rv2, bo.EPS, 1.0, stats_in=rec)
    s1 = bo.stats(yn, d["gamma"], d["beta"], d["rm"], d["rv"], momentum=1.0, K=K)
    held("records: variance (running var, momentum 1)", rv2, s1["running_var"], s1["running_var_bound"], 0)


# ---- backward sums from the dgrad epilogue ---------------------------------------------------------------------
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("cfg", bo.CONV_DGRAD)
def test_backward_sums_from_the_dgrad_epilogue(ops, cfg, split):
    from asvspoof2021_air_amd import _hip
    d = bo.conv_dgrad_case(cfg)
    x, w, dy, gamma, beta = G(d["x"]), G(d["w"]), G(d["dy"]), G(d["gamma"]), G(d["beta"])
    mean, invstd, scale, shift = ops.bn_stats(x, gamma, beta)
    with _hip.options(WINO4_SPLIT=split):
        dA0 = ops.conv2d_dgrad(dy, w, x.shape, 1, 1)
        dA1, sums = ops.conv2d_dgrad(dy, w, x.shape, 1, 1, bn=(x, mean, invstd, gamma, beta))
    assert sums is not None
    assert torch.equal(dA0, dA1), "the sums changed the data gradient"
    mask = passed_by_the_forward(ops, x, scale, shift)
    dx0, dg0, db0 = ops.bn_bwd(x, dA0, mean, invstd, gamma, beta, relu=True)
    dx1, dg1, db1 = ops.bn_bwd(x, dA1, mean, invstd, gamma, beta, relu=True, sums_in=sums)
    b = bo.bwd(d["x"], N_(dA1), N_(mean), N_(invstd), d["gamma"], d["beta"], N_(mask))
    for name, dx, dg, db in (("own pass", dx0, dg0, db0), ("epilogue sums", dx1, dg1, db1)):
        held(name + ": dbeta", db, b["dbeta"], b["dbeta_bound"], 0)
        held(name + ": dgamma", dg, b["dgamma"], b["dgamma_bound"], 0)
        held(name + ": dx", dx, b["dx"], b["dx_bound"])
    held("epilogue sums against own pass: dbeta", db1, N_(db0).astype(np.float64), 2 * b["dbeta_bound"], 0)
    held("epilogue sums against own pass: dgamma", dg1, N_(dg0).astype(np.float64), 2 * b["dgamma_bound"], 0)
    held("epilogue sums against own pass: dx", dx1, N_(dx0).astype(np.float64), 2 * b["dx_bound"])
