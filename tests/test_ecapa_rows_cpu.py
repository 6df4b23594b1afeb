"""CPU: the oracle of the wave-per-row ECAPA kernels (tests/ecapa_rows_oracle.py) against torch fp64 autograd, and an
fp32 numpy restatement of each kernel's arithmetic IN KERNEL ORDER (lane-strided partial sums, then the 64-lane
butterfly of air_wave_sum) against the oracle on exactly the inputs of tests/test_ecapa_rows_gpu.py.

The restatement alone must stay within HALF of every tolerance the GPU tests use: what is left belongs to the kernel.
If an input cannot meet that, the input is wrong for the tolerance, not the other way round.  The measured fractions
are printed (pytest -s) and recorded in the GPU module's docstring."""
import numpy as np
import pytest
import torch

import ecapa_rows_oracle as eo
from ecapa_rows_oracle import BWD_TOL, FWD_TOL, rel_to_scale

F = np.float32
LANE = np.arange(64)


# ---- fp32 restatements -----------------------------------------------------------------------------------------
def tree(v):
    """air_wave_sum: v += shfl_xor(v, o) for o = 32 .. 1 (every lane ends with the same bits)."""
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., LANE ^ o]
    return v[..., 0]


def lanes(a, fill=0.0):
    """(..., T) -> (..., K, 64) with frame t at [t // 64, t % 64], and the mask of real frames."""
    T = a.shape[-1]
    K = -(-T // 64)
    p = np.full(a.shape[:-1] + (K * 64,), fill, a.dtype)
    p[..., :T] = a
    m = np.zeros(K * 64, bool)
    m[:T] = True
    return p.reshape(a.shape[:-1] + (K, 64)), m.reshape(K, 64)


def fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def lane_sum(terms):
    v, m = lanes(terms)
    s = np.zeros(v.shape[:-2] + (64,), F)
    for k in range(v.shape[-2]):
        s = np.where(m[k], s + v[..., k, :], s)
    return tree(s)


def lane_fma_sum(a, b):
    va, m = lanes(a)
    vb, _ = lanes(b)
    s = np.zeros(va.shape[:-2] + (64,), F)
    for k in range(va.shape[-2]):
        s = np.where(m[k], fma(va[..., k, :], vb[..., k, :], s), s)
    return tree(s)


def k_row_stats(x, clamp_min):
    T = x.shape[-1]
    m = lane_sum(x) / F(T)
    d = x - m[..., None]
    q = lane_fma_sum(d, d) / F(T - 1)
    return m, np.sqrt(np.maximum(q, F(clamp_min)))


def k_row_stats_bwd(x, m, sd, dmean, dstd, clamp_min, dx0=None, relu_mask=False, old_predicate=False):
    T = x.shape[-1]
    k0 = dmean / F(T)
    live = sd * sd > F(clamp_min) if old_predicate else sd > np.sqrt(F(clamp_min))
    k1 = np.where(live, dstd / (F(T - 1) * sd), F(0))
    v = k0[..., None] + k1[..., None] * (x - m[..., None])
    if dx0 is not None:
        v = v + dx0
    if relu_mask:
        v = np.where(x > 0, v, F(0))
    return v.astype(F), lane_sum(v.astype(F))


def k_sigmoid(z):
    with np.errstate(over="ignore"):
        return (F(1) / (F(1) + np.exp(-z.astype(F)))).astype(F)


def k_se_fwd(x, z, res):
    return fma(x, np.broadcast_to(k_sigmoid(z)[..., None], x.shape), res)


def k_se_bwd(x, z, dout):
    g = k_sigmoid(z)
    acc = lane_fma_sum(dout, x)
    return dout * g[..., None], acc * g * (F(1) - g)


def k_asp_fwd(x, a):
    with np.errstate(under="ignore"):
        e = np.exp(a - a.max(-1, keepdims=True)).astype(F)
        w = (e / lane_sum(e)[..., None]).astype(F)
        s1 = lane_fma_sum(x, w)
        s2 = lane_fma_sum(x * x, w)
    return w, s1, np.sqrt(np.maximum(s2 - s1 * s1, F(1e-4))), s2


def k_asp_bwd(x, w, mu, sg, dmu, dsg, dx0=None):
    with np.errstate(under="ignore"):
        dq = np.where(sg > np.sqrt(F(1e-4)), dsg / (F(2) * sg), F(0)).astype(F)
        dm = dmu - F(2) * mu * dq
        dwv = dm[..., None] * x + dq[..., None] * x * x
        dot = lane_fma_sum(w, dwv)
        g = dm[..., None] * w + F(2) * dq[..., None] * x * w
        if dx0 is not None:
            g = dx0 + g
        da = (w * (dwv - dot[..., None])).astype(F)
    return g.astype(F), da, lane_sum(da)


def k_channel_sum(x):
    """256 threads stride one (b, c) plane in fp32; planes and threads are then folded in fp64."""
    B, C, S = x.shape
    n = -(-S // 256)
    p = np.zeros((B, C, n * 256), F)
    p[..., :S] = x
    p = p.reshape(B, C, n, 256)
    s = np.zeros((B, C, 256), F)
    for k in range(n):
        s = s + p[:, :, k]
    return s.astype(np.float64).sum((0, 2)).astype(F)


# ---- the oracle against fp64 autograd --------------------------------------------------------------------------
T64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))


@pytest.mark.parametrize("name", list(eo.rs_cases()))
def test_row_stats_oracle_is_autograd(name):
    d = eo.rs_cases()[name]
    c = eo.c32(d["clamp_min"])
    for relu in (False, True):
        x = np.maximum(d["x"], 0) if relu else d["x"]
        pre = T64(x).requires_grad_(True)
        r = torch.relu(pre) if relu else pre
        mean, std = r.mean(2), torch.sqrt(r.var(2).clamp(min=c))
        loss = (mean * T64(d["dmean"]) + std * T64(d["dstd"])).sum()
        if relu:
            loss = loss + (r * T64(d["dx0"])).sum()
        loss.backward()
        st = eo.row_stats(x, d["clamp_min"])
        assert rel_to_scale(st["mean"], mean.detach().numpy(), st["mean_scale"]) <= 1e-13
        assert rel_to_scale(st["std"], std.detach().numpy(), st["std_scale"]) <= 1e-13
        b = eo.row_stats_bwd(x, d["dmean"], d["dstd"], d["clamp_min"], d["dx0"] if relu else None, relu)
        assert rel_to_scale(b["dx"], pre.grad.numpy(), b["dx_scale"]) <= 1e-12, name
        assert rel_to_scale(b["rowsum"], pre.grad.sum(2).numpy(), b["rowsum_scale"]) <= 1e-12
    if name.startswith("clamp"):
        assert st["clamped"].tolist() == [[True, True, True, False, False]]
        assert (b["k1"][0, :3] == 0).all() and (b["k1"][0, 3:] != 0).all()
        assert (b["dx"][0, 0] == 0).all() and b["rowsum"][0, 0] == 0  # the dead channel under the ReLU mask


def _asp_autograd(x, a, dout):
    C = x.shape[1]
    xl, al = T64(x).requires_grad_(True), T64(a).requires_grad_(True)
    w = torch.softmax(al, 2)
    mu = (xl * w).sum(2)
    sg = torch.sqrt(((xl * xl * w).sum(2) - mu * mu).clamp(min=eo.c32(eo.ASP_CLAMP)))
    (mu * T64(dout[:, :C]) + sg * T64(dout[:, C:])).sum().backward()
    return w.detach().numpy(), mu.detach().numpy(), sg.detach().numpy(), xl.grad.numpy(), al.grad.numpy()


@pytest.mark.parametrize("name", list(eo.asp_cases()) + ["large-mean"])
def test_asp_oracle_is_autograd(name):
    d = eo.large_mean_case() if name == "large-mean" else eo.asp_cases()[name]
    C = d["x"].shape[1]
    w, mu, sg, dx, da = _asp_autograd(d["x"], d["a"], d["dout"])
    f = eo.asp_fwd(d["x"], a=d["a"])
    assert rel_to_scale(f["w"], w, f["w_scale"]) <= 1e-12
    assert rel_to_scale(f["mu"], mu, f["mu_scale"]) <= 1e-12
    assert rel_to_scale(f["sg"] ** 2, sg ** 2, f["sg2_scale"]) <= 1e-12
    b = eo.asp_bwd(d["x"], f["w"], d["dout"][:, :C], d["dout"][:, C:])
    if name == "softmax-range":
        # rows 1 (one-hot), 3 (constant x) and 4 (zero x) have q == 0 up to fp64 rounding: the clamp is taken; autograd
        # and the oracle must have taken the same side on every row for the comparison to mean anything
        assert f["clamped"].tolist() == [[False, True, False, True, True]]
        assert (b["dq"][0, [1, 3, 4]] == 0).all()
        assert np.isfinite(b["dx"]).all() and np.isfinite(b["da"]).all()
    assert rel_to_scale(b["dx"], dx, b["dx_scale"]) <= 1e-10, name
    assert rel_to_scale(b["da"], da, b["da_scale"]) <= 1e-10, name


@pytest.mark.parametrize("name", list(eo.se_cases()))
def test_se_oracle_is_autograd(name):
    d = eo.se_cases()[name]
    x, z = T64(d["x"]).requires_grad_(True), T64(d["z"]).requires_grad_(True)
    out = x * torch.sigmoid(z).unsqueeze(2) + T64(d["res"])
    out.backward(T64(d["dout"]))
    f, b = eo.se_fwd(d["x"], d["z"], d["res"]), eo.se_bwd(d["x"], d["z"], d["dout"])
    assert rel_to_scale(f["out"], out.detach().numpy(), f["out_scale"]) <= 1e-13
    assert rel_to_scale(b["dx"], x.grad.numpy(), b["dx_scale"]) <= 1e-13
    assert rel_to_scale(b["dz"], z.grad.numpy(), b["dz_scale"]) <= 1e-13
    assert np.isfinite(f["out"]).all() and np.isfinite(b["dz"]).all()


def test_channel_sum_oracle():
    x = eo.channel_sum_input((4, 64, 1))
    assert np.allclose(eo.channel_sum(x)["out"], T64(x).sum((0, 2)).numpy(), rtol=1e-14, atol=0)


# ---- the clamp predicate ---------------------------------------------------------------------------------------
def test_clamp_predicate_arithmetic():
    """The backward kernels used to decide "clamped?" as sd * sd > clamp_min with sd = sqrtf(clamp_min) from the
    forward.  In fp32 that product rounds ABOVE clamp_min for 1e-2, 1e-3 and 1e-6 (a clamped row then got the dstd term)
    and not for 1e-4, 1e-5, 2e-4 - the models' 1e-4 was luck.  sd > sqrtf(clamp_min) cannot misfire.  (numpy fp32 on the
    CPU: IEEE multiply and correctly rounded sqrt, the operations the GPU performs; the GPU clamp test confirms it.)"""
    for c, misfires in ((1e-4, False), (1e-5, False), (2e-4, False), (1e-2, True), (1e-3, True), (1e-6, True)):
        s = np.sqrt(F(c))
        assert bool(s * s > F(c)) == misfires, c
        assert not s > np.sqrt(F(c))


def test_new_predicate_leaves_the_models_clamp_unchanged():
    """At the models' clamp_min = 1e-4 the old and the new predicate give the same dx, bit for bit, on clamped and
    unclamped rows (the clamp rows: zero, constant, 0.5 sqrt(c), 2 sqrt(c), noise); at 1e-3 / 1e-2 only the old one
    disagrees with the oracle - on the 0.5 sqrt(c) row, whose x - mean is not zero."""
    for c in eo.CLAMPS:
        d = eo.rs_cases()["clamp-%g" % c]
        m, sd = k_row_stats(d["x"], c)
        assert (sd[0, :3] == np.sqrt(F(c))).all() and (sd[0, 3:] > np.sqrt(F(c))).all()
        new, _ = k_row_stats_bwd(d["x"], m, sd, d["dmean"], d["dstd"], c)
        old, _ = k_row_stats_bwd(d["x"], m, sd, d["dmean"], d["dstd"], c, old_predicate=True)
        want = eo.row_stats_bwd(d["x"], d["dmean"], d["dstd"], c)
        assert rel_to_scale(new, want["dx"], want["dx_scale"]) <= 0.5 * BWD_TOL
        if c == 1e-4:
            assert torch.equal(torch.from_numpy(old), torch.from_numpy(new))
        else:
            bad = rel_to_scale(old[0, 2], want["dx"][0, 2], want["dx_scale"][0, 2])
            print("clamp_min %g: old predicate, 0.5 sqrt(c) row off by %.3g of its scale" % (c, bad))
            assert bad > 100 * BWD_TOL
            assert np.array_equal(np.delete(old, 2, 1), np.delete(new, 2, 1))


# ---- the restatement within half of every GPU tolerance --------------------------------------------------------
def _note(worst, key, frac):
    worst[key] = max(worst.get(key, 0.0), frac)


def test_restatement_is_within_half_of_every_gpu_tolerance():
    worst = {}
    for name, d in eo.rs_cases().items():
        c = d["clamp_min"]
        for relu in (False, True):
            x = np.maximum(d["x"], 0) if relu else d["x"]
            st = eo.row_stats(x, c)
            m, sd = k_row_stats(x, c)
            _note(worst, "row mean", rel_to_scale(m, st["mean"], st["mean_scale"]) / FWD_TOL)
            _note(worst, "row std", rel_to_scale(sd, st["std"], st["std_scale"]) / FWD_TOL)
            _note(worst, "row sum", rel_to_scale(lane_sum(x), st["sum"], st["sum_scale"]) / FWD_TOL)
            b = eo.row_stats_bwd(x, d["dmean"], d["dstd"], c, d["dx0"] if relu else None, relu)
            dx, rs = k_row_stats_bwd(x, m, sd, d["dmean"], d["dstd"], c, d["dx0"] if relu else None, relu)
            _note(worst, "row_stats_bwd dx", rel_to_scale(dx, b["dx"], b["dx_scale"]) / BWD_TOL)
            _note(worst, "row_stats_bwd rowsum", rel_to_scale(rs, b["rowsum"], b["rowsum_scale"]) / BWD_TOL)
    cases = dict(eo.asp_cases())
    cases["large-mean"] = eo.large_mean_case()
    for name, d in cases.items():
        x, C = d["x"], d["x"].shape[1]
        w, mu, sg, s2 = k_asp_fwd(x, d["a"])
        assert np.isfinite(w).all() and np.isfinite(mu).all() and np.isfinite(sg).all(), name
        f = eo.asp_fwd(x, a=d["a"])
        _note(worst, "asp w", rel_to_scale(w, f["w"], f["w_scale"]) / FWD_TOL)
        fs = eo.asp_fwd(x, w=w)  # at the restatement's own stored weights
        _note(worst, "asp mu", rel_to_scale(mu, fs["mu"], fs["mu_scale"]) / FWD_TOL)
        if name == "large-mean":
            n = eo.large_mean_bound(x.shape[-1])
            _note(worst, "asp sg^2, large mean (of n 2^-24)", rel_to_scale(sg.astype(np.float64) ** 2, fs["sg2"], fs["s2"] + fs["mu"] ** 2) / n)
            continue
        _note(worst, "asp sg^2", rel_to_scale(sg.astype(np.float64) ** 2, fs["sg2"], fs["sg2_scale"]) / FWD_TOL)
        for acc in (False, True):
            dx0 = d["dx0"] if acc else None
            b = eo.asp_bwd(x, w, d["dout"][:, :C], d["dout"][:, C:], dx0)
            dx, da, rs = k_asp_bwd(x, w, mu, sg, d["dout"][:, :C], d["dout"][:, C:], dx0)
            assert np.isfinite(dx).all() and np.isfinite(da).all(), name
            _note(worst, "asp_bwd dx", rel_to_scale(dx, b["dx"], b["dx_scale"]) / BWD_TOL)
            _note(worst, "asp_bwd dlogits", rel_to_scale(da, b["da"], b["da_scale"]) / BWD_TOL)
            _note(worst, "asp_bwd rowsum", rel_to_scale(rs, da.astype(np.float64).sum(-1), np.abs(da.astype(np.float64)).sum(-1)) / BWD_TOL)
        if name == "softmax-range":
            assert sg[0, 1] == F(0.01) and sg[0, 3] == F(0.01) and sg[0, 4] == F(0.01)
    for name, d in eo.se_cases().items():
        f, b = eo.se_fwd(d["x"], d["z"], d["res"]), eo.se_bwd(d["x"], d["z"], d["dout"])
        dx, dz = k_se_bwd(d["x"], d["z"], d["dout"])
        _note(worst, "se fwd", rel_to_scale(k_se_fwd(d["x"], d["z"], d["res"]), f["out"], f["out_scale"]) / FWD_TOL)
        _note(worst, "se dx", rel_to_scale(dx, b["dx"], b["dx_scale"], b["dx_abs"]) / FWD_TOL)
        _note(worst, "se dz", rel_to_scale(dz, b["dz"], b["dz_scale"], b["dz_abs"]) / BWD_TOL)
    for shape in eo.CHANNEL_SUM_SHAPES:
        x = eo.channel_sum_input(shape)
        r = eo.channel_sum(x)
        _note(worst, "channel_sum", rel_to_scale(k_channel_sum(x), r["out"], r["out_scale"]) / BWD_TOL)
    for k, v in worst.items():
        print("restatement / tolerance  %-36s %.4f" % (k, v))
    bad = {k: v for k, v in worst.items() if not v <= 0.5}
    assert not bad, bad
