"""fp64 numpy restatements of the wave-per-row ECAPA kernels (csrc/ecapa_ops.hip, csrc/ecapa_bf16.hip), and the inputs
that tests/test_ecapa_rows_cpu.py and tests/test_ecapa_rows_gpu.py share.

Every function works on the last axis (time) of (..., T) arrays and returns a dict.  Next to each result ``k`` it
returns ``k_scale``: per row, the sum of the MAGNITUDES of the terms that form an element of that row - the quantity
an fp32 evaluation's rounding error is proportional to.  The GPU tests hold a kernel to ``tol * k_scale`` row by row,
so a kernel that is wrong only on rows of small magnitude cannot hide behind the tensor's maximum.

The clamp of the two standard deviations is the kernel's: ``clamp_min`` rounded to float32; a row is clamped unless its
variance is GREATER than that, and a clamped row passes no gradient through the deviation (torch.clamp(min=) passes
none below the bound either; the two differ only at equality, which no test input hits)."""
import numpy as np
import torch

from oracle.filler import synth_feat

FWD_TOL = 2e-5   # the project's bound for fp32 forward kernels (tests/test_ecapa_kernels_gpu.py)
BWD_TOL = 1e-4   # ... for backward kernels and reductions
ASP_CLAMP = 1e-4  # hard-coded in asp_fwd / asp_bwd
FLT_MIN = float(np.finfo(np.float32).tiny)


def c32(c):
    """The clamp as the kernel holds it."""
    return float(np.float32(c))


def f64(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def row_stats(x, clamp_min=1e-4):
    """mean over time and sqrt(clamp(unbiased variance, clamp_min)) per row."""
    x = f64(x)
    T = x.shape[-1]
    c = c32(clamp_min)
    mean = x.mean(-1)
    d = x - mean[..., None]
    var = (d * d).sum(-1) / max(T - 1, 1)
    mag = np.abs(x) + np.abs(mean)[..., None]  # magnitude of the terms of x - mean
    return {"mean": mean, "mean_scale": np.abs(x).sum(-1) / T,
            "var": var, "clamped": ~(var > c), "std": np.sqrt(np.maximum(var, c)),
            # d(std) = d(var) / (2 std) and d(var) <= 2 eps sqrt(sum d^2) sqrt(sum mag^2) / (T - 1): the deviation's own
            # scale is the deviation formed from the magnitudes (and the clamp, a term of the maximum)
            "std_scale": np.sqrt(np.maximum((mag * mag).sum(-1) / max(T - 1, 1), c)),
            "sum": x.sum(-1), "sum_scale": np.abs(x).sum(-1)}


def row_stats_bwd(x, dmean, dstd, clamp_min=1e-4, dx_old=None, relu_mask=False):
    """dx = [dx_old +] dmean / T + dstd (x - mean) / ((T - 1) std), the dstd term only on unclamped rows; relu_mask
    zeroes the result where x <= 0; rowsum = the time sums of the result."""
    x = f64(x)
    T = x.shape[-1]
    st = row_stats(x, clamp_min)
    k0 = f64(dmean) / T if dmean is not None else np.zeros(x.shape[:-1])
    k1 = np.zeros(x.shape[:-1])
    if dstd is not None:
        k1 = np.where(st["clamped"], 0.0, f64(dstd) / ((T - 1) * st["std"]))
    d = x - st["mean"][..., None]
    dx = k0[..., None] + k1[..., None] * d
    scale = np.abs(k0) + np.abs(k1) * np.abs(d).max(-1)
    if dx_old is not None:
        dx = dx + f64(dx_old)
        scale = scale + np.abs(f64(dx_old)).max(-1)
    if relu_mask:
        dx = np.where(x > 0, dx, 0.0)
    return {"dx": dx, "dx_scale": scale, "rowsum": dx.sum(-1), "rowsum_scale": np.abs(dx).sum(-1), "k0": k0, "k1": k1,
            "clamped": st["clamped"]}


def sigmoid(z):
    z = f64(z)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def se_fwd(x, z, res):
    """out = x * sigmoid(z) + res."""
    x, res = f64(x), f64(res)
    g = sigmoid(z)[..., None]
    return {"out": x * g + res, "out_scale": (np.abs(x) * g + np.abs(res)).max(-1), "g": g[..., 0]}


def se_bwd(x, z, dout):
    """dx = dout * g; dz = g (1 - g) sum_t dout x.  The kernel forms 1 - g in fp32: its terms are 1 and g, so the row
    scale of dz is g (1 + g) sum |dout x| (a saturated gate, g == 1.0f, returns dz == 0 where fp64 has ~e^-z).
    fp32 holds no g below its normal range (expf(-z) overflows at z < -88.7 and g becomes exactly 0): ``*_abs`` is that
    absolute floor, FLT_MIN of g, carried through the same products."""
    x, dout = f64(x), f64(dout)
    g = sigmoid(z)
    return {"dx": dout * g[..., None], "dx_scale": np.abs(dout).max(-1) * g, "dx_abs": FLT_MIN * np.abs(dout).max(-1),
            "dz": (dout * x).sum(-1) * g * (1.0 - g), "dz_scale": np.abs(dout * x).sum(-1) * g * (1.0 + g),
            "dz_abs": FLT_MIN * np.abs(dout * x).sum(-1), "g": g}


def softmax(a):
    a = f64(a)
    e = np.exp(a - a.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def asp_fwd(x, a=None, w=None):
    """w = softmax_T(a) (or the given, stored, weights); mu = sum x w; q = sum x^2 w - mu^2; sg = sqrt(clamp(q, 1e-4)).
    sg is judged through sg^2 on the scale of its terms, sum x^2 w + mu^2 (+ the clamp, a term of the maximum)."""
    x = f64(x)
    w = softmax(a) if w is None else f64(w)
    c = c32(ASP_CLAMP)
    mu = (x * w).sum(-1)
    s2 = (x * x * w).sum(-1)
    q = s2 - mu * mu
    return {"w": w, "w_scale": w.max(-1), "mu": mu, "mu_scale": (np.abs(x) * w).sum(-1), "q": q,
            "clamped": ~(q > c), "sg2": np.maximum(q, c), "sg2_scale": s2 + mu * mu + c, "sg": np.sqrt(np.maximum(q, c)),
            "s2": s2}


def asp_bwd(x, w, dmu, dsg, dx_old=None):
    """Backward of the pooling evaluated AT the given weights (the kernel keeps the stored w as its leaf):
    dq = dsg / (2 sg) on unclamped rows, dm = dmu - 2 mu dq; dx = [dx_old +] dm w + 2 dq x w;
    d logits = w (dw - sum_t w dw), dw = dm x + dq x^2."""
    x, w, dmu, dsg = f64(x), f64(w), f64(dmu), f64(dsg)
    f = asp_fwd(x, w=w)
    dq = np.where(f["clamped"], 0.0, dsg / (2.0 * f["sg"]))
    dm = dmu - 2.0 * f["mu"] * dq
    dm_mag = np.abs(dmu) + 2.0 * np.abs(f["mu"] * dq)
    dw = dm[..., None] * x + dq[..., None] * x * x
    dw_mag = dm_mag[..., None] * np.abs(x) + np.abs(dq)[..., None] * x * x
    dot = (w * dw).sum(-1, keepdims=True)
    dot_mag = (w * dw_mag).sum(-1, keepdims=True)
    dx = dm[..., None] * w + 2.0 * dq[..., None] * x * w
    dx_scale = (w * (dm_mag[..., None] + 2.0 * np.abs(dq)[..., None] * np.abs(x))).max(-1)
    if dx_old is not None:
        dx = dx + f64(dx_old)
        dx_scale = dx_scale + np.abs(f64(dx_old)).max(-1)
    da = w * (dw - dot)
    return {"dx": dx, "dx_scale": dx_scale, "da": da, "da_scale": (w * (dw_mag + dot_mag)).max(-1), "dq": dq,
            "clamped": f["clamped"]}


def channel_sum(x):
    """out[c] = sum over b and t of x[b, c, t]."""
    x = f64(x)
    return {"out": x.sum((0, 2)), "out_scale": np.abs(x).sum((0, 2))}


def rel_to_scale(got, want, scale, absolute=0.0):
    """max over the tensor of (|got - want| - absolute) / row scale (rows of scale 0 must be exact)."""
    got, want, scale, absolute = f64(got), f64(want), f64(scale), f64(absolute)
    assert got.shape == want.shape, (got.shape, want.shape)
    while scale.ndim < want.ndim:
        scale = scale[..., None]
    while absolute.ndim and absolute.ndim < want.ndim:
        absolute = absolute[..., None]
    err = np.maximum(np.abs(got - want) - absolute, 0.0)
    if not np.isfinite(got).all():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / np.broadcast_to(scale, err.shape))
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------
# Inputs.  Each builder returns float32 numpy arrays; the GPU tests run the kernels on them and the CPU test runs
# the fp32 kernel-order restatement on the same arrays.
ROWS = [(1, 1), (1, 7), (3, 5), (2, 6)]  # B * C = 1, 7, 15, 12: a ragged last workgroup (4 rows each) but for the last
RS_LENGTHS = [2, 3, 63, 64, 65, 128, 129, 1023, 1024, 1025, 1100]
ASP_LENGTHS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 1100]
CLAMPS = [1e-4, 1e-3, 1e-2]


def _n(shape, seed, scale=1.0):
    return synth_feat(tuple(shape), seed, scale=scale).numpy().astype(np.float32)


def _rs(x, seed):
    B, C, _ = x.shape
    return {"x": x, "dmean": _n((B, C), seed + 1), "dstd": _n((B, C), seed + 2), "dx0": _n(x.shape, seed + 3),
            "clamp_min": 1e-4}


def clamp_rows(c, T=77):
    """(1, 5, T): all zero | constant 5.0 | std 0.5 sqrt(c) | std 2 sqrt(c) | plain noise.  The two scaled rows sit on
    an offset of 4 deviations, so every frame is positive (a ReLU output that the mask keeps)."""
    z = synth_feat((2, T), 77).double().numpy()
    z = (z - z.mean(-1, keepdims=True)) / z.std(-1, ddof=1, keepdims=True)
    x = np.zeros((1, 5, T), np.float64)
    x[0, 1] = 5.0
    for r, k in ((2, 0.5), (3, 2.0)):
        s = k * np.sqrt(c)
        x[0, r] = s * z[r - 2] + 4.0 * s
    x[0, 4] = synth_feat((T,), 78).double().numpy() * 0.5
    assert (x[0, 2:4] > 0).all()
    return x.astype(np.float32)


def rs_cases():
    """name -> inputs of row_stats / row_stats_bwd / row_sum."""
    out = {}
    for B, C in ROWS:
        out["rows-%dx%d" % (B, C)] = _rs(_n((B, C, 77), 100 + C, 0.5), 110 + C)
    for T in RS_LENGTHS:
        out["T-%d" % T] = _rs(_n((1, 3, T), 200 + T, 0.5) + np.float32(0.25), 300 + T)
    x = _n((1, 3, 200), 400, 0.5)
    x *= np.array([1e-3, 1.0, 1e3], np.float32)[None, :, None]
    out["magnitudes"] = _rs(x, 410)
    out["magnitudes"]["clamp_min"] = 1e-12  # (the 1e-3 row has variance 2.5e-7: keep its deviation alive)
    for c in CLAMPS:
        d = _rs(clamp_rows(c), 420)
        d["clamp_min"] = c
        out["clamp-%g" % c] = d
    return out


def _asp(x, a, seed):
    B, C, _ = x.shape
    return {"x": x, "a": a, "dout": _n((B, 2 * C), seed + 1), "dx0": _n(x.shape, seed + 2)}


def softmax_range_rows(T=83):
    """(1, 5, T) x and logits: logits in [-60, -40] | one logit 100 above the rest | all-equal logits |
    constant x | all-zero x."""
    x = np.maximum(_n((1, 5, T), 500), 0)
    a = _n((1, 5, T), 501)
    u = synth_feat((T,), 502).numpy()
    a[0, 0] = -50.0 + 10.0 * np.clip(u, -1, 1)
    a[0, 1, 40] += 100.0
    x[0, 1, 40] = 1.5
    a[0, 2] = 0.75
    x[0, 3] = 1.0
    x[0, 4] = 0.0
    return x.astype(np.float32), a.astype(np.float32)


def deep_negative_logits(shape):
    """Logits in [-120, -100]: exp() of every one underflows fp32 (e^-104 < 2^-149), so a running maximum that starts
    at 0 instead of -inf leaves a sum of zero.  ([-60, -40] does not show that: e^-60 is an ordinary float.)"""
    return (-110.0 + 10.0 * np.clip(_n(shape, 1021), -1, 1)).astype(np.float32)


def asp_cases():
    """name -> inputs of asp_fwd / asp_bwd (x is a ReLU output, as in the model)."""
    out = {}
    for B, C in ROWS:
        out["rows-%dx%d" % (B, C)] = _asp(np.maximum(_n((B, C, 83), 600 + C), 0), _n((B, C, 83), 610 + C), 620 + C)
    for T in ASP_LENGTHS:
        out["T-%d" % T] = _asp(np.maximum(_n((1, 3, T), 700 + T), 0) + np.float32(0.125), _n((1, 3, T), 800 + T), 900 + T)
    x = np.maximum(_n((1, 3, 200), 1000), 0) + np.float32(0.125)
    x *= np.array([1e-3, 1.0, 1e3], np.float32)[None, :, None]  # (the 1e-3 row's deviation is clamped; its mu is not)
    out["magnitudes"] = _asp(x, _n((1, 3, 200), 1001), 1002)
    xs, as_ = softmax_range_rows()
    out["softmax-range"] = _asp(xs, as_, 1010)
    out["logits-below-underflow"] = _asp(np.maximum(_n((1, 3, 83), 1020), 0), deep_negative_logits((1, 3, 83)), 1022)
    return out


def large_mean_case():
    """x = 10 + 0.1 noise, T = 750: sum x^2 w - mu^2 cancels four digits."""
    x = (10.0 + 0.1 * synth_feat((2, 3, 750), 1100).double().numpy()).astype(np.float32)
    return _asp(x, _n((2, 3, 750), 1101), 1102)


def large_mean_bound(T):
    """n 2^-24 (sum x^2 w + mu^2), n = the kernel's chain: frames per lane + 6 tree levels + 2."""
    return (-(-T // 64) + 6 + 2) * 2.0 ** -24


SE_Z = [0.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4]


def se_cases():
    out = {}
    for B, C in ROWS:
        out["rows-%dx%d" % (B, C)] = {"x": _n((B, C, 61), 1200 + C), "z": _n((B, C), 1210 + C), "res": _n((B, C, 61), 1220 + C),
                                      "dout": _n((B, C, 61), 1230 + C)}
    x = _n((1, 3, 130), 1300)
    x *= np.array([1e-3, 1.0, 1e3], np.float32)[None, :, None]
    out["magnitudes"] = {"x": x, "z": _n((1, 3), 1301), "res": _n((1, 3, 130), 1302), "dout": _n((1, 3, 130), 1303)}
    out["gate-range"] = {"x": _n((1, 9, 61), 1310), "z": np.array([SE_Z], np.float32), "res": _n((1, 9, 61), 1311),
                         "dout": _n((1, 9, 61), 1312)}
    return out


CHANNEL_SUM_SHAPES = [(5, 512, 10), (7, 1024, 9), (3, 4096, 3), (1, 8, 300), (4, 64, 1)]


def channel_sum_input(shape):
    return _n(shape, 1400 + shape[0])
