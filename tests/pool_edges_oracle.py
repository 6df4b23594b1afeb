"""fp64 numpy restatement of the attentive pooling kernels (selfatt_fwd_kernel / selfatt_bwd_kernel, csrc/pool_head.hip):
the closed forms of their header comments, the inputs that tests/test_pool_edges_cpu.py and tests/test_pool_edges_gpu.py
share, and the term-magnitude scales the kernels are held to (FWD_TOL / BWD_TOL of tests/ecapa_rows_oracle.py times a
scale; nothing (B, T)- or (B, C, T)-wide is ever compared against a tensor's maximum).

x is (B, C, T), the attention vector a is (C,), the noise is (B, T, C) as the model draws it.

  s_t = <x[:, t], a>, u_t = tanh(s_t), alpha = softmax_t(u)
  avg_c = sum_t x alpha;  z = x alpha + noise;  std_c = sqrt(sum_t (z - mean z)^2 / (T - 1))
  coef_c = dstd_c / ((T - 1) std_c), 0 on a channel whose STORED deviation is exactly 0 (the kernel's convention: such a
           channel - all zero over time, no noise - passes no gradient through the deviation; autograd has 0 / 0 there)
  G = davg_c + coef_c (z - mean z);  dalpha_t = sum_c G x;  dw_t = alpha_t (dalpha_t - <alpha, dalpha>) (1 - u_t^2)
  dx[c, t] = G alpha_t + dw_t a_c;  datt[c] = sum_t dw_t x[c, t]  (per utterance)

The backward takes what the kernel takes: the stored alpha and the stored deviation.  Forward scales (magnitudes of
the terms):

  m_t = sum_c |x a|: what the rounding of s_t is proportional to; it reaches u_t through 1 - u_t^2
  alpha_scale[t] = alpha_t (1 + e_t + sum_t' alpha_t' e_t'), e_t = (1 - u_t^2) m_t + |u_t|
  avg_scale = sum_t |x| alpha;  std_scale = sqrt(sum_t (|x alpha| + |noise| + |mean z|)^2 / (T - 1))

Backward bounds.  The two terms of dx are bounded separately, element by element (tol = BWD_TOL, u32 = 2^-24):

  Gm = |davg| + |coef| (|x alpha| + |noise| + |mean z|): the terms of G.  G alpha_t is held to tol Gm alpha_t.
  dw_t is a product of three factors, each with its own error:
    dalpha_t - <alpha, dalpha>: tol (sum_c Gm |x| + <alpha, sum_c Gm |x|>), the terms of the two sums;
    1 - u_t^2: E_t = 2 |u| (1 - u^2) n u32 m_t + 9 u32 (1 + u^2) - the part propagated from s_t (a lane's fmaf chain
      of ceil(C / 64) terms and the 6-level wave sum: n = ceil(C / 64) + 8) and the fp32 roundings that form it
      (tanhf to 2 ulp, the square, the subtraction).  NOT tol (1 + u^2): on a saturated frame 1 - u^2 is exactly 0 in
      fp32 and in fp64, and then so is the first error - the terms of dalpha, however large, do not reach dx.
    dw_bound_t = alpha_t (tol (dalpha's terms) (1 - u^2 + E_t) + |dalpha_t - <alpha, dalpha>| E_t) + tol |dw_t|
  dx_bound[b, c, t] = tol Gm alpha_t + dw_bound_t |a_c|;   datt_bound[b, c] = sum_t dw_bound_t |x| + tol sum_t |dw_t x|
  Where every frame of an utterance is saturated (dw == 0, which the GPU test reads off datt == 0 on channels with
  x > 0), dx is held to ``g_bound`` = tol Gm alpha_t alone.

Residue.  A constant channel under uniform weights without noise has a deviation that is rounding residue (~1e-9); coef
is then ~1 / residue, G on THAT row is residue / residue in fp32 and ~0 in fp64, and Gm says so: the bound of that row
is far above any value it can hold, so the row is only required to be finite.  The same holds, less extremely, for a
constant channel with noise: its deviation is the noise's (1e-5) on a level of CONST / T.  That row's Gm also enters
the terms of dalpha of its utterance, but those reach dx and datt only through 1 - u^2, which is exactly 0 whenever the
weights are uniform - so no other row's bound feels it.  tests/test_pool_edges_cpu.py shows what the bounds still
catch: a backward that returns dx = 0, or that drops the deviation path, misses them by a factor above 100 on every
case - on the dead channels with noise (coef ~ 1e5 / (T - 1)) as on the live ones."""
import numpy as np
import torch

from oracle.filler import synth_feat

from ecapa_rows_oracle import BWD_TOL, FWD_TOL, rel_to_scale  # noqa: F401  (the GPU and CPU tests take them from here)

U32 = 2.0 ** -24
NCLASS = 5   # c % 5: dead (all zero) | a positive constant | 1e3 |r| | 1e-4 |r| | |r|
CONST = 2.5
CASES = [(2, 72, 2), (2, 72, 33), (1, 5, 7), (2, 256, 150)]  # (2, 256, 150): the variant that reads the map in place


def f64(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def _n(shape, seed, scale=1.0):
    return synth_feat(tuple(shape), seed, scale=scale).numpy().astype(np.float32)


def inputs(shape, with_noise, saturated):
    """x of the five channel classes, the attention vector (scale 0.1, or positive and large enough that the constant
    channels alone put every frame's <x, a> above 20), the noise (1e-5 of unit deviation, the reference's, or None) and
    the gradient of the (B, 2C) output."""
    B, C, T = shape
    s = 9000 + 10 * CASES.index(tuple(shape))
    r = np.abs(_n(shape, s).astype(np.float64))
    x = np.zeros(shape)
    for c in range(C):
        k = c % NCLASS
        if k == 1:
            x[:, c] = CONST
        elif k == 2:
            x[:, c] = 1e3 * r[:, c]
        elif k == 3:
            x[:, c] = 1e-4 * r[:, c]
        elif k == 4:
            x[:, c] = r[:, c]
    att = _n((C,), s + 1)
    att = 10.0 * (1.0 + np.abs(att)) if saturated else 0.1 * att
    return {"x": x.astype(np.float32), "att": att.astype(np.float32),
            "noise": 1e-5 * _n((B, T, C), s + 2) if with_noise else None, "dout": _n((B, 2 * C), s + 3)}


def _parts(x, att, noise, alpha=None):
    x, att = f64(x), f64(att).reshape(-1)
    s = np.einsum("bct,c->bt", x, att)
    m = np.einsum("bct,c->bt", np.abs(x), np.abs(att))
    u = np.tanh(s)
    if alpha is None:
        e = np.exp(u - u.max(-1, keepdims=True))
        alpha = e / e.sum(-1, keepdims=True)
    alpha = f64(alpha)
    wx = x * alpha[:, None, :]
    nz = np.zeros_like(x) if noise is None else np.transpose(f64(noise), (0, 2, 1))
    z = wx + nz
    zm = z.mean(-1, keepdims=True)
    zmag = np.abs(wx) + np.abs(nz) + np.abs(zm)
    return x, att, s, m, u, alpha, wx, z, zm, zmag


def fwd(x, att, noise=None, alpha=None):
    """alpha: None computes the weights; the stored weights evaluate the pooled statistics AT them."""
    x, att, s, m, u, alpha, wx, z, zm, zmag = _parts(x, att, noise, alpha)
    T = x.shape[-1]
    e = (1.0 - u * u) * m + np.abs(u)
    d = z - zm
    return {"s": s, "m": m, "alpha": alpha, "alpha_scale": alpha * (1.0 + e + (alpha * e).sum(-1, keepdims=True)),
            "avg": wx.sum(-1), "avg_scale": np.abs(wx).sum(-1),
            "std": np.sqrt((d * d).sum(-1) / (T - 1)), "std_scale": np.sqrt((zmag * zmag).sum(-1) / (T - 1))}


def bwd(x, att, noise, alpha, sd, dout, tol=BWD_TOL):
    """The backward at the stored weights ``alpha`` (B, T) and the stored deviations ``sd`` (B, C), with the bounds of
    the module docstring.  sd = zeros drops the deviation path (the guard's convention on every channel)."""
    x, att, s, m, u, alpha, wx, z, zm, zmag = _parts(x, att, noise, alpha)
    B, C, T = x.shape
    sd, dout = f64(sd), f64(dout)
    davg, dstd = dout[:, :C], dout[:, C:]
    with np.errstate(divide="ignore", invalid="ignore"):
        coef = np.where(sd > 0, dstd / ((T - 1) * sd), 0.0)
    G = davg[:, :, None] + coef[:, :, None] * (z - zm)
    Gm = np.abs(davg)[:, :, None] + np.abs(coef)[:, :, None] * zmag
    dal = (G * x).sum(1)
    dalm = (Gm * np.abs(x)).sum(1)
    dot = (alpha * dal).sum(-1, keepdims=True)
    dotm = (alpha * dalm).sum(-1, keepdims=True)
    q = 1.0 - u * u
    dw = alpha * (dal - dot) * q
    n = -(-C // 64) + 8
    E = 2.0 * np.abs(u) * q * n * U32 * m + 9.0 * U32 * (1.0 + u * u)
    dw_bound = alpha * (tol * (dalm + dotm) * (q + E) + np.abs(dal - dot) * E) + tol * np.abs(dw)
    a = att[None, :, None]
    g_alpha = G * alpha[:, None, :]
    g_bound = tol * Gm * alpha[:, None, :]
    return {"coef": coef, "dw": dw, "dw_bound": dw_bound, "g_alpha": g_alpha, "g_bound": g_bound,
            "dx": g_alpha + dw[:, None, :] * a, "dx_bound": g_bound + dw_bound[:, None, :] * np.abs(a),
            "mean_path": davg[:, :, None] * alpha[:, None, :] + dw[:, None, :] * a,
            "datt": (dw[:, None, :] * x).sum(-1),
            "datt_bound": (dw_bound[:, None, :] * np.abs(x)).sum(-1) + tol * np.abs(dw[:, None, :] * x).sum(-1), "saturated": bool((q == 0).all())}


def elementwise(got, want, scale):
    """max of |got - want| / scale over a tensor whose every element has its own scale (an exact element counts 0)."""
    got, want, scale = f64(got), f64(want), f64(scale)
    assert got.shape == want.shape == scale.shape, (got.shape, want.shape, scale.shape)
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / scale)
    return float(r.max())


def by_class(got, want, scale, C):
    """rel_to_scale per channel class: got / want (B, C, ...) with scale (B, C)."""
    return [rel_to_scale(f64(got)[:, k::NCLASS], f64(want)[:, k::NCLASS], f64(scale)[:, k::NCLASS]) if k < C else float("nan")
            for k in range(NCLASS)]


def bound_ratio_by_class(got, want, bound):
    """max of |got - want| / bound per channel class, every element on its own bound; got / want / bound (B, C, ...)."""
    got, want, bound = f64(got), f64(want), f64(bound)
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    r = np.where(np.isfinite(got), r, np.inf)
    C = got.shape[1]
    return [float(r[:, k::NCLASS].max()) if k < C else float("nan") for k in range(NCLASS)]
