"""fp64 numpy restatements of the fp32 BatchNorm of csrc/norm_act.hip (statistics, apply, backward), the inputs that
tests/test_bn_edges_cpu.py and tests/test_bn_edges_gpu.py share, and the error bounds the kernels are held to.

Everything is per channel.  Next to each result ``k`` a function returns ``k_scale``, built from the magnitudes of the
terms that form ``k``; the bounds below are multiples of those scales, so a channel of small scale cannot hide behind
a channel of large scale.

Inputs.  Channel c of an input belongs to class c % 8 (r = a seeded tensor of about unit deviation):

  0  r                                   benign control
  1  1000 + 0.1 r                        mean / std = 1e4
  2  -1e4 + r                            negative large mean
  3  the constant 3.25                   variance exactly 0
  4  r, first element of the channel 100 the shift K is an outlier: (mean - K) / std ~ 100
  5  1e-6 r                              variance << eps
  6  1e6 r                               squares ~ 1e12
  7  +1, -1 alternating over the plane   exact sums

The shift.  The kernels sum x - K (K = the channel's first element for the pass over x, the first non-empty record's K
for the records a convolution epilogue wrote) and form var = E[(x-K)^2] - E[x-K]^2.  The rounding of that is
proportional to ``var_scale = E[(x-K)^2] + (mean-K)^2``, which is ~2 var when K is a typical element and grows with
(mean-K)^2 when it is not: on class 4 the kernel-order emulation (tests/test_bn_edges_cpu.py) is off by 1.7e-5 of the
variance at (4, 16, 18, 75) (K = 100 against data of unit deviation; 3.3e-6 or less at the other shapes), 0.0034 of
its bound - the documented cost of an outlier shift; the bound grows with the scale by construction.

Bounds, from the summation structure (u = 2^-24, c(S) = ceil(S / 1024) + 4: the longest fp32 chain of a lane per image -
256 lanes x 4 elements - plus the quad tree and the final operations; images and lanes are folded in fp64):

  variance         2 c(S) u var_scale
  mean             u |mean| + 2 c(S) u mean_scale,  mean_scale = mean |x - K|
  invstd           0.5 invstd^3 var_bound + 2 u invstd
  running var      momentum N/(N-1) var_bound + 2 u (|(1-momentum) rv| + |momentum unbiased|); running mean likewise
  scale, shift     2 u |gamma invstd|, 2 u (|beta| + |mean scale|) against fp64 of the kernel's OWN mean and invstd
  apply            4 u y_scale, y_scale = |x scale| + |shift|, against fp64 x scale + shift of the kernel's own scale, shift
  dbeta, dgamma    2 c(S) u times sum |g|, sum |g xhat|
  dx               8 u dx_scale + |gamma| invstd (dbeta_bound + |xhat| dgamma_bound) / N

The backward's closed form is evaluated on the fp32 mean and invstd the kernel is given, so the kernel's own arithmetic
is isolated from the fp32 storage of the mean (which is also PyTorch's)."""
from fractions import Fraction

import numpy as np
import torch

from oracle.filler import synth_feat

U = 2.0 ** -24
EPS = 1e-5
MOMENTUM = 0.1
NCLASS = 8
SHAPES = [(3, 8, 5, 13),     # S = 65 is odd: the PEEL path
          (2, 8, 6, 11),     # S = 66: the two-element tail, S & 2
          (160, 8, 1, 12),   # more than 64 splits per channel: the ordered fold walks three chunks
          (1, 8, 1, 1),      # N = 1
          (4, 16, 18, 75)]   # the model's layer-1 map
MODEL_SHAPE = (4, 16, 18, 75)


def f64(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def chain(S):
    """c(S): the longest fp32 chain of a lane per image, the quad tree and the final operations."""
    return -(-S // 1024) + 4


def _n(shape, seed, scale=1.0):
    return synth_feat(tuple(shape), seed, scale=scale).numpy().astype(np.float32)


def _bcs(x):
    B, C = x.shape[0], x.shape[1]
    return B, C, int(np.prod(x.shape[2:], dtype=np.int64))


def classes(shape, seed):
    """float32 (B, C, *spatial) with channel c of class c % 8."""
    B, C = shape[0], shape[1]
    S = int(np.prod(shape[2:], dtype=np.int64))
    r = synth_feat((B, C, S), seed).double().numpy()
    x = np.empty((B, C, S), np.float64)
    alt = np.where(np.arange(S) % 2 == 0, 1.0, -1.0)
    for c in range(C):
        k = c % NCLASS
        if k == 0:
            x[:, c] = r[:, c]
        elif k == 1:
            x[:, c] = 1000.0 + 0.1 * r[:, c]
        elif k == 2:
            x[:, c] = -1e4 + r[:, c]
        elif k == 3:
            x[:, c] = 3.25
        elif k == 4:
            x[:, c] = r[:, c]
            x[0, c, 0] = 100.0
        elif k == 5:
            x[:, c] = 1e-6 * r[:, c]
        elif k == 6:
            x[:, c] = 1e6 * r[:, c]
        else:
            x[:, c] = alt[None, :]
    return x.astype(np.float32).reshape(shape)


def seed_of(shape):
    """Seeds chosen so that the elements whose ReLU mask the rounding can decide exist on classes 1 and 2 of the layer-1
    map and are at most 2 % of any channel (tests/test_bn_edges_cpu.py asserts both)."""
    return 7300 + 10 * SHAPES.index(tuple(shape))


def case(shape):
    """The inputs of one shape: x, the affine parameters, the running statistics, a gradient and an accumulate base."""
    C = shape[1]
    s = seed_of(shape)
    return {"x": classes(shape, s), "gamma": 1.0 + 0.3 * _n((C,), s + 1), "beta": 0.2 * _n((C,), s + 2),
            "rm": _n((C,), s + 3), "rv": np.abs(_n((C,), s + 4)) + np.float32(0.5), "dy": _n(shape, s + 5),
            "base": _n(shape, s + 6)}


def first_element(x):
    """The shift of the pass over x: the channel's first element (image 0, position 0)."""
    B, C, S = _bcs(x)
    return f64(x).reshape(B, C, S)[0, :, 0].copy()


def stats(x, gamma, beta, rm, rv, eps=EPS, momentum=MOMENTUM, K=None, keep=None):
    """Training-mode statistics per channel, their scales and their bounds (``*_bound``).  K: the shift the algorithm
    under test uses (see the module docstring); the results do not depend on it, the scales do.  keep: the weight of
    the old running statistics - the kernel's float32 ``1.0f - momentum`` unless given."""
    B, C, S = _bcs(x)
    N = B * S
    xc = np.moveaxis(f64(x).reshape(B, C, S), 1, 0).reshape(C, N)
    K = first_element(x) if K is None else f64(K)
    gamma, beta, rm, rv = f64(gamma), f64(beta), f64(rm), f64(rv)
    eps, momentum = float(np.float32(eps)), float(np.float32(momentum))
    mean = xc.mean(1)
    var = ((xc - mean[:, None]) ** 2).mean(1)
    d = xc - K[:, None]
    var_scale = (d * d).mean(1) + (mean - K) ** 2
    mean_scale = np.abs(d).mean(1)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    unb = N / (N - 1.0) if N > 1 else 1.0
    keep = float(np.float32(1.0) - np.float32(momentum)) if keep is None else keep
    c = chain(S)
    var_bound = 2 * c * U * var_scale
    mean_bound = U * np.abs(mean) + 2 * c * U * mean_scale
    return {"N": N, "K": K, "mean": mean, "mean_scale": mean_scale, "mean_bound": mean_bound,
            "var": var, "var_scale": var_scale, "var_bound": var_bound,
            "invstd": invstd, "invstd_bound": 0.5 * invstd ** 3 * var_bound + 2 * U * invstd,
            "scale": scale, "shift": shift,
            "running_mean": keep * rm + momentum * mean,
            "running_mean_bound": momentum * mean_bound + 2 * U * (np.abs(keep * rm) + np.abs(momentum * mean)),
            "running_var": keep * rv + momentum * var * unb,
            "running_var_bound": momentum * unb * var_bound + 2 * U * (np.abs(keep * rv) + np.abs(momentum * var * unb))}


def coeffs(mean, invstd, gamma, beta):
    """scale and shift in fp64 of the given (the kernel's own, fp32) mean and invstd, and their bounds."""
    mean, invstd, gamma, beta = f64(mean), f64(invstd), f64(gamma), f64(beta)
    scale = gamma * invstd
    return {"scale": scale, "scale_bound": 2 * U * np.abs(scale),
            "shift": beta - mean * scale, "shift_bound": 2 * U * (np.abs(beta) + np.abs(mean * scale))}


def eval_coeffs(gamma, beta, rm, rv, eps=EPS):
    """Evaluation-mode scale and shift from the running statistics.  The kernel forms rv + eps, its root, the
    reciprocal and two products in fp32: 4 u on the scale, and 2 u on the terms of the shift on top of the scale's."""
    gamma, beta, rm, rv = f64(gamma), f64(beta), f64(rm), f64(rv)
    scale = gamma / np.sqrt(rv + float(np.float32(eps)))
    return {"scale": scale, "scale_bound": 4 * U * np.abs(scale),
            "shift": beta - rm * scale, "shift_bound": 2 * U * np.abs(beta) + 6 * U * np.abs(rm * scale)}


def _per_channel(v, x):
    shp = [1] * x.ndim
    shp[1] = -1
    return f64(v).reshape(shp)


def apply(x, scale, shift, relu):
    """y = x scale + shift (max with 0 under relu); y_scale = |x scale| + |shift|; y_bound = 4 u y_scale."""
    x = f64(x)
    sc, sh = _per_channel(scale, x), _per_channel(shift, x)
    y = x * sc + sh
    ys = np.abs(x * sc) + np.abs(sh)
    return {"y": np.maximum(y, 0.0) if relu else y, "pre": y, "y_scale": ys, "y_bound": 4 * U * ys}


def bwd(x, g, mean, invstd, gamma, beta, mask=None, base=None):
    """The closed form of the kernel's header on the GIVEN mean and invstd:
    xhat = (x - mean) invstd, dbeta = sum g, dgamma = sum g xhat, dx = gamma invstd (g - dbeta/N - xhat dgamma/N)
    [+ base], with g zeroed where ``mask`` is false.  beta takes no part (it only enters the kernel's mask)."""
    B, C, S = _bcs(x)
    N = B * S
    x, g = f64(x), f64(g)
    if mask is not None:
        g = np.where(np.asarray(mask, bool), g, 0.0)
    mu, is_, ga = _per_channel(mean, x), _per_channel(invstd, x), _per_channel(gamma, x)
    ax = tuple(i for i in range(x.ndim) if i != 1)
    xhat = (x - mu) * is_
    dbeta = g.sum(ax)
    dgamma = (g * xhat).sum(ax)
    dbeta_scale = np.abs(g).sum(ax)
    dgamma_scale = np.abs(g * xhat).sum(ax)
    c = chain(S)
    dbeta_bound, dgamma_bound = 2 * c * U * dbeta_scale, 2 * c * U * dgamma_scale
    db, dg = _per_channel(dbeta, x), _per_channel(dgamma, x)
    dx = ga * is_ * (g - db / N - xhat * dg / N)
    dx_scale = np.abs(ga) * is_ * (np.abs(g) + np.abs(db) / N + np.abs(xhat) * np.abs(dg) / N)
    if base is not None:
        dx = dx + f64(base)
        dx_scale = dx_scale + np.abs(f64(base))
    dx_bound = 8 * U * dx_scale + np.abs(ga) * is_ * (_per_channel(dbeta_bound, x) + np.abs(xhat) * _per_channel(dgamma_bound, x)) / N
    return {"dbeta": dbeta, "dbeta_scale": dbeta_scale, "dbeta_bound": dbeta_bound,
            "dgamma": dgamma, "dgamma_scale": dgamma_scale, "dgamma_bound": dgamma_bound,
            "dx": dx, "dx_scale": dx_scale, "dx_bound": dx_bound, "xhat": xhat}


def exact_alternating(shape):
    """Class 7 in exact arithmetic: (mean, biased variance, unbiased variance) of +1, -1 alternating over each plane."""
    B = shape[0]
    S = int(np.prod(shape[2:], dtype=np.int64))
    N = B * S
    mean = Fraction(B * (S % 2), N)
    var = 1 - mean * mean
    return float(mean), float(var), float(var * N / (N - 1)) if N > 1 else float(var)


def invstd_of_zero_variance(eps=EPS):
    return np.float32(1.0 / np.sqrt(np.float64(np.float32(eps))))


def ratios(got, want, bound, axis=1):
    """max over each channel of |got - want| / bound (an exact element counts 0 whatever its bound), folded to the
    eight classes: a list of NCLASS floats (nan for a class the tensor has no channel of)."""
    got, want, bound = f64(got), f64(want), f64(bound)
    assert got.shape == want.shape, (got.shape, want.shape)
    bound = np.broadcast_to(bound, want.shape)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    r = np.where(np.isfinite(got), r, np.inf)
    if r.ndim > 1:
        r = np.moveaxis(r, axis, 0).reshape(r.shape[axis], -1).max(1)
    out = [float("nan")] * NCLASS
    for c in range(r.shape[0]):
        k = c % NCLASS
        out[k] = float(r[c]) if out[k] != out[k] else max(out[k], float(r[c]))
    return out


def fmt(what, rs):
    return "%-44s " % what + " ".join("%d:%-8.3g" % (k, v) for k, v in enumerate(rs)) + "  (max error / bound per class)"


def worst(rs):
    v = [r for r in rs if r == r]
    return max(v) if v else 0.0


# ---- inputs of the convolution-epilogue tests -----------------------------------------------------------------
CONV_STATS = [(3, 64, 4, 33, 128), (2, 64, 18, 75, 64)]    # (B, Cin, H, W, Cout): the classes ride on the residual
CONV_DGRAD = [(3, 128, 4, 33, 64), (2, 64, 18, 75, 64)]    # (B, Cout, H, W, Cin): the classes are the BatchNorm's input


def conv_stats_case(cfg):
    B, Cin, H, W, Cout = cfg
    s = 7100 + 10 * CONV_STATS.index(tuple(cfg))
    return {"x": _n((B, Cin, H, W), s), "w": _n((Cout, Cin, 3, 3), s + 1, 0.1), "res": classes((B, Cout, H, W), s + 2),
            "gamma": 1.0 + 0.3 * _n((Cout,), s + 3), "beta": 0.2 * _n((Cout,), s + 4), "rm": _n((Cout,), s + 5),
            "rv": np.abs(_n((Cout,), s + 6)) + np.float32(0.5)}


def conv_dgrad_case(cfg):
    B, Cout, H, W, Cin = cfg
    s = 7200 + 10 * CONV_DGRAD.index(tuple(cfg))
    return {"w": _n((Cout, Cin, 3, 3), s, 0.1), "dy": _n((B, Cout, H, W), s + 1), "x": classes((B, Cin, H, W), s + 2),
            "gamma": 1.0 + 0.3 * _n((Cin,), s + 3), "beta": 0.2 * _n((Cin,), s + 4)}


def record_shift(rec, C):
    """The shift of the records route: K of each channel's first non-empty record.  ``rec``: the float32 view of the
    buffer conv2d_fwd(..., stats=True) returned - a header {G, C, 0, 0}, then G records {n, K, s1, s2} per channel."""
    rec = np.asarray(rec, np.float32)
    G, Ch = int(rec[:2].view(np.int32)[0]), int(rec[:2].view(np.int32)[1])
    assert Ch == C, (Ch, C)
    r = rec[4:4 + 4 * C * G].reshape(C, G, 4)
    K = np.zeros(C)
    for c in range(C):
        live = np.nonzero(r[c, :, 0] > 0)[0]
        assert live.size, "channel %d has no record" % c
        K[c] = r[c, live[0], 1]
    return K
