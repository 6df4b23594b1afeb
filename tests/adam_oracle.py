"""Test infrastructure (numpy / PyTorch-CPU): the fp64 reference of air_adam_step, the elementwise bounds the GPU tests
hold the kernel to, the inputs they use, and the fp32 CPU restatement those bounds are checked against
(test_small_kernels_cpu.py) - never the kernel."""
import numpy as np
import torch

from oracle import train as o_train
from oracle.filler import synth_feat

EPS32 = 2.0 ** -24  # unit roundoff of float32
ADAM_DEFAULT = dict(lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=5e-4, grad_scale=1.0)
BIG_N = 4096 * 256 * 4 + 4 * 256 * 3 + 3  # second grid-stride trip (blocks are capped at 4096) + ragged tail
ADAM_N = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 100003, BIG_N]
ADAM_POINTS = [dict(weight_decay=0.0), dict(weight_decay=1e-2), dict(grad_scale=0.5), dict(grad_scale=0.125),
               dict(beta1=0.8, beta2=0.99), dict(eps=1e-3), dict(lr=1e-2)]
ADAM_POINT_N = 4 * 256 * 3 + 3  # several blocks and a three-element tail
ADAM_STEPS = [1, 2, 1000, 100000]  # single steps from non-zero moments

# Elementwise bounds from fp32 rounding of the kernel's formula (u = 2^-24), with p', m', v' the fp64 results and
# S = |g grad_scale| + |wd p|:
#   |dp| <= ADAM_CP u (|p'| + 16 |lr_bc1 m' / denom'|)
#   |dm| <= ADAM_CM u (|beta1 m| + (1 - beta1) S)
#   |dv| <= ADAM_CV u (beta2 v + (1 - beta2) S^2)
# S stands where one would first write |g_eff|, g_eff = g grad_scale + wd p: the fp32 sum carries an error of u S
# whatever it comes to, and among 4 million N(0, 1) gradients some cancel against wd p to 1 % of their terms (with
# |g_eff| in the bounds the fp32 CPU restatement itself misses them 103-fold in m and 206-fold in v).  Where nothing
# cancels S = |g_eff| and the bounds are the plain ones.
# The constants are NOT measured on the kernel: test_small_kernels_cpu.py holds the fp32 CPU restatement
# (oracle.train.adam_step_ on float32 tensors) to them on exactly these inputs.  With ADAM_CP = 2 the restatement
# misses the p bound at a few of the 4 197 379 elements of BIG_N, by a factor 1.32: there beta1 m and
# (1 - beta1) g_eff cancel to a small m', so the update's error is large against the update itself.  Hence
# ADAM_CP = 4, the smallest power of two that admits it.  Largest fractions of the bounds the restatement then uses
# over every case: p 0.66, m 0.26, v 0.54.
ADAM_CP, ADAM_CM, ADAM_CV = 4.0, 8.0, 8.0


def f32(x):
    return float(np.float32(x))


def adam_ref64(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, grad_scale):
    """One Adam step (coupled L2 decay, g <- g grad_scale + wd p) in float64 on float32 inputs.  The hyper-parameters
    are the float32 values the C entry point receives.  Returns p', m', v' and the three elementwise bounds."""
    p, g, m, v = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps, wd, gs = (f32(a) for a in (lr, beta1, beta2, eps, weight_decay, grad_scale))
    ge = g * gs + wd * p
    S = np.abs(g * gs) + np.abs(wd * p)
    m1 = b1 * m + (1.0 - b1) * ge
    v1 = b2 * v + (1.0 - b2) * ge * ge
    denom = np.sqrt(v1) / np.sqrt(1.0 - b2 ** step) + eps
    upd = lr / (1.0 - b1 ** step) * m1 / denom
    p1 = p - upd
    tol = (ADAM_CP * EPS32 * (np.abs(p1) + 16.0 * np.abs(upd)),
           ADAM_CM * EPS32 * (np.abs(b1 * m) + (1.0 - b1) * S),
           ADAM_CV * EPS32 * (b2 * v + (1.0 - b2) * S * S))
    return (p1, m1, v1), tol


def adam_restated32(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, grad_scale):
    """oracle.train.adam_step_ in float32 on the same inputs (gradient pre-scaled: g <- g grad_scale)."""
    p, g, m, v = (torch.from_numpy(np.array(a, dtype=np.float32)) for a in (p, g, m, v))
    o_train.adam_step_(p, g * f32(grad_scale), m, v, step, f32(lr), f32(beta1), f32(beta2), f32(eps), f32(weight_decay))
    return p.numpy(), m.numpy(), v.numpy()


def adam_inputs(n, k, moments=False):
    """Parameters, the N(0, k^2) gradient of step ``k`` and (optionally non-zero) moments: float32 numpy arrays."""
    p = synth_feat((n,), 1).numpy()
    g = synth_feat((n,), 10 + k, scale=float(k)).numpy()
    if moments:
        return p, g, synth_feat((n,), 3, scale=0.1).numpy(), (synth_feat((n,), 4, scale=0.1) ** 2).numpy()
    return p, g, np.zeros(n, np.float32), np.zeros(n, np.float32)


def adam_cases():
    """(n, hyper-parameters, steps, non-zero moments) of every Adam case of the GPU tests."""
    cases = [(n, ADAM_DEFAULT, (1, 2, 3), False) for n in ADAM_N]
    cases += [(ADAM_POINT_N, dict(ADAM_DEFAULT, **pt), (1, 2, 3), False) for pt in ADAM_POINTS]
    return cases + [(ADAM_POINT_N, ADAM_DEFAULT, (s,), True) for s in ADAM_STEPS]


def used(got, want, tol):
    """Largest fraction of its bound that an array uses (0 / 0 counts as 0)."""
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0.0, 0.0, d / tol)
    return float(r.max()) if r.size else 0.0


def assert_adam(got, ref, tol, what):
    for name, a, r, t in zip("pmv", got, ref, tol):
        d = np.abs(a.astype(np.float64) - r)
        bad = np.flatnonzero(~(d <= t))
        assert bad.size == 0, "%s: %s[%d] = %r, fp64 %r: off by %.3g > %.3g (%d of %d elements out of bound)" % (
            what, name, bad[0], a[bad[0]], r[bad[0]], d[bad[0]], t[bad[0]], bad.size, a.size)
