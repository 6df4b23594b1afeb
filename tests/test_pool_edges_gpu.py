"""GPU: the attentive pooling kernels (selfatt_fwd_kernel / selfatt_bwd_kernel, csrc/pool_head.hip) against the fp64
oracle of tests/pool_edges_oracle.py on the inputs a post-ReLU map really has: dead channels (all zero over time), a
constant channel, channels at 1e3, 1e-4 and 1; with the reference's noise (1e-5) and without; attention weights at scale
0.1 and at a scale that saturates tanh on every frame; T = 2 (the smallest length with a deviation), channel counts
that are no multiple of 64, and the variant that reads the map in place.

* The stored weights define the pooled statistics and the backward, as in the kernels: avg, std, dx and datt are held
  at the kernel's own alpha, alpha itself element by element on the scale of its own terms.
* Bounds: FWD_TOL of tests/ecapa_rows_oracle.py times the oracle's term-magnitude scale per (b, c) for the outputs; for
  dx and datt the oracle's element-by-element bounds, which keep the two terms of dx apart (BWD_TOL on the terms of
  G alpha; for dw the fp32 roundings that form 1 - tanh^2, so that a saturated frame lets nothing through).
  tests/test_pool_edges_cpu.py asserts that dx = 0, a backward without the deviation path, and datt = 0 miss them.
  Printed per channel class (pytest -s)."""
import numpy as np
import pytest
import torch

import pool_edges_oracle as po
from pool_edges_oracle import FWD_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from asvspoof2021_air_amd import ops
    return ops


def G(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def N_(t):
    return t.detach().cpu().numpy()


def held(what, got, want, scale, tol, C):
    assert np.isfinite(got).all(), what + ": not finite"
    rs = po.by_class(got, want, scale, C)
    print("%-28s " % what + " ".join("%d:%-8.3g" % (k, r / tol) for k, r in enumerate(rs)) + "  (max error / bound per class)")
    assert max(r for r in rs if r == r) <= tol, "%s: error / bound per class %s" % (what, [r / tol for r in rs])


def bounded(what, got, want, bound):
    assert np.isfinite(got).all(), what + ": not finite"
    rs = po.bound_ratio_by_class(got, want, bound)
    print("%-28s " % what + " ".join("%d:%-8.3g" % (k, r) for k, r in enumerate(rs)) + "  (max error / bound per class)")
    assert max(r for r in rs if r == r) <= 1.0, "%s: error / bound per class %s" % (what, rs)


@pytest.mark.parametrize("saturated", [False, True])
@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("shape", po.CASES)
def test_selfatt_pool_edges(ops, shape, with_noise, saturated):
    B, C, T = shape
    d = po.inputs(shape, with_noise, saturated)
    x, att, noise, dout = G(d["x"]), G(d["att"]), G(d["noise"]), G(d["dout"])
    out, alpha = ops.selfatt_pool_fwd(x, att, noise)
    outn, alphan = N_(out), N_(alpha)
    assert np.isfinite(outn).all() and np.isfinite(alphan).all()
    f0 = po.fwd(d["x"], d["att"], d["noise"])
    r = po.elementwise(alphan, f0["alpha"], f0["alpha_scale"])
    print("%-28s %.3g  (max error / bound)" % ("alpha", r / FWD_TOL))
    assert r <= FWD_TOL
    if saturated:
        assert np.abs(f0["s"]).min() > 20.0
        assert (alphan == np.float32(1.0) / np.float32(T)).all(), "every frame saturated: the weights are uniform"
    f = po.fwd(d["x"], d["att"], d["noise"], alpha=alphan)
    held("avg", outn[:, :C], f["avg"], f["avg_scale"], FWD_TOL, C)
    held("std", outn[:, C:], f["std"], f["std_scale"], FWD_TOL, C)
    dead = outn[:, C::po.NCLASS]
    if with_noise:
        own = np.transpose(d["noise"].astype(np.float64), (0, 2, 1))[:, 0::po.NCLASS].std(-1, ddof=1)
        assert po.rel_to_scale(dead, own, f["std_scale"][:, 0::po.NCLASS]) <= FWD_TOL, "a dead channel's deviation is the noise's"
        assert (dead > 0).all()
    else:
        assert (dead == 0).all(), "a dead channel without noise has deviation 0 exactly"
        assert (outn[:, 0:C:po.NCLASS] == 0).all()

    dx, datt = ops.selfatt_pool_bwd(x, att, noise, alpha, out, dout)
    dxn, dattn = N_(dx), N_(datt)
    assert np.isfinite(dxn).all() and np.isfinite(dattn).all()
    b = po.bwd(d["x"], d["att"], d["noise"], alphan, outn[:, C:], d["dout"])
    bounded("datt", dattn, b["datt"], b["datt_bound"])
    if saturated:
        assert b["saturated"]
    if b["saturated"]:
        # every frame saturated: 1 - tanh^2 is exactly 0, in fp32 as in fp64 - datt says so (x > 0 on the live channels)
        # and dx is then held to its first term alone, G alpha, on that term's own bound
        assert (dattn == 0).all(), "1 - tanh^2 of a saturated frame is exactly 0"
        bounded("dx (= G alpha)", dxn, b["g_alpha"], b["g_bound"])
    else:
        bounded("dx", dxn, b["dx"], b["dx_bound"])
    if not with_noise:
        # the guard: no gradient through a deviation that is exactly 0 - dx is the mean-path term alone
        assert (b["coef"][:, 0::po.NCLASS] == 0).all()
        assert np.array_equal(b["dx"][:, 0::po.NCLASS], b["mean_path"][:, 0::po.NCLASS])
