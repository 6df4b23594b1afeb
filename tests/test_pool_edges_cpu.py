"""CPU: the oracle of the attentive pooling kernels (tests/pool_edges_oracle.py) against fp64 autograd of
oracle.resnet.self_attention_pool on the inputs of tests/test_pool_edges_gpu.py.

Autograd of the deviation of a channel that is all zero over time without noise is 0 / 0; the kernels (and the oracle)
pass no gradient through such a deviation.  Autograd is therefore asked for the gradient of the loss WITHOUT the
deviations that are exactly 0 - which is that convention - and must then be finite on every case."""
import numpy as np
import pytest
import torch

import pool_edges_oracle as po
from oracle import resnet as o_resnet


def T64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


@pytest.mark.parametrize("saturated", [False, True])
@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("shape", po.CASES)
def test_oracle_is_autograd(shape, with_noise, saturated):
    B, C, T = shape
    d = po.inputs(shape, with_noise, saturated)
    x = T64(d["x"]).requires_grad_(True)
    a = T64(d["att"]).reshape(1, C).requires_grad_(True)
    nz = None if d["noise"] is None else T64(d["noise"])
    out = o_resnet.self_attention_pool(x.permute(0, 2, 1), a, nz)
    avg, std = out[:, :C], out[:, C:]
    dout = T64(d["dout"])
    live = std.detach() > 0
    if with_noise:
        assert bool(live.all())
    else:
        assert not bool(live[:, 0::po.NCLASS].any()), "a dead channel without noise has deviation 0"
    loss = (avg * dout[:, :C]).sum() + (torch.where(live, std, torch.zeros_like(std)) * dout[:, C:]).sum()
    loss.backward()
    assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(a.grad).all())

    f = po.fwd(d["x"], d["att"], d["noise"])
    assert np.abs(f["s"]).min() > 20.0 if saturated else True
    assert po.rel_to_scale(f["avg"], avg.detach().numpy(), f["avg_scale"]) <= 1e-12
    assert po.rel_to_scale(f["std"], std.detach().numpy(), f["std_scale"]) <= 1e-12
    alpha = torch.softmax(torch.tanh((x.detach().permute(0, 2, 1) @ a.detach().reshape(-1, 1)).squeeze(2)), 1).numpy()
    assert po.elementwise(f["alpha"], alpha, f["alpha_scale"]) <= 1e-12
    b = po.bwd(d["x"], d["att"], d["noise"], f["alpha"], f["std"], d["dout"])
    assert np.isfinite(b["dx"]).all() and np.isfinite(b["datt"]).all()
    # fp64 against fp64: 1e-5 of what the fp32 kernel is allowed, element by element
    assert max(po.bound_ratio_by_class(b["dx"], x.grad.numpy(), b["dx_bound"])) <= 1e-5
    assert max(po.bound_ratio_by_class(b["datt"].sum(0)[None], a.grad.numpy(), b["datt_bound"].sum(0)[None])) <= 1e-5
    if not with_noise:
        assert (b["coef"][:, 0::po.NCLASS] == 0).all()
        assert np.array_equal(b["dx"][:, 0::po.NCLASS], b["mean_path"][:, 0::po.NCLASS])
    assert b["saturated"] or not saturated
    if b["saturated"]:
        assert (b["dw"] == 0).all() and np.array_equal(b["dx"], b["g_alpha"]), "1 - tanh^2 is 0 in fp64 as well (|s| > 20)"
    if saturated:
        assert np.array_equal(f["alpha"], np.full((B, T), 1.0 / T))


@pytest.mark.parametrize("saturated", [False, True])
@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("shape", po.CASES)
def test_a_wrong_backward_misses_the_bounds(shape, with_noise, saturated):
    """The bounds of the GPU test, applied to the oracle's own result after a mutation, at the float32 weights and
    deviations a kernel would store.  dx = 0 must miss the bound by more than 100 on every channel class but the
    constant one (whose row may be residue, see the oracle) - the dead class included; a backward without the deviation
    path (coef = 0) must miss it by more than 100 on every case, and on the dead channels whenever there is noise
    (coef ~ 1e5 / (T - 1)); datt = 0 must miss its bound on every live class unless every frame is saturated (then 0 is
    the answer)."""
    d = po.inputs(shape, with_noise, saturated)
    f = po.fwd(d["x"], d["att"], d["noise"])
    alpha, sd = f["alpha"].astype(np.float32), f["std"].astype(np.float32)
    b = po.bwd(d["x"], d["att"], d["noise"], alpha, sd, d["dout"])
    bound = b["g_bound"] if b["saturated"] else b["dx_bound"]
    zero = po.bound_ratio_by_class(np.zeros_like(b["dx"]), b["dx"], bound)
    nodev = po.bound_ratio_by_class(po.bwd(d["x"], d["att"], d["noise"], alpha, np.zeros_like(sd), d["dout"])["dx"], b["dx"], bound)
    nodatt = po.bound_ratio_by_class(np.zeros_like(b["datt"]), b["datt"], b["datt_bound"])
    print("dx = 0   / bound per class:", ["%.3g" % v for v in zero])
    print("coef = 0 / bound per class:", ["%.3g" % v for v in nodev])
    print("datt = 0 / bound per class:", ["%.3g" % v for v in nodatt])
    assert all(zero[k] > 100 for k in (0, 2, 3, 4)), zero
    assert max(nodev) > 100, nodev
    if with_noise:
        assert nodev[0] > 100, nodev
    if not b["saturated"]:
        assert all(nodatt[k] > 1 for k in (1, 2, 3, 4)), nodatt
