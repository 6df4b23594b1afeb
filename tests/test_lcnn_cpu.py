"""CPU: the LCNN surface (model.py:511-610) - state_dict, seeded construction, the fp64 restatement against the
reference golden, the input-width guard and the C-ABI symbols of its kernels."""
import os
import re

import numpy as np
import pytest
import torch

import lcnn_oracle as o
from oracle.filler import fill_module_, fill_value, synth_feat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("air_lcnn_conv1_fwd", "air_lcnn_conv1_wgrad", "air_lcnn_conv1_wgrad_ws_bytes", "air_mfm_pool_fwd",
               "air_mfm_pool_bwd", "air_mfm_bias_grad", "air_mfm_bias_grad_ws_bytes", "air_copy_pad", "air_mul",
               "air_dropout_mask_ctr")


def test_state_dict_surface(golden):
    from asvspoof2021_air_amd.lcnn import LCNN
    g = golden("lcnn.npz")
    sd = LCNN(60, 256).state_dict()
    assert list(sd.keys()) == list(g["names"])
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == list(g["shapes"])
    assert "conv2.2.running_mean" in sd and "conv2.2.weight" not in sd and "conv3.3.running_var" in sd


def test_seeded_construction_draws_the_reference_numbers(golden):
    from asvspoof2021_air_amd.lcnn import LCNN
    g = golden("lcnn.npz")
    B, T, sx, sm = g["cfg"]
    torch.manual_seed(1203)
    net = LCNN(60, 256)
    sums = [float(p.detach().double().sum()) for _, p in net.named_parameters()]
    abss = [float(p.detach().double().abs().sum()) for _, p in net.named_parameters()]
    np.testing.assert_array_equal(sums, g["init_sum"])
    np.testing.assert_array_equal(abss, g["init_abs"])


def _filled_params():
    from asvspoof2021_air_amd.lcnn import LCNN
    net = fill_module_(LCNN(60, 256))
    return net, {k: v.detach().double() for k, v in net.state_dict().items()}


def test_restatement_vs_golden_forward_backward(golden):
    g = golden("lcnn.npz")
    B, T, sx, sm = (int(v) for v in g["cfg"])
    net, sd = _filled_params()
    x = synth_feat((B, 1, 60, T), seed=sx).double()
    params = {k: sd[k].clone().requires_grad_(True) for k, _ in net.named_parameters()}
    bufs = {k: v.clone() for k, v in sd.items() if "running" in k}
    with torch.no_grad():
        fe, oe, _ = o.forward(params, x, False, buffers=bufs)
    np.testing.assert_allclose(fe.numpy(), g["feat_eval"], rtol=1e-4, atol=1e-4 * np.abs(g["feat_eval"]).max())
    np.testing.assert_allclose(oe.numpy(), g["out_eval"], rtol=1e-4, atol=1e-4 * np.abs(g["out_eval"]).max())
    keep = torch.from_numpy(g["keep"])
    ft, ot, _ = o.forward(params, x, True, keep=keep, buffers=bufs)
    loss, neg = o.ocsoftmax(ft, fill_value("center", (1, 256)).double(), torch.from_numpy(g["labels"]))
    loss.backward()
    np.testing.assert_allclose(ft.detach().numpy(), g["feat_train"], rtol=1e-4,
                               atol=1e-4 * np.abs(g["feat_train"]).max())
    np.testing.assert_allclose(loss.item(), float(g["loss"]), rtol=1e-5)
    np.testing.assert_allclose(neg.detach().numpy(), g["neg"], atol=1e-5)
    gn = np.array([float(params[k].grad.norm()) if params[k].grad is not None else 0.0 for k in params])
    np.testing.assert_allclose(gn, g["grad_norm"], rtol=1e-4, atol=1e-12)
    assert gn[-2] == 0.0 and gn[-1] == 0.0  # fc_mu: no gradient under the OC-Softmax loss
    for k, v in bufs.items():
        np.testing.assert_allclose(v.numpy(), g["after/" + k], rtol=1e-5, atol=1e-6)


def test_route_select_equals_max_decisions():
    """The route bytes encode exactly the values torch's max(dim) / max_pool2d pick, ties included."""
    torch.manual_seed(5)
    pre = torch.randint(-3, 3, (2, 8, 7, 9)).double()  # many ties
    for pool in (False, True):
        r = o.routes_of(pre, pool)
        want = o.mfm(pre)
        if pool:
            want = torch.nn.functional.max_pool2d(want, 2, 2)
        assert torch.equal(o.route_select(pre, r, pool), want)
    # the gradient goes where torch sends it on ties (first candidate)
    a = pre.clone().requires_grad_(True)
    torch.nn.functional.max_pool2d(o.mfm(a), 2, 2).sum().backward()
    b = pre.clone().requires_grad_(True)
    o.route_select(b, o.routes_of(pre, True), True).sum().backward()
    assert torch.equal(a.grad, b.grad)


def test_width_guard():
    from asvspoof2021_air_amd.lcnn import LCNN
    net = LCNN(60, 256)
    with pytest.raises(ValueError, match="needs T // 16 = 46"):
        net.check_input(torch.zeros(2, 1, 60, 401))
    net.check_input(torch.zeros(2, 1, 60, 750))
    from asvspoof2021_air_amd import _hip
    with pytest.raises(_hip.AirError):  # CPU tensors: no fallback
        net(torch.zeros(2, 1, 60, 750))


def test_new_symbols_declared_and_exported():
    from asvspoof2021_air_amd import _hip, build
    build.build(verbose=False)
    text = open(os.path.join(ROOT, "include", "air_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(air_[a-z0-9_]+)\s*\(", text))
    lib = _hip.lib()
    for n in NEW_SYMBOLS:
        assert n in declared, n
        assert hasattr(lib, n), n
    assert int(lib.air_lcnn_conv1_wgrad_ws_bytes()) > 0

