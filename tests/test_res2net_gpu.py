"""GPU: SE-Res2Net-50 (model.py:256-509) on its HIP kernels - the narrow-channel convolutions against fp64 at every
layer shape the model trains with at B = 64, 60 x 750 (channel slices included), the pool / Res2 / SE / log_softmax
kernels against torch, the model forward / gradients / running statistics against the fp64 restatement
(tests/res2net_oracle.py), Trainer steps with every head eager and hipGraph-replayed, scoring from a whole-module
pickle, and the ATen launches of a step."""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import res2net_oracle as o
from oracle.filler import fill_module_, fill_value, synth_feat, synth_pcm

from _budget import STRICT  # noqa: E402

pytestmark = pytest.mark.gpu

H0, W0, BIG = 60, 750, 64


def _model():
    from asvspoof2021_air_amd.res2net import Res2Net, SEBottle2neck
    return fill_module_(Res2Net(SEBottle2neck, [3, 4, 6, 3], baseWidth=26, scale=4, pretrained=False,
                                num_classes=2)).cuda()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def close(got, want, rtol, name):
    got, want = got.detach().double(), want.detach().double().to(got.device)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(want.abs().max().item(), 1e-30)
    err = (got - want).abs().max().item() / scale
    assert err <= rtol, "%s: max err %.3g of scale %.3g (rel %.3g > %.3g)" % (name, err * scale, scale, err, rtol)


@contextlib.contextmanager
def _aten_conv():
    with torch.backends.cudnn.flags(enabled=False):
        yield


def _act64(x, scale, shift):
    xa = x.double()
    if scale is not None:
        xa = F.relu(xa * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    return xa


# ------------------------------------------------------------------------------------------- layer shapes
def narrow_layers(B=BIG, H=H0, W=W0):
    """(Cin, Cout, k, stride, H, W, slice) of every convolution of the model that runs on the narrow kernels, at input
    (B, 1, H, W); slice: the input / output is a channel slice of a 4x wider tensor (the Res2 branches)."""
    from asvspoof2021_air_amd.res2net import _generic_1x1
    out = [(1, 16, 3, 1, H, W, False), (16, 16, 3, 1, H, W, False)]
    h, w_ = H, W
    for _, cin, planes, stride, width, _, ds in o.blocks():
        out.append((cin, 4 * width, 1, 1, h, w_, False))
        out.append((width, width, 3, stride, h, w_, True))
        ho, wo = (h - 1) // stride + 1, (w_ - 1) // stride + 1
        if not _generic_1x1(4 * width, 2 * planes):
            out.append((4 * width, 2 * planes, 1, 1, ho, wo, False))
        if ds is not None and not _generic_1x1(cin, 2 * planes):
            out.append((cin, 2 * planes, 1, 1, -(-h // ds), -(-w_ // ds), False))
        h, w_ = ho, wo
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


LAYER_SHAPES = narrow_layers()


@pytest.mark.parametrize("cin,cout,k,stride,H,W,sliced", LAYER_SHAPES,
                         ids=["%dx%d_k%d_s%d_%dx%d%s" % (s[:6] + ("_slice" if s[6] else "",)) for s in LAYER_SHAPES])
def test_narrow_conv_layer_vs_fp64(cin, cout, k, stride, H, W, sliced):
    from asvspoof2021_air_amd import ops
    B = BIG
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    wt = (synth_feat((cout, cin, k, k), 2) * (2.0 / (cin * k * k)) ** 0.5).cuda()
    prologue = cin == 16 and cout == 16  # the stem's BatchNorm + ReLU prologue
    sc = (1.0 + 0.3 * synth_feat((cin,), 3)).cuda() if prologue else None
    sh = (0.2 * synth_feat((cin,), 4)).cuda() if prologue else None
    if sliced:
        xw = synth_feat((B, 4 * cin, H, W), 1).cuda()
        x = xw[:, cin:2 * cin]
        yw = torch.full((B, 4 * cout, Ho, Wo), 7.0, device="cuda")
        y = ops.conv_narrow_fwd(x, wt, stride, out=yw[:, 2 * cout:3 * cout])
        assert torch.all(yw[:, :2 * cout] == 7.0) and torch.all(yw[:, 3 * cout:] == 7.0)
    else:
        x = synth_feat((B, cin, H, W), 1).cuda()
        y = ops.conv_narrow_fwd(x, wt, stride, in_scale=sc, in_shift=sh, relu=prologue)
    idx = [0, B - 1]
    with _aten_conv(), torch.no_grad():
        want = F.conv2d(_act64(x[idx], sc, sh), wt.double(), None, stride, pad)
    close(y[idx], want, STRICT["conv_rtol"], "forward")
    dy = synth_feat((B, cout, Ho, Wo), 6).cuda()
    if cin > 1:
        if sliced:
            dxw = torch.full((B, 4 * cin, H, W), 5.0, device="cuda")
            dx = ops.conv_narrow_dgrad(dy, wt, (B, cin, H, W), stride, out=dxw[:, cin:2 * cin])
            assert torch.all(dxw[:, :cin] == 5.0) and torch.all(dxw[:, 2 * cin:] == 5.0)
        else:
            dx = ops.conv_narrow_dgrad(dy, wt, (B, cin, H, W), stride)
        with _aten_conv():
            xd = torch.zeros((2, cin, H, W), dtype=torch.float64, device="cuda", requires_grad=True)
            F.conv2d(xd, wt.double(), None, stride, pad).backward(dy[idx].double())
        close(dx[idx], xd.grad, STRICT["conv_rtol"], "dgrad")
        acc = synth_feat((B, cin, H, W), 9).cuda()
        got = ops.conv_narrow_dgrad(dy, wt, (B, cin, H, W), stride, out=acc.clone(), accumulate=True)
        assert torch.equal(got, dx + acc)
    gw = ops.conv_narrow_wgrad(x, dy, wt.shape, stride, in_scale=sc, in_shift=sh, relu=prologue)
    with _aten_conv():
        wd = torch.zeros(tuple(wt.shape), dtype=torch.float64, device="cuda", requires_grad=True)
        F.conv2d(_act64(x, sc, sh), wd, None, stride, pad).backward(dy.double())
    close(gw, wd.grad, STRICT["conv_rtol"], "wgrad")
    assert torch.equal(gw, ops.conv_narrow_wgrad(x, dy, wt.shape, stride, in_scale=sc, in_shift=sh, relu=prologue))


@pytest.mark.parametrize("cin,cout,k,stride,H,W", [(6, 6, 3, 2, 7, 9), (13, 5, 3, 1, 5, 4), (33, 17, 1, 1, 3, 5),
                                                  (1, 3, 3, 2, 1, 1), (256, 256, 1, 1, 2, 3), (70, 40, 3, 2, 6, 11)])
def test_narrow_conv_ragged_edges(cin, cout, k, stride, H, W):
    from asvspoof2021_air_amd import ops
    B = 3
    pad = k // 2
    x = synth_feat((B, cin, H, W), 1).cuda()
    wt = synth_feat((cout, cin, k, k), 2).cuda()
    y = ops.conv_narrow_fwd(x, wt, stride)
    with _aten_conv():
        xd = x.double().requires_grad_(True)
        wd = wt.double().requires_grad_(True)
        want = F.conv2d(xd, wd, None, stride, pad)
        dy = synth_feat(tuple(want.shape), 6).cuda()
        want.backward(dy.double())
    close(y, want, STRICT["conv_rtol"], "forward")
    close(ops.conv_narrow_dgrad(dy, wt, x.shape, stride), xd.grad, STRICT["conv_rtol"], "dgrad")
    close(ops.conv_narrow_wgrad(x, dy, wt.shape, stride), wd.grad, STRICT["conv_rtol"], "wgrad")


# -------------------------------------------------------------------------------------- elementwise kernels
POOLS = [  # (B, C, H, W, k, stride, pad, ceil_mode, count_include_pad)
    (BIG, 6, 60, 750, 3, 1, 1, False, True), (BIG, 13, 60, 750, 3, 2, 1, False, True),
    (BIG, 26, 30, 375, 3, 2, 1, False, True), (BIG, 52, 15, 188, 3, 2, 1, False, True),
    (BIG, 32, 60, 750, 2, 2, 0, True, False), (BIG, 64, 30, 375, 2, 2, 0, True, False),
    (BIG, 128, 15, 188, 2, 2, 0, True, False), (2, 13, 60, 401, 3, 2, 1, False, True),
    (2, 32, 15, 201, 2, 2, 0, True, False), (3, 5, 1, 1, 3, 2, 1, False, True), (3, 5, 1, 3, 2, 2, 0, True, False)]


@pytest.mark.parametrize("B,C,H,W,k,s,p,ceil,cip", POOLS)
def test_avgpool_bit_exact(B, C, H, W, k, s, p, ceil, cip):
    from asvspoof2021_air_amd import ops
    xw = synth_feat((B, 4 * C, H, W), 21).cuda()
    x = xw[:, 3 * C:]
    want = F.avg_pool2d(x, k, s, p, ceil_mode=ceil, count_include_pad=cip)
    Ho, Wo = want.shape[2], want.shape[3]
    yw = torch.zeros((B, 4 * C, Ho, Wo), device="cuda")
    y = ops.avgpool2d_fwd(x, k, s, p, ceil, cip, out=yw[:, 3 * C:])
    assert torch.equal(y, want)
    dy = synth_feat(tuple(want.shape), 22).cuda()
    xt = x.detach().clone().requires_grad_(True)
    F.avg_pool2d(xt, k, s, p, ceil_mode=ceil, count_include_pad=cip).backward(dy)
    dxw = torch.zeros_like(xw)
    dx = ops.avgpool2d_bwd(dy, x.shape, k, s, p, ceil, cip, out=dxw[:, 3 * C:])
    assert torch.equal(dx, xt.grad)
    assert torch.count_nonzero(dxw[:, :3 * C]) == 0


@pytest.mark.parametrize("B,C,H,W", [(BIG, 6, 60, 750), (BIG, 13, 30, 375), (BIG, 26, 15, 188), (BIG, 52, 8, 94),
                                     (2, 13, 30, 201)])
def test_res2_relu_apply_bit_exact(B, C, H, W):
    from asvspoof2021_air_amd import ops
    x = synth_feat((B, C, H, W), 31).cuda()
    scale, shift = (1.0 + 0.3 * synth_feat((C,), 32)).cuda(), (0.2 * synth_feat((C,), 33)).cuda()
    addw = synth_feat((B, 4 * C, H, W), 34).cuda()
    cat = torch.zeros((B, 4 * C, H, W), device="cuda")
    y2 = torch.empty((B, C, H, W), device="cuda")
    ops.res2_bn_relu_apply(x, scale, shift, cat[:, C:2 * C], add=addw[:, 2 * C:3 * C], y2=y2)
    v = torch.relu(x * scale.view(1, C, 1, 1) + shift.view(1, C, 1, 1))
    assert torch.equal(cat[:, C:2 * C], v)
    assert torch.equal(y2, v + addw[:, 2 * C:3 * C])
    assert torch.count_nonzero(cat[:, :C]) == 0 and torch.count_nonzero(cat[:, 2 * C:]) == 0
    ops.res2_bn_relu_apply(x, scale, shift, cat[:, 3 * C:])
    assert torch.equal(cat[:, 3 * C:], v)


@pytest.mark.parametrize("B,C,H,W", [(BIG, 32, 60, 750), (BIG, 64, 30, 375), (BIG, 128, 15, 188), (BIG, 256, 8, 94),
                                     (2, 64, 30, 201)])
def test_se_tail_kernels(B, C, H, W):
    from asvspoof2021_air_amd import ops
    x = synth_feat((B, C, H, W), 41).cuda()
    z = (2.0 * synth_feat((B, C), 42)).cuda()
    r = synth_feat((B, C, H, W), 43).cuda()
    out = ops.se_relu_fwd(x, z, r)
    g = 1.0 / (1.0 + torch.exp(-z))
    assert torch.equal(out, torch.relu(x * g[:, :, None, None] + r))
    dout = synth_feat((B, C, H, W), 44).cuda()
    dx, dz, dres = ops.se_relu_bwd(x, z, out, dout)
    dpre = torch.where(out > 0, dout, torch.zeros_like(dout))
    assert torch.equal(dres, dpre)
    assert torch.equal(dx, dpre * g[:, :, None, None])
    gd = g.double()
    want = (dpre.double() * x.double()).sum((2, 3)) * gd * (1 - gd)
    close(dz, want, 1e-5, "dz")
    assert torch.equal(dz, ops.se_relu_bwd(x, z, out, dout)[1])


@pytest.mark.parametrize("B,C", [(1, 2), (64, 2), (4096, 2), (7, 5)])
def test_log_softmax_kernels(B, C):
    from asvspoof2021_air_amd import ops
    zz = (3.0 * synth_feat((B, C), 51)).cuda()
    out = ops.log_softmax_fwd(zz)
    zd = zz.double().requires_grad_(True)
    want = F.log_softmax(zd, dim=-1)
    close(out, want, 1e-6, "log_softmax")
    dout = synth_feat((B, C), 52).cuda()
    want.backward(dout.double())
    close(ops.log_softmax_bwd(out, dout), zd.grad, 1e-5, "log_softmax backward")


# ------------------------------------------------------------------------------------------------ the model
def _fp64_params(model):
    return {k: v.detach().double().requires_grad_(True) for k, v in model.named_parameters()}


def _buffers64(model):
    return {k: v.detach().double().clone() for k, v in model.state_dict().items() if "running" in k}


@pytest.mark.parametrize("B,T", [(2, 750), (8, 750), (2, 401), (BIG, 750)])
def test_forward_and_gradients_vs_fp64(B, T):
    model = _model()
    x = synth_feat((B, 1, H0, T), seed=61 + T).cuda()
    gf = synth_feat((B, 256), 62).cuda()
    go = synth_feat((B, 2), 63).cuda()
    P = _fp64_params(model)
    bufs = _buffers64(model)
    model.eval()
    with torch.no_grad():
        fe, oe = model(x)
        fe64, oe64 = o.forward(P, x.double(), False, buffers=_buffers64(model))
    assert _rel(fe.cpu(), fe64.detach().cpu()) <= 1e-4
    assert _rel(oe.cpu(), oe64.detach().cpu()) <= 1e-4
    model.train()
    feat, out = model(x)
    ((feat * gf).sum() + (out * go).sum()).backward()
    f64, o64 = o.forward(P, x.double(), True, buffers=bufs)
    ((f64 * gf.double()).sum() + (o64 * go.double()).sum()).backward()
    assert _rel(feat.detach().cpu(), f64.detach().cpu()) <= 1e-4
    assert _rel(out.detach().cpu(), o64.detach().cpu()) <= 1e-4
    # the band of plain fp32: with the filler's parameters the deep BatchNorm chain at small B amplifies fp32
    # rounding, and torch's own fp32 gradients are off the fp64 ones by up to ~1 % (273 of 295 tensors above 1e-3
    # at B = 2).  Each gradient is held to 1e-3 or to three times that band, whichever is larger.
    P32 = {k: v.detach().clone().requires_grad_(True) for k, v in model.named_parameters()}
    f32, o32 = o.forward(P32, x, True, buffers={k: v.float() for k, v in _buffers64(model).items()})
    ((f32 * gf).sum() + (o32 * go).sum()).backward()
    bad = []
    for k, p in model.named_parameters():
        r = _rel(p.grad.cpu(), P[k].grad.cpu())
        band = _rel(P32[k].grad.cpu(), P[k].grad.cpu())
        if r > max(1e-3, 3 * band):
            bad.append((k, r, band))
    assert not bad, bad
    sd = model.state_dict()
    for k, v in bufs.items():
        close(sd[k], v, 1e-5, k)
    assert int(sd["layer2.0.bns.1.num_batches_tracked"]) == int(fill_value("layer2.0.bns.1.num_batches_tracked",
                                                                             ()).item()) + 1


def test_golden_forward_and_gradient_norms(golden):
    g = golden("res2net.npz")
    for T in (750, 401):
        model = _model()
        x = synth_feat((2, 1, H0, T), seed=int(g["cfg"][1]) + T).cuda()
        model.eval()
        with torch.no_grad():
            fe, oe = model(x)
        assert _rel(fe.cpu(), g["feat_eval/%d" % T]) <= 1e-4
        assert _rel(oe.cpu(), g["out_eval/%d" % T]) <= 1e-4
        model.train()
        feat, out = model(x)
        labels = torch.from_numpy(g["labels"]).cuda()
        F.nll_loss(out, labels).backward()  # CrossEntropyLoss on log-probs == nll of log_softmax(log-probs)
        gn = np.array([float(p.grad.double().norm()) for _, p in model.named_parameters()])
        ref = g["grad_norm/ce/%d" % T]
        # the reference's own fp32 run is off the fp64 restatement by up to 7 % on a few SE gradients (printed by
        # make_golden_res2net.py); the strict bound is test_forward_and_gradients_vs_fp64's
        r = np.abs(gn - ref) / (ref + 1e-30)
        assert np.median(r) <= 2e-3 and r.max() <= 0.15, (np.median(r), r.max())
        sd = model.state_dict()
        for k in sd:
            if "running" in k:
                np.testing.assert_allclose(sd[k].cpu().numpy(), g["after/%d/%s" % (T, k)], rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------------------------------ training
@pytest.mark.parametrize("add_loss", [None, "ang_iso", "isolate", "iso_sq", "p2sgrad"])
def test_trainer_heads_graph_replay_bit_identical(add_loss):
    from asvspoof2021_air_amd.train import Trainer
    pcm = synth_pcm(4, 16000, seed=71).cuda()
    labels = torch.tensor([0, 1, 1, 0]).cuda()
    runs = []
    for graph in (False, True):
        torch.manual_seed(5)
        tr = Trainer(_model(), add_loss=add_loss, feat_len=200)
        if tr.loss is not None:
            fill_module_(tr.loss)
        if graph:
            tr.enable_graph(True)
        losses = [float(tr.step(pcm, labels)[0]) for _ in range(3)]
        torch.cuda.synchronize()
        runs.append((losses, tr.model.arena().flat.clone(), {k: v.clone() for k, v in tr.model.state_dict().items()}))
    assert all(np.isfinite(runs[0][0]))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1])
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k


def test_three_adam_steps_vs_fp64():
    """Three Trainer steps (CE head) against the fp64 restatement under torch's Adam, bounded by 1e-4 or three times
    what a plain fp32 run of the restatement is off fp64 (the band test_forward_and_gradients_vs_fp64 explains)."""
    from asvspoof2021_air_amd.train import Trainer
    B, T = 4, 200
    model = _model()
    tr = Trainer(model, add_loss=None, feat_len=T)
    pcm = synth_pcm(B, 16000, seed=81).cuda()
    labels = torch.tensor([0, 1, 1, 0]).cuda()
    runs = {}
    for dt in (torch.float64, torch.float32):
        P = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in model.named_parameters()}
        bufs = {k: v.detach().to(dt).clone() for k, v in model.state_dict().items() if "running" in k}
        opt = torch.optim.Adam(list(P.values()), lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0005)
        runs[dt] = (P, bufs, opt, [])
    for _ in range(3):
        with torch.no_grad():
            x = tr.features(pcm, None)
        loss, _ = tr.step(pcm, labels)
        for dt, (P, bufs, opt, losses) in runs.items():
            opt.zero_grad()
            _, ol = o.forward(P, x.to(dt), True, buffers=bufs)
            lo = F.nll_loss(ol, labels)
            lo.backward()
            opt.step()
            losses.append(lo.item())
        l64, l32 = runs[torch.float64][3][-1], runs[torch.float32][3][-1]
        assert abs(float(loss) - l64) <= max(1e-4, 3 * abs(l32 - l64)) * max(1.0, abs(l64)), (float(loss), l64, l32)
    torch.cuda.synchronize()
    # Adam moves an element whose gradient is rounding noise by up to lr per step in a direction the noise picks:
    # every element stays within three such steps of fp64 both ways, and all but a few tensors within the fp32 band
    P64, P32 = runs[torch.float64][0], runs[torch.float32][0]
    lr, off = 5e-4, []
    for k, p in model.named_parameters():
        d = (p.detach().double() - P64[k].detach()).abs().max().item()
        assert d <= 6 * lr, (k, d)
        band = (P32[k].detach().double() - P64[k].detach()).abs().max().item()
        if d > max(1e-3 * P64[k].abs().max().item(), 3 * band):
            off.append((k, d, band))
    assert len(off) <= 0.05 * len(P64), off


def test_score_from_pickle():
    from asvspoof2021_air_amd.generate_score import batch_scores
    model = _model()
    model.train()
    x = synth_feat((2, 1, H0, 300), seed=91).cuda()
    feat, out = model(x)
    out.sum().backward()  # builds the arena, the side stream and the gradient views
    buf = io.BytesIO()
    torch.save(model, buf)
    buf.seek(0)
    m2 = torch.load(buf, weights_only=False)
    m2.eval()
    model.eval()
    s1 = batch_scores(model, x)
    s2 = batch_scores(m2, x)
    assert torch.equal(s1, s2)
    with torch.no_grad():
        P = {k: v.detach().double() for k, v in model.named_parameters()}
        _, o64 = o.forward(P, x.double(), False, buffers=_buffers64(model))
    close(s1, -torch.softmax(o64, dim=1)[:, 0], 1e-4, "score")


def _aten_kernels_per_step(tr, pcm, labels, steps=2):
    """{kernel name: launches per step} of the ATen kernels among the device kernels of ``steps`` eager train steps
    (after two warm-up steps), and the set of all kernel names (tests/test_lcnn_gpu.py's measure)."""
    from torch.profiler import ProfilerActivity, profile
    for _ in range(2):
        tr.step(pcm, labels)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            tr.step(pcm, labels)
        torch.cuda.synchronize()
    names = {}
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            names[ev.name] = names.get(ev.name, 0) + 1
    aten = {k: v / steps for k, v in names.items() if "at::" in k or "elementwise" in k or "Functor" in k}
    return aten, set(names)


def test_step_runs_no_aten_compute_beyond_the_resnet_step():
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.resnet import ResNet
    from asvspoof2021_air_amd.train import Trainer
    pcm = synth_pcm(4, 16000, seed=97).cuda()
    labels = torch.tensor([0, 1, 1, 0]).cuda()
    tr = Trainer(_model(), loss_module=fill_module_(AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)),
                 feat_len=750)
    aten_m, all_m = _aten_kernels_per_step(tr, pcm, labels)
    assert any("narrow_fwd_kernel" in k for k in all_m) and any("se_relu_bwd_kernel" in k for k in all_m), \
        sorted(all_m)[:20]  # the trace does see the library's kernels
    r = fill_module_(ResNet(3, 256, resnet_type="18", nclasses=2))
    r.set_attention_noise(None)
    tr = Trainer(r, loss_module=fill_module_(AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)), feat_len=750)
    aten_r, _ = _aten_kernels_per_step(tr, pcm, labels)
    extra = {k: v for k, v in aten_m.items() if v > aten_r.get(k, 0)}
    assert not extra, (extra, aten_r)
