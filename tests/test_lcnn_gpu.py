"""GPU: the LCNN (model.py:511-610) on its HIP kernels - the MFM / pool kernels bit-exact against torch, the fused conv1
against fp64, the model forward / gradients / running statistics against the golden and the fp64 restatement
(tests/lcnn_oracle.py), Trainer steps eager and hipGraph-replayed, scoring from a whole-module pickle, and one
full-size step."""
import io

import numpy as np
import pytest
import torch

import lcnn_oracle as o
from oracle.filler import fill_module_, fill_value, synth_feat, synth_pcm

pytestmark = pytest.mark.gpu


def _model(seed=None):
    from asvspoof2021_air_amd.lcnn import LCNN
    m = fill_module_(LCNN(60, 256)).cuda()
    if seed is not None:
        m._mask_seed = seed
    return m


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("shape,C,pool", [((2, 96, 30, 375), 96, True), ((3, 128, 15, 187), 96, True),
                                          ((2, 64, 7, 93), 64, False), ((2, 64, 7, 93), 64, True),
                                          ((4, 160, 1, 1), 160, False)])
def test_mfm_pool_kernels_bit_exact(shape, C, pool):
    from asvspoof2021_air_amd import ops
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-4, 4, shape, generator=g).float()  # integers: many exact ties (first candidate wins)
    x[0, 0] = torch.randn(shape[2:], generator=g)
    bias = torch.randint(-2, 2, (C,), generator=g).float()
    y, r = ops.mfm_pool_fwd(x.cuda(), C=C, bias=bias.cuda(), pool=pool)
    # torch: the reference's bias add, view(B, 2, C/2, ...).max(1), max_pool2d
    xt = (x[:, :C] + bias.view(1, C, 1, 1)).requires_grad_(True)
    want = o.mfm(xt)
    if pool:
        want = torch.nn.functional.max_pool2d(want, 2, 2)
    assert torch.equal(y.cpu(), want.detach())
    assert torch.equal(r.cpu(), o.routes_of(xt.detach(), pool))
    dy = torch.randn(want.shape, generator=g)
    want.backward(dy)
    dx = ops.mfm_pool_bwd(dy.cuda(), r, shape, C=C, pool=pool).cpu()
    assert torch.equal(dx[:, :C], xt.grad)
    assert torch.count_nonzero(dx[:, C:]) == 0
    db = ops.mfm_bias_grad(dy.cuda(), r).cpu().double()
    np.testing.assert_allclose(db.numpy(), xt.grad.double().sum((0, 2, 3)).numpy(), rtol=1e-5, atol=1e-4)


def test_conv1_fused_forward_and_weight_gradient():
    from asvspoof2021_air_amd import ops
    B, H, W = 2, 60, 750
    x = synth_feat((B, 1, H, W), seed=31)
    w = fill_value("conv1.0.weight", (64, 1, 5, 5))
    b = fill_value("conv1.0.bias", (64,))
    y, r = ops.lcnn_conv1_fwd(x.cuda(), w.cuda(), b.cuda())
    pre = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), padding=2)
    want = torch.nn.functional.max_pool2d(o.mfm(pre), 2, 2)
    scale = want.abs().max().item()
    assert (y.cpu().double() - want).abs().max().item() <= 1e-5 * scale
    routes = o.routes_of(pre, True)
    flips = int((r.cpu() != routes).sum())
    assert flips <= 1e-4 * r.numel(), flips
    # weight / bias gradient through the GPU's own decisions
    dy = synth_feat(tuple(y.shape), seed=32)
    dw = torch.empty(64, 1, 5, 5, device="cuda")
    db = torch.empty(64, device="cuda")
    ops.lcnn_conv1_wgrad(x.cuda(), dy.cuda(), r, dw, db)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = torch.nn.functional.conv2d(x.double(), w64, b64, padding=2)
    (o.route_select(pre, r.cpu(), True) * dy.double()).sum().backward()
    assert (dw.cpu().double() - w64.grad).abs().max().item() <= 1e-5 * w64.grad.abs().max().item()
    assert (db.cpu().double() - b64.grad).abs().max().item() <= 1e-5 * b64.grad.abs().max().item()
    # deterministic: a second run returns the same bits
    dw2, db2 = torch.empty_like(dw), torch.empty_like(db)
    ops.lcnn_conv1_wgrad(x.cuda(), dy.cuda(), r, dw2, db2)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


def test_dropout_mask_counter_advances():
    from asvspoof2021_air_amd import ops
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    a = ops.dropout_mask_ctr((8, 4416), 0.7, 77, ctr, "cuda")
    b = ops.dropout_mask_ctr((8, 4416), 0.7, 77, ctr, "cuda")
    assert int(ctr.item()) == 2 * 8 * 4416 // 4
    assert not torch.equal(a, b)
    vals = set(np.unique(a.cpu().numpy()).tolist())
    assert vals <= {0.0, np.float32(1 / 0.3)}
    assert abs((a > 0).float().mean().item() - 0.3) < 0.01
    # one draw body with air_dropout_mask: the device-counter form at offset 0 is the host-offset form at offset 0
    from asvspoof2021_air_amd.adversarial import dropout_mask
    assert torch.equal(a, dropout_mask((8, 4416), 0.7, 77, 0, "cuda"))


# ------------------------------------------------------------------------------------------------ model
def _oracle_params(m):
    return {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.named_parameters()}


def _oracle_bufs(m):
    return {k: v.detach().cpu().double().clone() for k, v in m.state_dict().items() if "running" in k}


def test_forward_vs_golden_b2(golden):
    g = golden("lcnn.npz")
    B, T, sx, _ = (int(v) for v in g["cfg"])
    x = synth_feat((B, 1, 60, T), seed=sx)
    m = _model().eval()
    with torch.no_grad():
        fe, oe = m(x.cuda())
    tol = lambda a: 1e-3 * np.abs(a).max()
    np.testing.assert_allclose(fe.cpu().numpy(), g["feat_eval"], atol=tol(g["feat_eval"]))
    np.testing.assert_allclose(oe.cpu().numpy(), g["out_eval"], atol=tol(g["out_eval"]))
    m.train()
    m.set_dropout_mask(torch.from_numpy(g["keep"]))
    with torch.no_grad():
        ft, ot = m(x.cuda())
    np.testing.assert_allclose(ft.cpu().numpy(), g["feat_train"], atol=tol(g["feat_train"]))
    np.testing.assert_allclose(ot.cpu().numpy(), g["out_train"], atol=tol(g["out_train"]))
    for k, v in m.state_dict().items():  # running statistics after one train-mode forward
        if "running" in k:
            np.testing.assert_allclose(v.cpu().numpy(), g["after/" + k], rtol=1e-4, atol=1e-5)
        if k.endswith("num_batches_tracked"):
            assert int(v.item()) == 1


@pytest.mark.parametrize("B", [2, 8, 64])
def test_forward_and_grads_vs_fp64(B):
    """Forward train + eval against the fp64 restatement; every parameter gradient against an fp64 backward that took
    the GPU's own MFM / pool decisions.  The decisions that differ from fp64's own (rounding near a tie) are counted:
    they must be rare, and the distance of the full fp64 run is then what they explain.  B = 64 is the reference's
    training batch: the launch shapes the model trains with (split counts, pixel tiles, the zero-padded 48-channel
    weight gradients)."""
    x = synth_feat((B, 1, 60, 750), seed=40 + B)
    m = _model()
    gk = torch.Generator().manual_seed(50 + B)
    keep = (torch.rand(B, 4416, generator=gk) >= 0.7).float() / 0.3
    m.set_dropout_mask(keep)
    m.train()
    bufs0 = _oracle_bufs(m)
    feat, saved = m.forward_saved(x.cuda())
    torch.cuda.synchronize()
    gpu_routes = {"conv1": saved["r1"].cpu(), "head": saved["rh"].cpu().view(B, 80, 1, 1)}
    for ent in saved["layers"]:
        gpu_routes[ent[0]] = ent[5].cpu()
    p64 = _oracle_params(m)
    f64, _, own = o.forward(p64, x.double(), True, keep=keep, buffers=bufs0, routes=gpu_routes)
    flips = sum(int((own[k] != gpu_routes[k]).sum()) for k in gpu_routes)
    total = sum(v.numel() for v in gpu_routes.values())
    assert flips <= 1e-4 * total, (flips, total)
    assert _rel(feat.cpu(), f64.detach()) <= 1e-4
    dfeat = synth_feat((B, 256), seed=60 + B)
    grads = m.backward_saved(saved, dfeat.cuda())
    torch.cuda.synchronize()
    f64.backward(dfeat.double())
    for (name, _, _, _), gr in zip(m.arena().entries, grads):
        if name.startswith("fc_mu"):
            assert gr is None
            continue
        want = p64[name].grad.numpy()
        got = gr.cpu().numpy()
        assert _rel(got, want) <= 1e-3, (name, _rel(got, want))
        assert np.abs(got - want).max() <= 1e-2 * np.abs(want).max(), name
    # eval mode on the updated running statistics
    m.eval()
    with torch.no_grad():
        fe, oe = m(x.cuda())
        fe64, oe64, _ = o.forward({k: v.detach() for k, v in p64.items()}, x.double(), False, buffers=_oracle_bufs(m))
    assert _rel(fe.cpu(), fe64) <= 1e-4 and _rel(oe.cpu(), oe64) <= 1e-4
    for k, v in m.state_dict().items():
        if "running" in k:
            np.testing.assert_allclose(v.cpu().numpy(), bufs0[k].numpy(), rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------------------------------ Trainer
def _trainer(m, graph=False, B=4):
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.train import Trainer
    lossm = fill_module_(AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0))
    tr = Trainer(m, loss_module=lossm, feat_len=750)
    if graph:
        tr.enable_graph(True)
    return tr


def _batch(B, i):
    return synth_pcm(B, 16000, seed=100 + i).cuda(), torch.tensor([0, 1] * (B // 2)).cuda()


def test_trainer_eager_step_and_trajectory_vs_fp64():
    """Three Trainer steps (Adam on the arena, SGD on the centre: main_train.py:175-176, :272) against the same three
    steps in fp64.  Step 1 is pre-update: loss and scores at 1e-4.  The first Adam updates are ~lr * sign(g), so a
    gradient entry within rounding of 0 can flip its whole update: the later losses get 1e-3, and every tensor's total
    update has to match fp64's to 10 % in relative L2 (a wrong gradient moves O(1) of a tensor's entries the wrong
    way)."""
    from oracle.train import adam_step_, sgd_step_
    B = 4
    m = _model()
    gk = torch.Generator().manual_seed(3)
    keep = (torch.rand(B, 4416, generator=gk) >= 0.7).float() / 0.3
    m.set_dropout_mask(keep)
    tr = _trainer(m)
    pcm, labels = _batch(B, 0)
    x = tr.features(pcm).cpu().double()
    p0 = {k: v.detach().cpu().double() for k, v in m.named_parameters()}
    p64 = {k: v.clone() for k, v in p0.items()}
    b64 = _oracle_bufs(m)
    c64 = fill_value("center", (1, 256)).double()
    mom = {k: (torch.zeros_like(v), torch.zeros_like(v)) for k, v in p64.items()}
    for step in range(1, 4):
        loss, neg = tr.step(pcm, labels)
        pr = {k: v.clone().requires_grad_(True) for k, v in p64.items()}
        cr = c64.clone().requires_grad_(True)
        f64, _, _ = o.forward(pr, x, True, keep=keep, buffers=b64)
        l64, n64 = o.ocsoftmax(f64, cr, labels.cpu())
        l64.backward()
        if step == 1:
            np.testing.assert_allclose(loss.item(), l64.item(), rtol=1e-4)
            np.testing.assert_allclose(neg.cpu().numpy(), n64.detach().numpy(), atol=1e-4)
        else:
            np.testing.assert_allclose(loss.item(), l64.item(), rtol=1e-3)
        with torch.no_grad():
            for k, p in p64.items():
                if pr[k].grad is not None:  # fc_mu: no gradient under ang_iso, left alone like torch.optim.Adam
                    adam_step_(p, pr[k].grad, mom[k][0], mom[k][1], step)
            sgd_step_(c64, cr.grad, 5e-4)
    for k, v in m.named_parameters():
        got, want = v.detach().cpu().double() - p0[k], p64[k] - p0[k]
        if k.startswith("fc_mu"):
            assert torch.count_nonzero(got) == 0
            continue
        assert _rel(got.numpy(), want.numpy()) <= 0.1, (k, _rel(got.numpy(), want.numpy()))
    np.testing.assert_allclose(tr.loss.center.detach().cpu().numpy(), c64.numpy(), atol=1e-5)


def test_graph_replay_bit_identical_to_eager_and_fresh_masks():
    B = 4
    me, mg = _model(seed=1234), _model(seed=1234)
    te, tg = _trainer(me), _trainer(mg, graph=True)
    ctrs = []
    for i in range(5):
        pcm, labels = _batch(B, i)
        if i == 3:
            tg.use_graph = False  # an eager step between replays
        le, ne = te.step(pcm, labels)
        lg, ng = tg.step(pcm, labels)
        tg.use_graph = True
        torch.cuda.synchronize()
        assert torch.equal(le, lg) and torch.equal(ne, ng), i
        assert torch.equal(me.arena().flat, mg.arena().flat), i
        assert int(me._mask_ctr.item()) == int(mg._mask_ctr.item())
        ctrs.append(int(mg._mask_ctr.item()))
    assert tg._graph is not None
    quads = (B * 4416 + 3) // 4
    assert ctrs == [quads * (i + 1) for i in range(5)]  # every replay drew a fresh mask


def test_generate_score_from_whole_module_pickle(tmp_path):
    from asvspoof2021_air_amd import generate_score as gs
    B = 4
    m = _model()
    tr = _trainer(m)
    tr.step(*_batch(B, 0))
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    m2 = torch.load(buf, weights_only=False).cuda()
    lossm = tr.loss
    feats = torch.stack([synth_feat((1, 750, 60), seed=200 + i) for i in range(B)])  # (B, 1, T, 60) as preprocess.py
    names = ["LA_%d" % i for i in range(B)]
    labels = torch.zeros(B, dtype=torch.int64)
    f1 = str(tmp_path / "s1.txt")
    fn = str(tmp_path / "sn.txt")
    gs.test_on_dataset(m2, [(feats[i:i + 1], names[i:i + 1], None, labels[i:i + 1]) for i in range(B)], f1, lossm,
                       "ocsoftmax")
    gs.test_on_dataset(m2, [(feats, names, None, labels)], fn, lossm, "ocsoftmax")
    s1 = [float(l.split()[1]) for l in open(f1)]
    sn = [float(l.split()[1]) for l in open(fn)]
    # the same utterance scored alone and in a batch of 4 is not bit-identical: the generic convolutions pick their
    # pixel tiling (and with it the summation order) from the batch size.  Rounding-level agreement is what holds.
    np.testing.assert_allclose(s1, sn, rtol=1e-5, atol=1e-6)
    with torch.no_grad():
        sc = gs.batch_scores(m2, feats.cuda().transpose(2, 3).contiguous(), lossm, "ocsoftmax")
    want = "".join(gs.format_score_line(n, v, "bonafide") for n, v in zip(names, (-sc).float().cpu().tolist()))
    assert open(fn).read() == want


def test_full_size_step():
    B = 64
    m = _model()
    tr = _trainer(m)
    pcm = synth_pcm(B, 64000, seed=9).cuda()
    labels = (torch.arange(B) % 2).cuda()
    loss, neg = tr.step(pcm, labels)
    torch.cuda.synchronize()
    assert np.isfinite(loss.item()) and torch.isfinite(neg).all()
    assert torch.isfinite(m.arena().flat).all()


def test_full_size_step_vs_fp64():
    """One Trainer step at the reference's training size (B = 64, 4 s, feat_len 750) on a fixed dropout mask: its loss
    and scores (pre-update, as step 1 of test_trainer_eager_step_and_trajectory_vs_fp64) against fp64 evaluated with
    the GPU's own MFM / pool decisions, taken by a twin model's forward on the same input; the decisions fp64 would take
    otherwise are counted.  The gradients at B = 64: test_forward_and_grads_vs_fp64[64]."""
    B = 64
    gk = torch.Generator().manual_seed(9)
    keep = (torch.rand(B, 4416, generator=gk) >= 0.7).float() / 0.3
    m, twin = _model(), _model()
    m.set_dropout_mask(keep)
    twin.set_dropout_mask(keep)
    tr = _trainer(m)
    pcm = synth_pcm(B, 64000, seed=9).cuda()
    labels = (torch.arange(B) % 2).cuda()
    x = tr.features(pcm)
    twin.train()
    _, saved = twin.forward_saved(x)
    torch.cuda.synchronize()
    routes = {"conv1": saved["r1"].cpu(), "head": saved["rh"].cpu().view(B, 80, 1, 1)}
    for ent in saved["layers"]:
        routes[ent[0]] = ent[5].cpu()
    p64 = {k: v.detach().cpu().double() for k, v in m.named_parameters()}
    b64 = _oracle_bufs(m)
    loss, neg = tr.step(pcm, labels)
    torch.cuda.synchronize()
    assert np.isfinite(loss.item()) and torch.isfinite(neg).all()
    with torch.no_grad():
        f64, _, own = o.forward(p64, x.cpu().double(), True, keep=keep, buffers=b64, routes=routes)
        l64, n64 = o.ocsoftmax(f64, fill_value("center", (1, 256)).double(), labels.cpu())
    flips = sum(int((own[k] != routes[k]).sum()) for k in routes)
    total = sum(v.numel() for v in routes.values())
    assert flips <= 1e-4 * total, (flips, total)
    np.testing.assert_allclose(loss.item(), l64.item(), rtol=1e-4)
    np.testing.assert_allclose(neg.cpu().numpy(), n64.numpy(), atol=1e-4)


def _aten_kernels_per_step(tr, pcm, labels, steps=2):
    """{kernel name: launches per step} of the ATen kernels among the device kernels of ``steps`` eager train steps
    (after two warm-up steps: arenas, optimiser state and workspaces exist), and the set of all kernel names."""
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
    """The LCNN train step's device kernels are HIP kernels of the library: any ATen kernel in it (per step, after
    warm-up) must also be in the ResNet step, at most as often."""
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.resnet import ResNet
    from asvspoof2021_air_amd.train import Trainer
    B = 4
    pcm, labels = _batch(B, 0)
    aten_l, all_l = _aten_kernels_per_step(_trainer(_model()), pcm, labels)
    assert any("conv1_fwd_kernel" in k for k in all_l) and any("mfm_pool_bwd_kernel" in k for k in all_l), \
        sorted(all_l)[:20]  # the trace does see the library's kernels
    r = fill_module_(ResNet(3, 256, resnet_type="18", nclasses=2))
    r.set_attention_noise(None)
    tr = Trainer(r, loss_module=fill_module_(AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)), feat_len=750)
    aten_r, _ = _aten_kernels_per_step(tr, pcm, labels)
    print("LCNN ATen kernels per step:", aten_l, "ResNet:", aten_r)
    extra = {k: v for k, v in aten_l.items() if v > aten_r.get(k, 0)}
    assert not extra, (extra, aten_r)
