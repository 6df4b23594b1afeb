"""GPU: the loss heads of csrc/loss_heads.hip (P2SGrad, Isolate / IsolateSquare, AMSoftmax) against the golden from the
real reference and the fp64 restatement (tests/loss_heads_oracle.py), their edges and determinism; ``Trainer`` under
every ``add_loss`` head (eager trajectory against fp64, hipGraph replay bit-identical to eager, the CE head's tail,
no ATen kernels beyond the OC-Softmax step); scoring and checkpoints of the heads."""
import os

import numpy as np
import pytest
import torch

import lcnn_oracle as lo
import loss_heads_oracle as o
from oracle.filler import fill_module_, fill_value, synth_pcm

pytestmark = pytest.mark.gpu


def _d(t):
    return t.detach().cpu().double()


def _close(got, want, rtol=1e-5, what=""):
    """fp32 against fp64 at ~rtol of the output's scale (NaN where the reference has NaN)."""
    got, want = np.asarray(_d(got) if torch.is_tensor(got) else got, np.float64), np.asarray(
        _d(want) if torch.is_tensor(want) else want, np.float64)
    scale = np.nanmax(np.abs(want)) if np.isfinite(want).any() else 1.0
    np.testing.assert_allclose(got, want, rtol=rtol, atol=rtol * max(scale, 1e-30) * 4, equal_nan=True, err_msg=what)


def _heads(P):
    from asvspoof2021_air_amd.loss import AMSoftmax, IsolateLoss, IsolateSquareLoss, P2SGradLoss
    m = {"p2s0": P2SGradLoss(256, 2, smooth=0.0), "p2s0.1": P2SGradLoss(256, 2, smooth=0.1),
         "iso": IsolateLoss(2, 256), "isosq": IsolateSquareLoss(2, 256), "ams": AMSoftmax(2, 256)}
    with torch.no_grad():
        for k, v in m.items():
            (v.centers if k == "ams" else v.weight if k.startswith("p2s") else v.center).copy_(
                P["ams" if k == "ams" else "p2s" if k.startswith("p2s") else "iso"])
    return {k: v.cuda() for k, v in m.items()}


def _run(m, x, labels):
    """(outputs, dx, dparam) of one head module on the GPU."""
    xx = x.cuda().requires_grad_(True)
    out = m(xx, labels.cuda())
    loss = out[0] if isinstance(out, tuple) else out
    loss.backward()
    p = next(m.parameters())
    res = (out, xx.grad.clone(), p.grad.clone())
    p.grad = None
    return res


@pytest.mark.parametrize("case", ["mixed", "bona"])
def test_heads_vs_reference_golden(golden, case):
    g = golden("heads.npz")
    B = int(g["cfg"][0])
    x, labels = o.inputs(B)
    if case == "bona":
        labels = torch.zeros(B, dtype=torch.int64)
    H = _heads(o.params())
    for k in ("p2s0", "p2s0.1"):
        (loss, neg), dx, dw = _run(H[k], x, labels)
        tag = "%s_%s" % (k, case)
        _close(loss, g[tag + "_loss"], what=tag)
        _close(neg, g[tag + "_neg"], what=tag)
        _close(dx, g[tag + "_dx"], 1e-4, tag)
        _close(dw, g[tag + "_dw"], 1e-4, tag)
    for k in ("iso", "isosq"):
        loss, dx, dc = _run(H[k], x, labels)
        tag = "%s_%s" % (k, case)
        if case == "bona":
            assert torch.isnan(loss).item() and torch.isfinite(dx).all() and torch.isfinite(dc).all()
        _close(loss, g[tag + "_loss"], what=tag)
        _close(dx, g[tag + "_dx"], 1e-4, tag)
        _close(dc, g[tag + "_dc"], 1e-4, tag)
    with torch.no_grad():
        lg, mg = H["ams"](x.cuda(), labels.cuda())
    _close(lg, g["ams_%s_logits" % case])
    _close(mg, g["ams_%s_margin" % case])


@pytest.mark.parametrize("B", [1, 2, 64, 128, 4096])
def test_heads_vs_fp64(B):
    x, labels = o.inputs(B, seed=1400 + B)
    P = o.params()
    H = _heads(P)
    for k, smooth in (("p2s0", 0.0), ("p2s0.1", 0.1)):
        (loss, neg), dx, dw = _run(H[k], x, labels)
        (l64, n64), (dx64, dw64) = o.grads(lambda a, w: o.p2sgrad(a, w, labels, smooth), _d(x), _d(P["p2s"]))
        _close(loss, l64, what=k)
        _close(neg, n64, what=k)
        _close(dx, dx64, 1e-4, k)  # per-element gradients: a few ulp of the row sums
        _close(dw, dw64, 1e-4, k)
    for k, sq in (("iso", False), ("isosq", True)):
        loss, dx, dc = _run(H[k], x, labels)
        l64, (dx64, dc64) = o.grads(lambda a, c: o.isolate(a, c, labels, square=sq), _d(x), _d(P["iso"]))
        _close(loss, l64, what=k)
        _close(dx, dx64, 1e-4, k)
        _close(dc, dc64, 1e-4, k)
    with torch.no_grad():
        lg, mg = H["ams"](x.cuda(), labels.cuda())
    l64, m64 = o.amsoftmax(_d(x), _d(P["ams"]), labels)
    _close(lg, l64)
    _close(mg, m64)


def test_edges():
    from asvspoof2021_air_amd import ops
    from asvspoof2021_air_amd._hip import AirError
    P = o.params()
    H = _heads(P)
    x, labels = o.inputs(8)
    # Isolate: rows AT the centre pass no gradient (the norm's gradient is 0 there) and a one-class batch is NaN
    x[1] = P["iso"][0]
    x[2] = P["iso"][0]
    for k, sq in (("iso", False), ("isosq", True)):
        loss, dx, dc = _run(H[k], x, labels)
        assert torch.count_nonzero(dx[1:3]) == 0
        l64, (dx64, dc64) = o.grads(lambda a, c: o.isolate(a, c, labels, square=sq), _d(x), _d(P["iso"]))
        _close(loss, l64)
        _close(dx, dx64, 1e-4)
        _close(dc, dc64, 1e-4)
        ones = torch.ones(8, dtype=torch.int64)
        loss1, dx1, dc1 = _run(H[k], x, ones)
        assert torch.isnan(loss1).item() and torch.isfinite(dx1).all() and torch.isfinite(dc1).all()
    # P2SGrad: rows parallel / antiparallel to a weight column give cos = +-1 (clamped, finite, exact at 1e-6)
    w = P["p2s"].renorm(2, 1, 1e-5).mul(1e5)
    x[3], x[4] = 3.0 * w[:, 0], -0.5 * w[:, 0]
    (loss, neg), dx, dw = _run(H["p2s0"], x, labels)
    assert torch.isfinite(dx).all() and torch.isfinite(dw).all() and torch.isfinite(loss)
    np.testing.assert_allclose(neg[3:5].cpu().numpy(), [-1.0, 1.0], atol=1e-6)
    (l64, n64), (dx64, _) = o.grads(lambda a, ww: o.p2sgrad(a, ww, labels, 0.0), _d(x), _d(P["p2s"]))
    _close(loss, l64)
    _close(dx, dx64, 1e-4)
    # B = 4097 is refused by every launch
    xb, lb = o.inputs(4097)
    xb, lb = xb.cuda(), lb.cuda()
    for call in (lambda: ops.p2sgrad_fwd(xb, P["p2s"].cuda(), lb, 0.0),
                 lambda: ops.p2sgrad_bwd(xb, P["p2s"].cuda(), lb, 0.0),
                 lambda: ops.isolate_fwd(xb, P["iso"].cuda(), lb, 0.9, 0.2, False),
                 lambda: ops.isolate_bwd(xb, P["iso"].cuda(), lb, 0.9, 0.2, True),
                 lambda: ops.amsoftmax_fwd(xb, P["ams"].cuda(), lb, 20.0, 0.9)):
        with pytest.raises(AirError, match="unsupported|EUNSUPPORTED|-2"):
            call()
    with pytest.raises(NotImplementedError):
        H["ams"](x.cuda().requires_grad_(True), labels.cuda())  # forward-only, as the reference uses it


def test_two_launches_bit_identical():
    x, labels = o.inputs(128, seed=1500)
    H = _heads(o.params())
    for k in ("p2s0.1", "iso", "isosq"):
        a, b = _run(H[k], x, labels), _run(H[k], x, labels)
        la, lb_ = (a[0][0], b[0][0]) if isinstance(a[0], tuple) else (a[0], b[0])
        assert torch.equal(la, lb_) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), k
    with torch.no_grad():
        a, b = H["ams"](x.cuda(), labels.cuda()), H["ams"](x.cuda(), labels.cuda())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ Trainer
def _lcnn(seed=None):
    from asvspoof2021_air_amd.lcnn import LCNN
    m = fill_module_(LCNN(60, 256, nclasses=2)).cuda()
    if seed is not None:
        m._mask_seed = seed
    return m


def _resnet():
    from asvspoof2021_air_amd.resnet import ResNet
    m = fill_module_(ResNet(3, 256, resnet_type="18", nclasses=2)).cuda()
    m.set_attention_noise(None)
    return m


def _ecapa(dtype):
    from asvspoof2021_air_amd.ecapa_tdnn import Bottle2neck, Res2Net2
    return fill_module_(Res2Net2(Bottle2neck, C=512, model_scale=8, nOut=2, n_mels=60)).cuda().set_compute_dtype(dtype)


def _trainer(m, head, graph=False, **kw):
    from asvspoof2021_air_amd.train import Trainer
    torch.manual_seed(0)
    tr = Trainer(m, add_loss=head, r_real=0.9, r_fake=0.2, **kw)
    if tr.loss is not None:
        fill_module_(tr.loss)
        if head in ("isolate", "iso_sq"):
            with torch.no_grad():
                tr.loss.center.mul_(0.1)
    if graph:
        tr.enable_graph(True)
    return tr


def _batch(B, i, L=16000):
    return synth_pcm(B, L, seed=100 + i).cuda(), torch.tensor([0, 1] * (B // 2)).cuda()


def _head64(head, f64, out64, p, labels):
    if head is None:
        return o.cross_entropy(out64, labels)
    if head == "isolate":
        return o.isolate(f64, p, labels, r_real=0.9, r_fake=0.2)
    return o.p2sgrad(f64, p, labels, 0.0)[0]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.mark.parametrize("head", [None, "isolate", "p2sgrad"])
def test_lcnn_trainer_trajectory_vs_fp64(head):
    """Three Trainer steps (Adam on the arena, SGD on the head parameter) against the same steps in fp64, as
    tests/test_lcnn_gpu.py does for OC-Softmax: loss at 1e-4 before any update, 1e-3 after; the step-1 gradient of the
    whole arena within 1e-3 relative L2 of fp64's; every tensor's total update within 10 % relative L2 of fp64's - except
    the biases of the convolutions whose MFM output feeds a BatchNorm: their gradient is ~0 in exact arithmetic (the
    normalisation removes the shift wherever the channel wins the MFM), and the first Adam updates (~lr * sign(g)) turn
    its rounding into full-size steps.  The step-1 gradient of the whole arena is within 1 % relative L2 of fp64's (MFM
    and pool decisions within rounding of a tie may go the other way in fp32).  Under CE fc_mu receives a gradient
    and moves."""
    from oracle.train import adam_step_, sgd_step_
    B = 4
    m = _lcnn()
    gk = torch.Generator().manual_seed(3)
    keep = (torch.rand(B, 4416, generator=gk) >= 0.7).float() / 0.3
    m.set_dropout_mask(keep)
    tr = _trainer(m, head)
    pcm, labels = _batch(B, 0)
    if head is None:  # the filled fc_mu classifies this batch at a CE of 1e-7: train against the other labels
        labels = 1 - labels
    x = tr.features(pcm).cpu().double()
    p0 = {k: v.detach().cpu().double() for k, v in m.named_parameters()}
    p64 = {k: v.clone() for k, v in p0.items()}
    b64 = {k: v.detach().cpu().double().clone() for k, v in m.state_dict().items() if "running" in k}
    h64 = _d(next(tr.loss.parameters())) if tr.loss is not None else None
    mom = {k: (torch.zeros_like(v), torch.zeros_like(v)) for k, v in p64.items()}
    for step in range(1, 4):
        loss, _ = tr.step(pcm, labels)
        pr = {k: v.clone().requires_grad_(True) for k, v in p64.items()}
        hr = h64.clone().requires_grad_(True) if h64 is not None else None
        f64, out64, _ = lo.forward(pr, x, True, keep=keep, buffers=b64)
        l64 = _head64(head, f64, out64, hr, labels.cpu())
        l64.backward()
        # (atol: after one step the CE head separates the batch at a loss of ~1e-7, at the resolution of fp32)
        np.testing.assert_allclose(loss.item(), l64.item(), rtol=1e-4 if step == 1 else 1e-3, atol=1e-6 if step > 1 else 0)
        if step == 1:
            got = torch.cat([m.arena().grad_view(k).cpu().double().flatten() for k in p64 if pr[k].grad is not None])
            want = torch.cat([pr[k].grad.flatten() for k in p64 if pr[k].grad is not None])
            assert _rel(got.numpy(), want.numpy()) <= 1e-2, _rel(got.numpy(), want.numpy())
        with torch.no_grad():
            for k, p in p64.items():
                if pr[k].grad is not None:
                    adam_step_(p, pr[k].grad, mom[k][0], mom[k][1], step)
            if hr is not None:
                sgd_step_(h64, hr.grad, 5e-4)
    for k, v in m.named_parameters():
        got, want = v.detach().cpu().double() - p0[k], p64[k] - p0[k]
        if k.startswith("fc_mu") and head is not None:
            assert torch.count_nonzero(got) == 0
            continue
        if k.startswith("fc_mu"):
            assert torch.count_nonzero(got) == got.numel()  # the CE head trains fc_mu
        if k.endswith(".0.bias") and k.split(".")[0] in lo.BN_INDEX:
            continue
        assert _rel(got.numpy(), want.numpy()) <= 0.1, (k, _rel(got.numpy(), want.numpy()))
    if h64 is not None:
        np.testing.assert_allclose(_d(next(tr.loss.parameters())).numpy(), h64.numpy(), atol=1e-5)


def _graph_vs_eager(make, head, steps=5, B=4, **kw):
    me, mg = make(), make()
    te, tg = _trainer(me, head, **kw), _trainer(mg, head, graph=True, **kw)
    for i in range(steps):
        pcm, labels = _batch(B, i)
        if i == 3:
            tg.use_graph = False  # an eager step between replays
        le, se = te.step(pcm, labels)
        lg, sg = tg.step(pcm, labels)
        tg.use_graph = True
        torch.cuda.synchronize()
        assert torch.equal(le, lg) or (torch.isnan(le).item() and torch.isnan(lg).item()), (head, i)
        assert (se is None and sg is None) or torch.equal(se, sg), (head, i)
        assert torch.equal(me.arena().flat, mg.arena().flat), (head, i)
        for pe, pg in zip(te._loss_params(), tg._loss_params()):
            assert torch.equal(pe, pg), (head, i)
    assert tg._graph is not None
    return me, te


@pytest.mark.parametrize("model", ["resnet", "lcnn"])
@pytest.mark.parametrize("head", [None, "isolate", "p2sgrad"])
def test_graph_replay_bit_identical_to_eager(model, head):
    make = {"resnet": _resnet, "lcnn": lambda: _lcnn(seed=1234)}[model]
    m0 = make()
    tail0 = {k: v.detach().clone() for k, v in m0.named_parameters() if k.startswith("fc_mu")}
    me, te = _graph_vs_eager(make, head)
    moved = [not torch.equal(v, tail0[k]) for k, v in me.named_parameters() if k.startswith("fc_mu")]
    assert all(moved) if head is None else not any(moved)
    assert me.arena().tail_has_grad == (head is None)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_ecapa_ce_head_graph_replay_and_tail(dtype):
    """ECAPA under CE: the gradient enters through fc7 / bn7 (ecapa_tdnn.py's tail), Adam moves them, and hipGraph
    replay is bit-identical to the eager step."""
    make = lambda: _ecapa(dtype)
    m0 = make()
    tail0 = {k: v.detach().clone() for k, v in m0.named_parameters() if k.startswith(("fc7", "bn7"))}
    assert tail0
    me, te = _graph_vs_eager(make, None, steps=4, B=8, feat_len=128, ecapa=True)
    for k, v in me.named_parameters():
        if k in tail0:
            assert not torch.equal(v, tail0[k]), k
    assert me.arena().tail_has_grad


def _aten_kernels_per_step(tr, pcm, labels, steps=2):
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


@pytest.mark.parametrize("head", [None, "isolate", "iso_sq", "p2sgrad"])
def test_step_runs_no_aten_compute_beyond_the_ocsoftmax_step(head):
    B = 4
    pcm, labels = _batch(B, 0)
    ref, _ = _aten_kernels_per_step(_trainer(_lcnn(), "ang_iso"), pcm, labels)
    got, names = _aten_kernels_per_step(_trainer(_lcnn(), head), pcm, labels)
    want = {None: "softmax_ce", "isolate": "iso_bwd_kernel", "iso_sq": "iso_bwd_kernel", "p2sgrad": "p2s_bwd_kernel"}
    assert any(want[head] in k for k in names), sorted(names)[:30]
    extra = {k: v for k, v in got.items() if v > ref.get(k, 0)}
    assert not extra, (extra, ref)


@pytest.mark.parametrize("head", [None, "isolate", "iso_sq", "ang_iso", "p2sgrad"])
def test_eval_batch_loss_and_score(head):
    """Trainer.eval_batch: main_train.py:526-575's dev loss and score of each head, against fp64 on the same features."""
    from asvspoof2021_air_amd import ops
    tr = _trainer(_lcnn(), head)
    pcm, labels = _batch(4, 7)
    loss, score = tr.eval_batch(pcm, labels)
    with torch.no_grad():
        feats, logits = tr.model(tr.features(pcm))
    f, lg, lab = _d(feats), _d(logits), labels.cpu()
    if head is None:
        want_l, want_s = o.cross_entropy(lg, lab), torch.softmax(lg, 1)[:, 0]
    elif head in ("isolate", "iso_sq"):
        c = _d(tr.loss.center)
        want_l = o.isolate(f, c, lab, 0.9, 0.2, square=head == "iso_sq")
        want_s = torch.norm(f - c, p=2, dim=1)
    elif head == "p2sgrad":
        want_l, want_s = o.p2sgrad(f, _d(tr.loss.weight), lab, 0.0)
    else:
        want_l, want_s = lo.ocsoftmax(f, _d(tr.loss.center), lab)
    _close(loss, want_l, 1e-5)
    _close(score, want_s, 1e-5)
    assert not tr.model.training
    del ops


# ------------------------------------------------------------------------------------------------ scoring / checkpoints
@pytest.mark.parametrize("add_loss", ["p2sgrad", "amsoftmax"])
def test_generate_score_heads(add_loss):
    """generate_score.batch_scores / GraphedScorer with the p2sgrad and amsoftmax heads (generate_score.py:98-110):
    the oracle's score on the model's features; batch 1 == batch N; graphed batch 1 == eager."""
    from asvspoof2021_air_amd.generate_score import GraphedScorer, batch_scores
    from asvspoof2021_air_amd.loss import AMSoftmax, P2SGradLoss
    m = _lcnn().eval()
    head = (P2SGradLoss(256, 2, smooth=0.0) if add_loss == "p2sgrad" else AMSoftmax(2, 256)).cuda()
    fill_module_(head)
    from asvspoof2021_air_amd.feature_extraction import LFCC
    lfcc = LFCC(320, 160, 512, 16000, 20, with_energy=False).cuda()
    lfcc.mutate_input = False
    pcm, _ = _batch(4, 9)
    feat = lfcc.forward_padded(pcm, 750, None).unsqueeze(1).contiguous()
    s = batch_scores(m, feat, head, add_loss)
    with torch.no_grad():
        feats, _ = m(feat)
    zeros = torch.zeros(4, dtype=torch.int64)
    if add_loss == "p2sgrad":
        want = o.p2sgrad(_d(feats), _d(head.weight), zeros, 0.0)[1]
    else:
        want = torch.softmax(o.amsoftmax(_d(feats), _d(head.centers), zeros)[0], 1)[:, 0]
    _close(s, want, 1e-5)
    ones = torch.cat([batch_scores(m, feat[i:i + 1], head, add_loss) for i in range(4)])
    _close(ones, s, 1e-5)  # (the model's kernels may differ with the batch size; the head's rows are independent:)
    zl = zeros.cuda()
    with torch.no_grad():
        if add_loss == "p2sgrad":
            rows = torch.cat([head(feats[i:i + 1], zl[:1])[1] for i in range(4)])
            assert torch.equal(rows, head(feats, zl)[1])
        else:
            rows = torch.cat([head(feats[i:i + 1], zl[:1])[0] for i in range(4)])
            assert torch.equal(rows, head(feats, zl)[0])
    gs = GraphedScorer(m, feat[:1], head, add_loss)
    for i in range(4):
        assert torch.equal(gs(feat[i:i + 1]).clone(), ones[i:i + 1])


def test_checkpoints_per_head(tmp_path):
    """add_loss=None writes no loss-model file; the p2sgrad and isolate loss pickles load back with torch.load and score."""
    from asvspoof2021_air_amd.generate_score import batch_scores
    pcm, labels = _batch(4, 11)
    tr = _trainer(_lcnn(), None)
    tr.set_out_fold(str(tmp_path / "ce"))
    tr.step(pcm, labels)
    tr.save_checkpoint(0, val_loss=1.0)
    assert sorted(os.listdir(tmp_path / "ce" / "checkpoint")) == ["anti-spoofing_feat_model_1.pt"]
    assert not os.path.exists(tmp_path / "ce" / "anti-spoofing_loss_model.pt")
    for head in ("p2sgrad", "isolate"):
        tr = _trainer(_lcnn(), head)
        out = str(tmp_path / head)
        tr.set_out_fold(out)
        tr.step(pcm, labels)
        assert tr.save_checkpoint(0, val_loss=tr.eval_batch(pcm, labels)[0].item() if head == "p2sgrad" else 1.0)
        model = torch.load(os.path.join(out, "anti-spoofing_feat_model.pt"), weights_only=False).eval()
        lossm = torch.load(os.path.join(out, "anti-spoofing_loss_model.pt"), weights_only=False)
        assert type(lossm) is type(tr.loss)
        for a, b in zip(lossm.parameters(), tr.loss.parameters()):
            assert torch.equal(a, b)
        feat = tr.features(pcm)
        if head == "p2sgrad":
            assert torch.equal(batch_scores(model, feat, lossm, "p2sgrad"), batch_scores(tr.model.eval(), feat, tr.loss,
                                                                                         "p2sgrad"))
        else:
            loss = lossm(model(feat)[0], labels)
            assert torch.isfinite(loss)


def test_isolate_lr_decay_quirk():
    """main_train.py:287-300: set_epoch decays the isolate head's SGD rate but never iso_sq's."""
    for head, want in (("isolate", 2.5e-4), ("iso_sq", 5e-4), ("p2sgrad", 2.5e-4)):
        tr = _trainer(_lcnn(), head)
        tr.set_epoch(30)
        assert tr.feat_optimizer.param_groups[0]["lr"] == 2.5e-4
        assert tr.loss_optimizer.param_groups[0]["lr"] == want, head
    tr = _trainer(_lcnn(), None)
    tr.set_epoch(30)
    assert tr.loss_optimizer is None and tr.loss is None
