"""GPU: every 2-D convolution route at the shapes the models train with, and at the edges of the dispatch heuristics.

One call of air_conv2d_fwd_pre / _dgrad_pre / _wgrad picks among about fifteen kernels and launch shapes from B, H, W,
Cin and Cout (csrc/conv2d.hip); several of the choices (K split, pixel-tile count, every split count) flip with the
batch.  So:

* the convolution calls of one eager ResNet-18 and one LCNN train step at B = 64 are recorded (shapes and flags,
  through wrappers around the ``ops`` entry points the models call) and each distinct signature is replayed alone
  against a float64 evaluation of the same operation, with the kernels that served it read from the profiler;
* boundary cases pin one route each (kernel names, the pixel-tile count from the template arguments, whether a
  ``reduce_partials_kernel`` followed) and hold it against fp64;
* the dispatch options nothing else sets are swept, each held to its kernel's bound, with the alternative shown to run;
* every ``*_kernel`` of the four convolution sources is launched by some case (or is on the allow-list with a reason);
* the stride-2 weight gradients without a kernel instance are refused, not answered;
* every route runs on a workspace of exactly air_conv2d_ws_bytes(p) bytes between sentinels, and is refused one byte below
  its own need.

References: float64 F.conv2d on the GPU through ATen's own convolution (MIOpen off: it has no fp64 kernels), checked
once against CPU float64.  Forward / data gradient are compared on the first, a middle and the last utterance (the
kernel still runs on the whole batch); weight gradients on the whole batch.  Bounds: STRICT["conv_rtol"] for the
direct and split-bf16 kernels, wino_conv_bound() for the Winograd forward / data gradient, 1e-5 for the Winograd weight
gradient (tests/test_kernels_gpu.py)."""
import contextlib
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.filler import fill_module_, synth_feat, synth_pcm

from _budget import STRICT, record, wino_conv_bound  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asvspoof2021_air_amd", "csrc")
CONV_SOURCES = ("conv2d.hip", "conv_wino.hip", "conv_wino4.hip", "conv_bf3.hip")
# kernels of those sources that no case launches, with the reason
ALLOW_UNLAUNCHED = {}
WRAPPED = ("conv2d_fwd", "conv2d_dgrad", "conv2d_wgrad", "conv2d_fwd_s2_pair", "conv2d_dgrad_s2_pair",
           "lcnn_conv1_fwd", "lcnn_conv1_wgrad")
WINO_WGRAD_RTOL = 1e-5


@pytest.fixture(scope="module")
def ops():
    from asvspoof2021_air_amd import ops
    yield ops
    # the fp64 references at B = 64 leave gigabytes in this process's allocator cache: hand them back to the device
    # before later modules start processes of their own on the same GPU
    _HARVEST.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else tuple(int(u) for u in v)


def _shape(t):
    return None if t is None else tuple(t.shape)


# ------------------------------------------------------------------------------------------------ kernels of a call
_KNAME = re.compile(r"(\w+_kernel)(<[^()]*>)?")


def kernels_of(fn):
    """(result of fn(), [device kernel names in launch order, with template arguments])."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    evs = [ev for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA]
    evs.sort(key=lambda ev: ev.time_range.start)
    names = []
    for ev in evs:
        m = _KNAME.search(ev.name)
        if m:
            names.append(m.group(1) + (m.group(2) or "").replace(" ", ""))
    return out, names


def base(name):
    return name.split("<")[0]


def targs(name):
    m = re.search(r"<([^<>]*)>", name)
    return [a.strip() for a in m.group(1).split(",")] if m else []


def conv_mts(names):
    """Pixel-tile counts (template argument MT) of the direct forward / one-pass stride-2 dgrad launches."""
    out = []
    for n in names:
        if base(n) == "conv_fwd_kernel":
            out.append(int(targs(n)[6]))
        elif base(n) == "conv_s2_dgrad_kernel":
            out.append(int(targs(n)[1]))
    return out


def source_kernels():
    ks = set()
    for f in CONV_SOURCES:
        src = open(os.path.join(CSRC, f)).read()
        ks |= set(re.findall(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s*)?void\s+(\w+_kernel)\s*\(", src))
    return ks


# ------------------------------------------------------------------------------------------------ fp64 references
@contextlib.contextmanager
def _aten_conv():
    with torch.backends.cudnn.flags(enabled=False):
        yield


def _act64(x, scale, shift):
    xa = x.double()
    if scale is not None:
        xa = F.relu(xa * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    return xa


def ref_fwd(x, w, stride, padding, scale=None, shift=None):
    with _aten_conv(), torch.no_grad():
        return F.conv2d(_act64(x, scale, shift), w.double(), None, stride, padding)


def ref_dgrad(dy, w, x_shape, stride, padding):
    with _aten_conv():
        xd = torch.zeros(x_shape, dtype=torch.float64, device=dy.device, requires_grad=True)
        y = F.conv2d(xd, w.double(), None, stride, padding)
        y.backward(dy.double())
    return xd.grad


def ref_wgrad(x, dy, w_shape, stride, padding, scale=None, shift=None):
    with _aten_conv():
        wd = torch.zeros(w_shape, dtype=torch.float64, device=x.device, requires_grad=True)
        y = F.conv2d(_act64(x, scale, shift), wd, None, stride, padding)
        y.backward(dy.double())
    return wd.grad


def close(got, want, rtol, name):
    got, want = got.detach().double(), want.detach().double().to(got.device)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(want.abs().max().item(), 1e-30)
    err = (got - want).abs().max().item() / scale
    assert err <= rtol, "%s: max err %.3g of scale %.3g (rel %.3g > %.3g)" % (name, err * scale, scale, err, rtol)
    return err


def subset(B):
    return sorted({0, B // 2, B - 1})


def is_wino(names):
    return any(base(n) in ("wino_conv_kernel", "wino4_conv_kernel") for n in names)


# ------------------------------------------------------------------------------------------------ replay of one call
def _guarded(shape, device="cuda"):
    """A view into the middle third of a buffer filled with 7: a store outside the view lands in a guard."""
    buf = torch.full((3,) + tuple(shape), 7.0, device=device)
    return buf, buf[1]


def _guards_intact(buf):
    return bool((buf[0] == 7.0).all()) and bool((buf[2] == 7.0).all())


def _weights(shape, seed):
    fan = shape[1] * shape[2] * shape[3]
    return synth_feat(shape, seed, scale=(2.0 / fan) ** 0.5).cuda()


def replay(ops, sig, check=True):
    """Run one recorded signature on synthetic data at exactly its shape and flags; return the kernels that served the
    HIP call.  check=True: hold the result to fp64 (and the flag-specific checks)."""
    s = dict(sig)
    op = s["op"]
    if op == "conv2d_fwd":
        xs, ws, st, pd = s["x"], s["w"], s["stride"], s["padding"]
        B, Cin = xs[0], xs[1]
        x = synth_feat(xs, 1).cuda()
        w = _weights(ws, 2)
        sc = sh = res = None
        if s["pro"]:
            sc = (1.0 + 0.2 * synth_feat((Cin,), 3)).cuda()
            sh = (0.3 * synth_feat((Cin,), 4)).cuda()
        d = ops._conv_desc(xs, ws, st, pd)
        yshape = (B, ws[0], d.Ho, d.Wo)
        if s["residual"]:
            res = synth_feat(yshape, 5).cuda()
        kw = dict(in_scale=sc, in_shift=sh, relu=s["relu"], residual=res)
        (y, rec), names = kernels_of(lambda: ops.conv2d_fwd(x, w, st, pd, stats=True, **kw) if s["stats"]
                                     else (ops.conv2d_fwd(x, w, st, pd, **kw), None))
        if not check:
            return names
        if s["w_packed"]:
            pk = ops.conv2d_prepack(w, xs, st, pd, 0)
            assert torch.equal(ops.conv2d_fwd(x, w, st, pd, w_packed=pk, **kw), y), "prepacked forward differs"
        idx = subset(B)
        want = ref_fwd(x[idx], w, st, pd, sc, sh)
        if res is not None:
            want = want + res[idx].double()
        close(y[idx], want, wino_conv_bound() if is_wino(names) else STRICT["conv_rtol"], "forward %s" % (sig,))
        if s["stats"]:
            assert rec is not None, "the model got fused statistics for this layer, the replay did not"
            assert torch.equal(y, ops.conv2d_fwd(x, w, st, pd, **kw))
            gamma, beta = (1.0 + 0.3 * synth_feat((ws[0],), 34)).cuda(), (0.2 * synth_feat((ws[0],), 35)).cuda()
            a = ops.bn_stats(y, gamma, beta)
            b = ops.bn_stats(y, gamma, beta, stats_in=rec)
            yd = y.double()
            close(b[0], yd.mean((0, 2, 3)), 2e-6, "epilogue mean")
            close(b[1], 1.0 / torch.sqrt(yd.var((0, 2, 3), unbiased=False) + 1e-5), 2e-6, "epilogue invstd")
            close(b[2], a[2], 2e-6, "epilogue scale")
            close(b[3], a[3], 4e-6, "epilogue shift")
        return names
    if op == "conv2d_dgrad":
        xs, ws, st, pd = s["x"], s["w"], s["stride"], s["padding"]
        B, Cin = xs[0], xs[1]
        d = ops._conv_desc(xs, ws, st, pd)
        dy = synth_feat((B, ws[0], d.Ho, d.Wo), 6).cuda()
        w = _weights(ws, 2)
        acc = synth_feat(xs, 7).cuda() if s["accumulate"] else None
        buf = out = None
        if s["out"]:
            buf, out = _guarded(xs)
        bn = None
        if s["bn"]:
            bx = (synth_feat(xs, 44) * 1.3 + 0.2).cuda()
            gamma, beta = (1.0 + 0.3 * synth_feat((Cin,), 46)).cuda(), (0.2 * synth_feat((Cin,), 47)).cuda()
            mean, invstd, _, _ = ops.bn_stats(bx, gamma, beta)
            bn = (bx, mean, invstd, gamma, beta)
        got, names = kernels_of(lambda: ops.conv2d_dgrad(dy, w, xs, st, pd, accumulate=acc, out=out, bn=bn))
        if not check:
            return names
        sums = None
        if bn is not None:
            got, sums = got
            assert sums is not None, "the model got fused BatchNorm sums for this layer, the replay did not"
        if buf is not None:
            assert _guards_intact(buf), "data gradient wrote outside its out= view"
        plain = ops.conv2d_dgrad(dy, w, xs, st, pd, accumulate=acc)
        if bn is not None:
            assert torch.equal(got, plain), "the BatchNorm sums changed the data gradient"
            dx0, dg0, db0 = ops.bn_bwd(bn[0], got, *bn[1:], relu=True)
            dx1, dg1, db1 = ops.bn_bwd(bn[0], got, *bn[1:], relu=True, sums_in=sums)
            close(dg1, dg0, 2e-6, "epilogue dgamma")
            close(db1, db0, 2e-6, "epilogue dbeta")
            close(dx1, dx0, 2e-6, "epilogue dx")
        if s["w_packed"]:
            pk = ops.conv2d_prepack(w, xs, st, pd, 1)
            assert torch.equal(ops.conv2d_dgrad(dy, w, xs, st, pd, accumulate=acc, w_packed=pk), plain), \
                "prepacked data gradient differs"
        idx = subset(B)
        want = ref_dgrad(dy[idx], w, (len(idx),) + tuple(xs[1:]), st, pd)
        if acc is not None:
            want = want + acc[idx].double()
        close(got[idx], want, wino_conv_bound() if is_wino(names) else STRICT["conv_rtol"], "dgrad %s" % (sig,))
        return names
    if op == "conv2d_wgrad":
        xs, ws, st, pd = s["x"], s["w"], s["stride"], s["padding"]
        B, Cin = xs[0], xs[1]
        d = ops._conv_desc(xs, ws, st, pd)
        x = synth_feat(xs, 1).cuda()
        dy = synth_feat((B, ws[0], d.Ho, d.Wo), 6).cuda()
        sc = sh = None
        if s["pro"]:
            sc = (1.0 + 0.2 * synth_feat((Cin,), 3)).cuda()
            sh = (0.3 * synth_feat((Cin,), 4)).cuda()
        buf = out = None
        if s["out"]:
            buf, out = _guarded(ws)
        got, names = kernels_of(lambda: ops.conv2d_wgrad(x, dy, ws, st, pd, sc, sh, relu=s["relu"], out=out))
        if not check:
            return names
        if buf is not None:
            assert _guards_intact(buf), "weight gradient wrote outside its out= view"
        want = ref_wgrad(x, dy, ws, st, pd, sc, sh)
        rtol = WINO_WGRAD_RTOL if any(base(n) == "wino_wgrad_kernel" for n in names) else STRICT["conv_rtol"]
        close(got, want, rtol, "wgrad %s" % (sig,))
        return names
    if op == "conv2d_fwd_s2_pair":
        xs, ws = s["x"], s["w"]
        B = xs[0]
        x = synth_feat(xs, 1).cuda()
        w = _weights(ws, 2)
        wsc = _weights((ws[0], ws[1], 1, 1), 3)
        (y, ysc), names = kernels_of(lambda: ops.conv2d_fwd_s2_pair(x, w, wsc))
        if not check:
            return names
        if s["packed"]:
            pk = ops.conv2d_fwd_s2_pair_prepack(w, wsc, xs)
            y2, ysc2 = ops.conv2d_fwd_s2_pair(x, w, wsc, packed=pk)
            assert torch.equal(y, y2) and torch.equal(ysc, ysc2), "prepacked pair forward differs"
        idx = subset(B)
        close(y[idx], ref_fwd(x[idx], w, 2, 1), STRICT["conv_rtol"], "pair forward 3x3 %s" % (sig,))
        close(ysc[idx], ref_fwd(x[idx], wsc, 2, 0), STRICT["conv_rtol"], "pair forward shortcut %s" % (sig,))
        return names
    if op == "conv2d_dgrad_s2_pair":
        xs, ws = s["x"], s["w"]
        B = xs[0]
        d = ops._conv_desc(xs, ws, 2, 1)
        dy = synth_feat((B, ws[0], d.Ho, d.Wo), 6).cuda()
        dysc = synth_feat((B, ws[0], d.Ho, d.Wo), 8).cuda()
        w = _weights(ws, 2)
        wsc = _weights((ws[0], ws[1], 1, 1), 3)
        acc = synth_feat(xs, 7).cuda() if s["accumulate"] else None
        buf = out = None
        if s["out"]:
            buf, out = _guarded(xs)
        got, names = kernels_of(lambda: ops.conv2d_dgrad_s2_pair(dy, w, dysc, wsc, xs, accumulate=acc, out=out))
        if not check:
            return names
        assert got is not None
        if buf is not None:
            assert _guards_intact(buf), "pair data gradient wrote outside its out= view"
        if s["packed"]:
            pk = ops.conv2d_dgrad_s2_pair_prepack(w, wsc, xs)
            assert torch.equal(ops.conv2d_dgrad_s2_pair(dy, w, dysc, wsc, xs, accumulate=acc, packed=pk), got), \
                "prepacked pair data gradient differs"
        idx = subset(B)
        sub = (len(idx),) + tuple(xs[1:])
        want = ref_dgrad(dy[idx], w, sub, 2, 1) + ref_dgrad(dysc[idx], wsc, sub, 2, 0)
        if acc is not None:
            want = want + acc[idx].double()
        close(got[idx], want, STRICT["conv_rtol"], "pair dgrad %s" % (sig,))
        return names
    if op in ("lcnn_conv1_fwd", "lcnn_conv1_wgrad"):
        import lcnn_oracle as o
        xs = s["x"]
        B = xs[0]
        x = synth_feat(xs, 31)
        w = synth_feat((64, 1, 5, 5), 33, scale=0.2)
        b = synth_feat((64,), 34, scale=0.1)
        (y, r), names_f = kernels_of(lambda: ops.lcnn_conv1_fwd(x.cuda(), w.cuda(), b.cuda()))
        dy = synth_feat(tuple(y.shape), 32).cuda()
        dw = torch.empty(64, 1, 5, 5, device="cuda")
        db = torch.empty(64, device="cuda")
        _, names_w = kernels_of(lambda: ops.lcnn_conv1_wgrad(x.cuda(), dy, r, dw, db))
        names = names_f if op == "lcnn_conv1_fwd" else names_w
        if not check:
            return names
        if op == "lcnn_conv1_fwd":
            idx = subset(B)
            pre = F.conv2d(x[idx].double(), w.double(), b.double(), padding=2)
            want = F.max_pool2d(o.mfm(pre), 2, 2)
            close(y[idx], want, STRICT["conv_rtol"], "lcnn conv1 forward")
            flips = int((r[idx].cpu() != o.routes_of(pre, True)).sum())
            assert flips <= 1e-4 * r[idx].numel(), flips
        else:
            w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
            pre = F.conv2d(x.double(), w64, b64, padding=2)
            (o.route_select(pre, r.cpu(), True) * dy.cpu().double()).sum().backward()
            close(dw, w64.grad, STRICT["conv_rtol"], "lcnn conv1 weight gradient")
            close(db, b64.grad, STRICT["conv_rtol"], "lcnn conv1 bias gradient")
        return names
    raise AssertionError(op)


# ------------------------------------------------------------------------------------------------ harvest
def _sig(name, a):
    """Signature of one recorded call: its geometry and every flag that can change the route or the epilogue."""
    t = _shape
    if name in ("conv2d_fwd", "conv2d_dgrad", "conv2d_wgrad"):
        xs = tuple(a["x_shape"]) if name == "conv2d_dgrad" else t(a["x"])
        ws = tuple(a["w_shape"]) if name == "conv2d_wgrad" else t(a["w"])
        s = {"op": name, "x": xs, "w": ws, "stride": _pair(a["stride"]), "padding": _pair(a["padding"])}
        if name != "conv2d_dgrad":
            s.update(pro=a["in_scale"] is not None, relu=bool(a["relu"]))
        if name == "conv2d_fwd":
            s.update(residual=a["residual"] is not None, w_packed=a["w_packed"] is not None, stats=bool(a["stats"]))
        if name == "conv2d_dgrad":
            s.update(accumulate=a["accumulate"] is not None, w_packed=a["w_packed"] is not None,
                     bn=a["bn"] is not None, out=a["out"] is not None)
        if name == "conv2d_wgrad":
            s.update(out=a["out"] is not None)
    elif name == "conv2d_fwd_s2_pair":
        s = {"op": name, "x": t(a["x"]), "w": t(a["w"]), "packed": a["packed"] is not None}
    elif name == "conv2d_dgrad_s2_pair":
        s = {"op": name, "x": tuple(a["x_shape"]), "w": t(a["w"]), "accumulate": a["accumulate"] is not None,
             "out": a["out"] is not None, "packed": a["packed"] is not None}
    else:
        s = {"op": name, "x": t(a["x"])}
    return tuple(sorted(s.items()))


@contextlib.contextmanager
def recording(ops):
    """Wrap the ops entry points the models call; yields the list of signatures, in call order."""
    seen = []
    with pytest.MonkeyPatch.context() as mp:
        for name in WRAPPED:
            orig = getattr(ops, name)
            sig = inspect.signature(orig)

            def wrapper(*args, _orig=orig, _bind=sig.bind, _name=name, **kw):
                b = _bind(*args, **kw)
                b.apply_defaults()
                seen.append(_sig(_name, b.arguments))
                return _orig(*args, **kw)
            mp.setattr(ops, name, wrapper)
        yield seen


def _resnet_trainer():
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.resnet import ResNet
    from asvspoof2021_air_amd.train import Trainer
    m = fill_module_(ResNet(3, 256, resnet_type="18", nclasses=2))
    m.set_attention_noise(None)
    return Trainer(m, loss_module=fill_module_(AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)), feat_len=750)


def _lcnn_trainer():
    from asvspoof2021_air_amd.lcnn import LCNN
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.train import Trainer
    m = fill_module_(LCNN(60, 256)).cuda()
    return Trainer(m, loss_module=fill_module_(AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)), feat_len=750)


_HARVEST = {}


def harvest(ops, model):
    """Distinct convolution signatures of one eager train step at B = 64, 4 s, feat_len 750, default options."""
    if model not in _HARVEST:
        tr = _resnet_trainer() if model == "resnet" else _lcnn_trainer()
        assert not tr.use_graph
        B = 64
        pcm = synth_pcm(B, 64000, seed=9).cuda()
        labels = (torch.arange(B) % 2).cuda()
        with recording(ops) as seen:
            loss, _ = tr.step(pcm, labels)
            torch.cuda.synchronize()
        assert np.isfinite(loss.item())
        sigs = list(dict.fromkeys(seen))
        for name in WRAPPED:
            assert getattr(ops, name).__name__ == name, "wrapper left behind"
        _HARVEST[model] = sigs
    return _HARVEST[model]


def _fmt(sig):
    s = dict(sig)
    flags = [k for k, v in s.items() if v is True]
    geo = "x%s w%s" % (s["x"], s.get("w", ""))
    if "stride" in s:
        geo += " s%s p%s" % (s["stride"], s["padding"])
    return "%-20s %s %s" % (s["op"], geo, ",".join(flags))


def _route(names):
    ks = [n for n in names if base(n) not in ("pack_weights_kernel",)]
    return {"kernels": ks, "mt": conv_mts(names), "reduce": any(base(n) == "reduce_partials_kernel" for n in names)}


@pytest.mark.parametrize("model", ["resnet", "lcnn"])
def test_model_convolutions_at_training_batch_vs_fp64(ops, model):
    """Every distinct convolution call of one B = 64 train step, replayed alone at its shape and flags against fp64,
    with the route table (signature -> kernels) printed and recorded."""
    sigs = harvest(ops, model)
    ops_seen = {dict(s)["op"] for s in sigs}
    want_ops = {"conv2d_fwd", "conv2d_dgrad", "conv2d_wgrad"}
    want_ops |= {"conv2d_fwd_s2_pair", "conv2d_dgrad_s2_pair"} if model == "resnet" else {"lcnn_conv1_fwd",
                                                                                           "lcnn_conv1_wgrad"}
    assert want_ops <= ops_seen, (want_ops - ops_seen)
    assert all(dict(s)["x"][0] == 64 for s in sigs)
    table = []
    print("\nroute table, %s at B = 64:" % model)
    for sig in sigs:
        names = replay(ops, sig)
        r = _route(names)
        table.append({"sig": _fmt(sig), **r})
        print("  %s -> %s%s" % (_fmt(sig), " ".join(r["kernels"]), "  mt=%s" % r["mt"] if r["mt"] else ""))
    record("conv_routes_%s_b64" % model, table)


# ------------------------------------------------------------------------------------------------ boundary cases
def _c(op, x, w, stride=1, padding=0, **flags):
    s = {"op": op, "x": tuple(x), "w": tuple(w), "stride": _pair(stride), "padding": _pair(padding)}
    if op != "conv2d_dgrad":
        s.update(pro=False, relu=False)
    if op == "conv2d_fwd":
        s.update(residual=False, w_packed=False, stats=False)
    if op == "conv2d_dgrad":
        s.update(accumulate=False, w_packed=False, bn=False, out=False)
    if op == "conv2d_wgrad":
        s.update(out=False)
    s.update(flags)
    return tuple(sorted(s.items()))


def _pair_c(op, x, w, **flags):
    s = {"op": op, "x": tuple(x), "w": tuple(w), "packed": False}
    if op == "conv2d_dgrad_s2_pair":
        s.update(accumulate=False, out=False)
    s.update(flags)
    return tuple(sorted(s.items()))


C5 = (256, 512, 3, 3)  # the ResNet's conv5: (num_nodes = 3, 3) taps over the whole height, padding (0, 1)
# Why each case sits where it does, by the predicates of conv2d.hip (the route asserts below are what pins them; the
# arithmetic is here so that a reader can redo it when the heuristics change):
# * fwd_ksplit: pixel tiles = B Ho ceil(Wo / 32), workgroups = ceil(tiles / 4) ceil(Cout / (32 mt)), K slices =
#   min(4, 1536 / workgroups) while >= 8 chunks of 8 channels remain per slice.  conv5 at B = 64: W = 188 -> 384 tiles,
#   mt 1, 768 workgroups, 2 slices; W = 400 -> 832 tiles, mt 2, 832 workgroups, 1 slice.
# * pick_mt: 64-channel tiles (mt 2) unless the 768-slot round of 32-channel tiles is > 8 % fuller than the 512-slot
#   round of 64-channel ones: conv5 at W = 47 is mt 2 at B = 8 (16 workgroups), mt 1 at B = 64 (256).
# * skinny_wgrad_chunks: 512 / B chunks per utterance - B = 300 gives one; skinny3_wgrad_parts: min(B H, 256) -
#   1152 at B = 64 (capped), 72 at B = 4; generic 1x1 at (2, 64, 2, 64): 8 pixel tiles < 256 workgroups, nsplit = 8.
# * conv1's row-staged weight gradient stages (16 ceil4(Wo) + 9 (ceil4(W + 2) + 4)) floats: 150,288 bytes at W = 1500,
#   160,288 at W = 1600, either side of the 150 KB limit.
# (id, signature, options, has kernels, lacks kernels, mt of every direct launch (None: not checked), reduce follows)
CASES = [
    # K split of the plain forward around its workgroup limit: 768 workgroups split in two, 832 not
    ("ksplit_on", _c("conv2d_fwd", (64, 512, 3, 188), C5, 1, (0, 1)), {}, ["conv_fwd_kernel"], [], [1], True),
    ("ksplit_off", _c("conv2d_fwd", (64, 512, 3, 400), C5, 1, (0, 1)), {}, ["conv_fwd_kernel"],
     ["reduce_partials_kernel"], [2], False),
    # pixel-tile count: 64-channel tiles at a small batch, 32-channel ones at the training batch, and forced either way
    ("mt2", _c("conv2d_fwd", (8, 512, 3, 47), C5, 1, (0, 1)), {}, ["conv_fwd_kernel"], [], [2], True),
    ("mt1", _c("conv2d_fwd", (64, 512, 3, 47), C5, 1, (0, 1)), {}, ["conv_fwd_kernel"], [], [1], True),
    ("mt_forced1", _c("conv2d_fwd", (8, 512, 3, 47), C5, 1, (0, 1), residual=True), {"CONV_MT": 1},
     ["conv_fwd_kernel"], [], [1], False),
    ("mt_forced2", _c("conv2d_fwd", (64, 512, 3, 47), C5, 1, (0, 1), residual=True), {"CONV_MT": 2},
     ["conv_fwd_kernel"], [], [2], False),
    ("mt_forced1_1x1", _c("conv2d_fwd", (16, 128, 9, 94), (256, 128, 1, 1), 1, 0, pro=True, relu=True), {"CONV_MT": 1},
     ["conv_fwd_kernel"], [], [1], False),
    ("mt_forced2_1x1", _c("conv2d_fwd", (16, 128, 9, 94), (256, 128, 1, 1), 1, 0, pro=True, relu=True), {"CONV_MT": 2},
     ["conv_fwd_kernel"], [], [2], False),
    # Winograd F(2x2) below W = 4, F(4x4 | 3x4) from W = 4
    ("wino2_w3", _c("conv2d_fwd", (4, 64, 6, 3), (64, 64, 3, 3), 1, 1), {}, ["wino_conv_kernel"], ["wino4_conv_kernel"],
     None, False),
    ("wino4_w4", _c("conv2d_fwd", (4, 64, 6, 4), (64, 64, 3, 3), 1, 1), {}, ["wino4_conv_kernel"], ["wino_conv_kernel"],
     None, False),
    ("wino2_w3_dgrad", _c("conv2d_dgrad", (4, 64, 6, 3), (64, 64, 3, 3), 1, 1, accumulate=True), {},
     ["wino_conv_kernel"], ["wino4_conv_kernel"], None, False),
    ("wino4_w4_dgrad", _c("conv2d_dgrad", (4, 64, 6, 4), (64, 64, 3, 3), 1, 1, accumulate=True), {},
     ["wino4_conv_kernel"], ["wino_conv_kernel"], None, False),
    # weight gradients
    ("wino_wgrad", _c("conv2d_wgrad", (6, 64, 9, 40), (128, 64, 3, 3), 1, 1), {}, ["wino_wgrad_kernel"], [], None,
     True),
    ("wino_pad_wgrad_cin48", _c("conv2d_wgrad", (8, 48, 15, 94), (128, 48, 3, 3), 1, 1), {},
     ["copy_rows_kernel", "wino_wgrad_kernel"], [], None, True),
    ("wino_pad_wgrad_cin32", _c("conv2d_wgrad", (8, 32, 15, 94), (64, 32, 3, 3), 1, 1, out=True), {},
     ["copy_rows_kernel", "wino_wgrad_kernel"], [], None, True),
    ("skinny1x1_one_chunk", _c("conv2d_wgrad", (300, 16, 2, 64), (64, 16, 1, 1)), {}, ["conv_wgrad_1x1_skinny_kernel"],
     ["conv_wgrad_kernel"], None, True),
    ("skinny1x1_b64", _c("conv2d_wgrad", (64, 16, 18, 750), (64, 16, 1, 1), pro=True, relu=True), {},
     ["conv_wgrad_1x1_skinny_kernel"], ["conv_wgrad_kernel"], None, True),
    ("skinny1x1_ragged_hw", _c("conv2d_wgrad", (2, 16, 5, 75), (64, 16, 1, 1)), {}, ["conv_wgrad_kernel"],
     ["conv_wgrad_1x1_skinny_kernel"], None, True),
    ("skinny3_256_parts", _c("conv2d_wgrad", (64, 16, 18, 40), (64, 16, 3, 3), 1, 1), {},
     ["conv_wgrad_3x3_skinny_kernel"], ["wino_wgrad_kernel"], None, True),
    ("skinny3_few_parts", _c("conv2d_wgrad", (4, 16, 18, 40), (64, 16, 3, 3), 1, 1, pro=True, relu=True), {},
     ["conv_wgrad_3x3_skinny_kernel"], [], None, True),
    ("generic_wgrad_nsplit_eq_ntiles", _c("conv2d_wgrad", (2, 64, 2, 64), (64, 64, 1, 1)), {}, ["conv_wgrad_kernel"],
     [], None, True),
    ("generic_wgrad_s2_1x1", _c("conv2d_wgrad", (64, 256, 5, 188), (512, 256, 1, 1), 2, 0, pro=True, relu=True), {},
     ["conv_wgrad_kernel"], [], None, True),
    ("generic_wgrad_s2_3x3_pro", _c("conv2d_wgrad", (8, 64, 9, 75), (128, 64, 3, 3), 2, 1, pro=True, relu=True), {},
     ["conv_wgrad_kernel"], ["conv_s2w_bf3_kernel"], None, True),
    ("bf3_wgrad_s2", _c("conv2d_wgrad", (8, 64, 9, 75), (128, 64, 3, 3), 2, 1), {}, ["conv_s2w_bf3_kernel"],
     ["conv_wgrad_kernel"], None, True),
    # stride-2 forward / data gradient
    ("bf3_fwd_s2", _c("conv2d_fwd", (8, 64, 9, 75), (128, 64, 3, 3), 2, 1, w_packed=True), {},
     ["conv_s2_bf3_kernel"], ["conv_fwd_kernel"], None, False),
    ("direct_fwd_s2_pro", _c("conv2d_fwd", (8, 64, 9, 75), (128, 64, 3, 3), 2, 1, pro=True, relu=True), {},
     ["conv_fwd_kernel"], [], [2], False),
    ("pair_fwd_s2", _pair_c("conv2d_fwd_s2_pair", (8, 64, 18, 75), (128, 64, 3, 3), packed=True), {},
     ["conv_s2_bf3_kernel"], [], None, False),
    ("pair_dgrad_s2_bf3", _pair_c("conv2d_dgrad_s2_pair", (8, 64, 18, 75), (128, 64, 3, 3), accumulate=True,
                                  packed=True), {}, ["conv_s2d_bf3_kernel"], [], None, False),
    ("pair_dgrad_s2_f32", _pair_c("conv2d_dgrad_s2_pair", (8, 64, 18, 75), (128, 64, 3, 3), accumulate=True),
     {"CONV_S2": 7}, ["conv_s2_dgrad_kernel"], ["conv_s2d_bf3_kernel"], None, False),
    ("lone_dgrad_s2", _c("conv2d_dgrad", (8, 64, 9, 75), (128, 64, 3, 3), 2, 1, accumulate=True), {},
     ["conv_s2_dgrad_kernel"], [], None, False),
    ("parity_class_dgrad_s2", _c("conv2d_dgrad", (8, 64, 9, 75), (128, 64, 3, 3), 2, 1), {"CONV_S2": 0},
     ["conv_fwd_kernel"], ["conv_s2_dgrad_kernel"], None, False),
    ("dgrad_s2_1x1", _c("conv2d_dgrad", (8, 64, 9, 75), (128, 64, 1, 1), 2, 0, accumulate=True), {},
     ["conv_fwd_kernel"], [], None, False),
    # conv5's data gradient: one 1 x 3 row convolution per kernel row
    ("conv5_row_dgrad", _c("conv2d_dgrad", (64, 512, 3, 94), C5, 1, (0, 1), w_packed=True), {},
     ["conv_fwd_kernel<1,3,1,0,16,1"], ["reduce_partials_kernel"], None, False),
    # ResNet conv1 (1 -> 16, 9x3, stride (3, 1)): the row-staged weight gradient until its LDS staging passes 150 KB
    ("conv1_fwd", _c("conv2d_fwd", (8, 1, 60, 750), (16, 1, 9, 3), (3, 1), (1, 1)), {}, ["conv_direct_fwd_kernel"], [],
     None, False),
    ("conv1_wgrad_rows_w1500", _c("conv2d_wgrad", (4, 1, 60, 1500), (16, 1, 9, 3), (3, 1), (1, 1)), {},
     ["conv_direct_wgrad_rows_kernel"], ["conv_direct_wgrad_kernel"], None, True),
    ("conv1_wgrad_w1600", _c("conv2d_wgrad", (4, 1, 60, 1600), (16, 1, 9, 3), (3, 1), (1, 1)), {},
     ["conv_direct_wgrad_kernel"], ["conv_direct_wgrad_rows_kernel"], None, True),
    # LCNN conv1 (fused 5x5 + bias + MFM + pool) at the training batch
    ("lcnn_conv1_fwd", (("op", "lcnn_conv1_fwd"), ("x", (64, 1, 60, 750))), {}, [], [], None, None),
    ("lcnn_conv1_wgrad", (("op", "lcnn_conv1_wgrad"), ("x", (64, 1, 60, 750))), {}, [], [], None, None),
]


def _has(names, k):
    return any(n.startswith(k) for n in names)


def check_route(names, has, lacks, mts, reduce):
    assert names, "no device kernel seen"
    for k in has:
        assert _has(names, k), (k, names)
    for k in lacks:
        assert not _has(names, k), (k, names)
    if mts is not None:
        got = conv_mts(names)
        assert got and set(got) == set(mts), (mts, names)
    if reduce is not None:
        assert _has(names, "reduce_partials_kernel") == reduce, (reduce, names)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_boundary_route_vs_fp64(ops, case):
    """One route per case: the kernels that served the call, the pixel-tile count, the K-split / split-K reduction,
    and the result against fp64."""
    from asvspoof2021_air_amd import _hip
    cid, sig, opts, has, lacks, mts, reduce = case
    with _hip.options(**opts):
        names = replay(ops, sig)
    record("conv_route_case", {"case": cid, **_route(names)})
    check_route(names, has, lacks, mts, reduce)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("k,cout", [(3, 64), (3, 192), (1, 64), (1, 192)])
def test_stride2_weight_gradient_without_an_instance_is_refused(ops, k, cout):
    """Stride 2 with Cout % 128 != 0: the split-K kernel has 32-channel-tile instances only for stride 2 and the
    split-bf16 kernel needs Cout % 128 == 0 - the call must fail loudly, never hand back numbers (the forward and data
    gradient of the same layer are served)."""
    from asvspoof2021_air_amd import _hip
    x = synth_feat((2, 64, 9, 40), 1).cuda()
    w = _weights((cout, 64, k, k), 2)
    p = 1 if k == 3 else 0
    y = ops.conv2d_fwd(x, w, 2, p)
    dy = torch.ones_like(y)
    assert torch.isfinite(ops.conv2d_dgrad(dy, w, x.shape, 2, p)).all()
    out = torch.full(tuple(w.shape), 7.0, device="cuda")
    with pytest.raises(_hip.AirError):
        ops.conv2d_wgrad(x, dy, tuple(w.shape), 2, p, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------ options
BIG = 1 << 20

OPTION_CASES = [
    # WGRAD_WGS: one split, a ragged last split (70 pixel tiles in 3), splits left empty (70 in 32 of 3), the default
    # (one tile each) and far more than there are pixel tiles
    *[("WGRAD_WGS=%d" % v, _c("conv2d_wgrad", (5, 64, 7, 64), (64, 64, 1, 1)), {"WGRAD_WGS": v},
       ["conv_wgrad_kernel"], [], True) for v in (1, 3, 32, 256, BIG)],
    *[("WGRAD_WGS=%d s2" % v, _c("conv2d_wgrad", (5, 64, 13, 75), (128, 64, 3, 3), 2, 1, pro=True, relu=True),
       {"WGRAD_WGS": v}, ["conv_wgrad_kernel"], [], True) for v in (1, 6, 64, 256, BIG)],
    # WINO_WGRAD_WGS: the same over the Winograd weight gradient's 70 row segments, plain and on the zero-padded x
    *[("WINO_WGRAD_WGS=%d" % v, _c("conv2d_wgrad", (7, 64, 9, 40), (64, 64, 3, 3), 1, 1), {"WINO_WGRAD_WGS": v},
       ["wino_wgrad_kernel"], [], True) for v in (1, 3, 32, 256, BIG)],
    *[("WINO_WGRAD_WGS=%d pad" % v, _c("conv2d_wgrad", (7, 48, 15, 40), (64, 48, 3, 3), 1, 1), {"WINO_WGRAD_WGS": v},
       ["copy_rows_kernel", "wino_wgrad_kernel"], [], True) for v in (1, 3, 256, BIG)],
    ("DIRECT_WGRAD_ROWS=0", _c("conv2d_wgrad", (8, 1, 60, 750), (16, 1, 9, 3), (3, 1), (1, 1)),
     {"DIRECT_WGRAD_ROWS": 0}, ["conv_direct_wgrad_kernel"], ["conv_direct_wgrad_rows_kernel"], True),
    ("SKINNY_WGRAD=0 1x1", _c("conv2d_wgrad", (64, 16, 18, 76), (64, 16, 1, 1), pro=True, relu=True),
     {"SKINNY_WGRAD": 0}, ["conv_wgrad_kernel"], ["conv_wgrad_1x1_skinny_kernel"], True),
    ("SKINNY_WGRAD=0 3x3", _c("conv2d_wgrad", (8, 16, 18, 76), (64, 16, 3, 3), 1, 1), {"SKINNY_WGRAD": 0},
     ["wino_wgrad_kernel", "copy_rows_kernel"], ["conv_wgrad_3x3_skinny_kernel"], True),
    ("SKINNY_WGRAD=0 3x3 pro", _c("conv2d_wgrad", (8, 16, 18, 76), (64, 16, 3, 3), 1, 1, pro=True, relu=True),
     {"SKINNY_WGRAD": 0}, ["conv_wgrad_kernel"], ["conv_wgrad_3x3_skinny_kernel"], True),
    # WINO4_DEPHASE is a run-time argument of the same wino4_conv_kernel (a start delay), not another kernel: the
    # profiler can only show that kernel ran, not that the delay took effect - what these cases hold is the fp64 bound
    ("WINO4_DEPHASE=1", _c("conv2d_fwd", (64, 64, 18, 750), (64, 64, 3, 3), 1, 1, residual=True), {"WINO4_DEPHASE": 1},
     ["wino4_conv_kernel"], [], None),
    ("WINO4_DEPHASE=1 dgrad", _c("conv2d_dgrad", (16, 128, 9, 375), (128, 128, 3, 3), 1, 1, accumulate=True),
     {"WINO4_DEPHASE": 1}, ["wino4_conv_kernel"], [], None),
]


@pytest.mark.parametrize("case", OPTION_CASES, ids=[c[0] for c in OPTION_CASES])
def test_dispatch_option_holds_its_kernels_bound(ops, case):
    """include/air_hip.h: options "never change results beyond the documented rounding of the kernel they select" -
    each value at a shape where it changes the launch, against fp64, with the kernel it selects seen to run."""
    from asvspoof2021_air_amd import _hip
    cid, sig, opts, has, lacks, reduce = case
    with _hip.options(**opts):
        names = replay(ops, sig)
    check_route(names, has, lacks, None, reduce)


# ------------------------------------------------------------------------------------------------ workspace
AIR_EWORKSPACE = -4
W64, W128S2 = (64, 64, 3, 3), (128, 64, 3, 3)
X_S2 = (2, 64, 9, 12)
# One small descriptor per route, called through the C entry point on a workspace of exactly air_conv2d_ws_bytes(p)
# bytes.  need: the floats the route itself checks for (csrc/conv2d.hip, fwd_route / dgrad_route / wgrad_route), written
# out from the launch's own layout:
# * Winograd transforms: Cout Cin 16 floats for F(2x2), Cout Cin 36 + 1024 for F(4x4); split-bf16 planes: 6 bytes a weight
# * K-split forward, (64, 512, 1, 1) on 2 x 2 x 32 pixels: one workgroup, 16 chunks of 32 channels -> 2 slices; the slab
#   and two copies of y
# * data gradient slabs: Cin (to 64) x Cout (to 32) x taps
# * weight gradients: partials x Cout Cin taps - 6 Winograd segments (2 x 3 tile rows x 1); 2 split-bf16 segments (10 rows
#   in steps of 8); 10 and 8 split-K pixel tiles; min(B H, 256) = 8 skinny 3x3 rows; 2 x 1 skinny 1x1 chunks; B Ho = 4
#   rows of conv1; on zero-padded x the 2 x 64 x 48 copy of x, 6 partials and the 64-channel dW
# (id, op, x, w, stride, padding, flags, options, has kernels, lacks kernels, need in floats)
WS_CASES = [
    ("wino2_fwd", "fwd", (2, 64, 6, 3), W64, 1, 1, {"residual": True}, {}, ["wino_conv_kernel"], ["wino4_conv_kernel"],
     64 * 64 * 16),
    ("wino2_dgrad", "dgrad", (2, 64, 6, 3), W64, 1, 1, {}, {}, ["wino_conv_kernel"], ["wino4_conv_kernel"], 64 * 64 * 16),
    ("wino4_fwd", "fwd", (2, 64, 6, 4), W64, 1, 1, {}, {}, ["wino4_conv_kernel"], ["wino_conv_kernel"],
     64 * 64 * 36 + 1024),
    ("wino4_dgrad", "dgrad", (2, 64, 6, 4), W64, 1, 1, {"accumulate": True}, {}, ["wino4_conv_kernel"],
     ["wino_conv_kernel"], 64 * 64 * 36 + 1024),
    ("ksplit_fwd", "fwd", (2, 512, 2, 32), (64, 512, 1, 1), 1, 0, {}, {}, ["conv_fwd_kernel", "reduce_partials_kernel"],
     [], 64 * 512 + 2 * (2 * 64 * 2 * 32)),
    ("bf3_fwd_s2", "fwd", X_S2, W128S2, 2, 1, {}, {}, ["conv_s2_bf3_kernel"], ["conv_fwd_kernel"], 128 * 64 * 9 * 6 // 4),
    ("bf3_wgrad_s2", "wgrad", X_S2, W128S2, 2, 1, {}, {}, ["conv_s2w_bf3_kernel", "reduce_partials_kernel"],
     ["conv_wgrad_kernel"], 2 * 128 * 64 * 9),
    ("splitk_wgrad_s2_pro", "wgrad", X_S2, W128S2, 2, 1, {"pro": True}, {}, ["conv_wgrad_kernel", "reduce_partials_kernel"],
     ["conv_s2w_bf3_kernel"], 10 * 128 * 64 * 9),
    ("lone_dgrad_s2", "dgrad", X_S2, W128S2, 2, 1, {"accumulate": True}, {}, ["conv_s2_dgrad_kernel"], [], 64 * 128 * 9),
    ("parity_class_dgrad_s2", "dgrad", X_S2, W128S2, 2, 1, {}, {"CONV_S2": 0}, ["conv_fwd_kernel"],
     ["conv_s2_dgrad_kernel"], 64 * 128 * 9),
    ("wino_wgrad", "wgrad", (2, 64, 6, 8), W64, 1, 1, {}, {}, ["wino_wgrad_kernel", "reduce_partials_kernel"], [],
     6 * 64 * 64 * 9),
    ("wino_pad_wgrad", "wgrad", (2, 48, 6, 8), (64, 48, 3, 3), 1, 1, {}, {},
     ["copy_rows_kernel", "wino_wgrad_kernel", "reduce_partials_kernel"], [], 2 * 64 * 48 + (6 + 1) * 64 * 64 * 9),
    ("skinny3_wgrad", "wgrad", (2, 16, 4, 8), (64, 16, 3, 3), 1, 1, {"pro": True}, {},
     ["conv_wgrad_3x3_skinny_kernel", "reduce_partials_kernel"], [], 8 * 64 * 16 * 9),
    ("skinny1_wgrad", "wgrad", (2, 16, 2, 64), (64, 16, 1, 1), 1, 0, {}, {},
     ["conv_wgrad_1x1_skinny_kernel", "reduce_partials_kernel"], ["conv_wgrad_kernel"], 2 * 64 * 16),
    ("splitk_wgrad_nsplit_eq_ntiles", "wgrad", (2, 64, 2, 64), (64, 64, 1, 1), 1, 0, {}, {},
     ["conv_wgrad_kernel", "reduce_partials_kernel"], [], 8 * 64 * 64),
    ("direct_fwd", "fwd", (2, 1, 12, 16), (16, 1, 9, 3), (3, 1), (1, 1), {}, {}, ["conv_direct_fwd_kernel"], [], 0),
    ("direct_wgrad", "wgrad", (2, 1, 12, 16), (16, 1, 9, 3), (3, 1), (1, 1), {}, {},
     ["conv_direct_wgrad_rows_kernel", "reduce_partials_kernel"], [], 4 * 16 * 27),
    ("conv5_row_dgrad", "dgrad", (2, 64, 3, 16), W64, 1, (0, 1), {}, {}, ["conv_fwd_kernel<1,3,1,0,16,1"],
     ["reduce_partials_kernel"], 64 * 64 * 9),
]
SENTINEL = 0xA5


@pytest.mark.parametrize("case", WS_CASES, ids=[c[0] for c in WS_CASES])
def test_route_stays_inside_the_declared_workspace(ops, case):
    """Every route on a workspace of exactly air_conv2d_ws_bytes(p) bytes cut from the middle of a sentinel-filled
    buffer: the route's kernels run, the result holds the route's bound against fp64, no byte outside the slice
    changes, and one byte less than the route's own need is refused before anything is written."""
    import ctypes
    from asvspoof2021_air_amd import _hip
    from asvspoof2021_air_amd._hip import ci, csz, dptr, stream
    cid, op, xs, wshape, st, pd, flags, opts, has, lacks, need = case
    lib = _hip.lib()
    d = ops._conv_desc(xs, wshape, st, pd)
    B, Cin = xs[0], xs[1]
    yshape = (B, wshape[0], d.Ho, d.Wo)
    x, w, dy = synth_feat(xs, 1).cuda(), _weights(wshape, 2), synth_feat(yshape, 6).cuda()
    sc = sh = extra = None
    if flags.get("pro"):
        sc, sh = (1.0 + 0.2 * synth_feat((Cin,), 3)).cuda(), (0.3 * synth_feat((Cin,), 4)).cuda()
    if flags.get("residual") or flags.get("accumulate"):
        extra = synth_feat(yshape if op == "fwd" else xs, 5).cuda()
    null = ctypes.c_void_p(0)
    oshape = {"fwd": yshape, "dgrad": tuple(xs), "wgrad": tuple(wshape)}[op]

    def call(out, ws, nbytes):
        wsp = ctypes.c_void_p(ws.data_ptr())
        if op == "fwd":
            return lib.air_conv2d_fwd_pre(ctypes.byref(d), dptr(x), dptr(w), null, dptr(out), dptr(sc, allow_none=True),
                                          dptr(sh, allow_none=True), ci(1 if sc is not None else 0),
                                          dptr(extra, allow_none=True), null, wsp, csz(nbytes), stream())
        if op == "dgrad":
            return lib.air_conv2d_dgrad_pre(ctypes.byref(d), dptr(dy), dptr(w), null, dptr(out),
                                            dptr(extra, allow_none=True), wsp, csz(nbytes), stream())
        return lib.air_conv2d_wgrad(ctypes.byref(d), dptr(x), dptr(dy), dptr(out), dptr(sc, allow_none=True),
                                    dptr(sh, allow_none=True), ci(1 if sc is not None else 0), wsp, csz(nbytes), stream())

    with _hip.options(**opts):
        n = int(lib.air_conv2d_ws_bytes(ctypes.byref(d)))
        assert n >= 4 * need + 256, (n, need)
        guard = (n + 65535) // 65536 * 65536  # an overrun of up to the whole size again lands in the sentinel
        buf = torch.full((guard + n + guard,), SENTINEL, dtype=torch.uint8, device="cuda")
        ws = buf[guard:guard + n]
        out = torch.full(oshape, 7.0, device="cuda")
        rc, names = kernels_of(lambda: call(out, ws, n))
        assert rc == 0, rc
        check_route(names, has, lacks, None, None)
        assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + n:] == SENTINEL).all()), \
            "the route wrote outside air_conv2d_ws_bytes(p)"
        if need > 0:
            small = torch.full(oshape, 7.0, device="cuda")
            assert call(small, ws, 4 * need - 1) == AIR_EWORKSPACE
            torch.cuda.synchronize()
            assert bool((small == 7.0).all()), "a refused call wrote its output"
    if op == "fwd":
        want = ref_fwd(x, w, st, pd, sc, sh)
    elif op == "dgrad":
        want = ref_dgrad(dy, w, tuple(xs), st, pd)
    else:
        want = ref_wgrad(x, dy, wshape, st, pd, sc, sh)
    if extra is not None:
        want = want + extra.double()
    if any(base(k) == "wino_wgrad_kernel" for k in names):
        rtol = WINO_WGRAD_RTOL
    else:
        rtol = wino_conv_bound() if is_wino(names) else STRICT["conv_rtol"]
    close(out, want, rtol, "%s on an exact workspace" % cid)


# ------------------------------------------------------------------------------------------------ coverage
def test_fp64_reference_on_gpu_matches_cpu():
    """The GPU fp64 references (ATen's own convolution) agree with CPU fp64 at a small shape, stride 1 and 2."""
    for (xs, ws, st, pd) in (((3, 16, 9, 20), (32, 16, 3, 3), 1, 1), ((3, 16, 9, 21), (32, 16, 3, 3), 2, 1),
                             ((2, 8, 7, 11), (16, 8, 1, 1), 2, 0), ((2, 4, 3, 10), (8, 4, 3, 3), 1, (0, 1))):
        x = synth_feat(xs, 1).double()
        w = synth_feat(ws, 2).double()
        y = F.conv2d(x, w, None, st, pd)
        dy = synth_feat(tuple(y.shape), 3).double()
        xr = x.clone().requires_grad_(True)
        wr = w.clone().requires_grad_(True)
        F.conv2d(xr, wr, None, st, pd).backward(dy)
        for got, want in ((ref_fwd(x.cuda(), w.cuda(), st, pd), y),
                          (ref_dgrad(dy.cuda(), w.cuda(), xs, st, pd), xr.grad),
                          (ref_wgrad(x.cuda(), dy.cuda(), ws, st, pd), wr.grad)):
            assert got.dtype == torch.float64
            close(got, want, 1e-12, "fp64 GPU vs CPU %s" % (xs,))


def test_every_conv_kernel_is_launched_by_some_case(ops):
    """Every __global__ *_kernel of the four convolution sources runs in some case (HIP calls only, no references)."""
    from asvspoof2021_air_amd import _hip
    seen = set()
    for _, sig, opts, *_rest in CASES + OPTION_CASES:
        with _hip.options(**opts):
            seen |= {base(n) for n in replay(ops, sig, check=False)}
    # the weight transforms run ahead of time (air_conv2d_prepack*), one by one and batched
    jobs = [((4, 64, 6, 75), (64, 64, 3, 3), 1, 1, {}), ((4, 64, 6, 3), (64, 64, 3, 3), 1, 1, {}),
            ((4, 64, 9, 75), (128, 64, 3, 3), 2, 1, {}), ((4, 64, 9, 75), (128, 64, 1, 1), 2, 0, {})]

    def prepack_all():
        for xs, ws, st, pd, _ in jobs:
            w = _weights(ws, 5)
            for which in (0, 1):
                ops.conv2d_prepack(w, xs, st, pd, which)
        w3, wsc = _weights((128, 64, 3, 3), 6), _weights((128, 64, 1, 1), 7)
        ops.conv2d_fwd_s2_pair_prepack(w3, wsc, (4, 64, 18, 75))
        ops.conv2d_dgrad_s2_pair_prepack(w3, wsc, (4, 64, 18, 75))
        with ops.prepack_batch():
            for xs, ws, st, pd, _ in jobs:
                w = _weights(ws, 8)
                for which in (0, 1):
                    ops.conv2d_prepack(w, xs, st, pd, which)
    _, names = kernels_of(prepack_all)
    seen |= {base(n) for n in names}
    kernels = source_kernels()
    assert len(kernels) >= 20 and "conv_fwd_kernel" in kernels, kernels
    assert set(ALLOW_UNLAUNCHED) <= kernels, "allow-list names a kernel that no longer exists"
    missing = kernels - seen - set(ALLOW_UNLAUNCHED)
    assert not missing, sorted(missing)
    launched_anyway = set(ALLOW_UNLAUNCHED) & seen
    assert not launched_anyway, launched_anyway
