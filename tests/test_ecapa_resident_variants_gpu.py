"""GPU: ``Res2Net2(context=False / summed=True)`` on the bf16-RESIDENT path (``set_compute_dtype("bf16", variants=True)``).

Kernels (csrc/ecapa_bf16.hip): the SE gate's second output (the running sum of summed=True), the bf16 add of two
resident tensors and the statistics-free ReLU-mask + row-sum pass of context=False are pure functions of stored bf16
values, so each is held BIT FOR BIT to the composition it replaces.  Model: every stored tensor of the train-mode forward
teacher-forced as tests/test_ecapa_bf16_gpu.py does for the default options, the gradients against the fp64 evaluation of
tests/ecapa_resident_variants_oracle.py, hipGraph replay against eager, and the public surface."""
import pickle
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ecapa_resident_variants_oracle as vo
from oracle.filler import fill_module_, synth_feat, synth_pcm
from test_ecapa_bf16_gpu import BN_FLOOR, SENT16, _bn64, close32, res, ulp_ok, val

from _budget import check_bf16_band

pytestmark = pytest.mark.gpu

VARIANTS = [("cfsf", False, False), ("ctst", True, True), ("cfst", False, True)]
# wave-per-row kernels, 4 rows per workgroup, Tp = 256 ceil(T / 256): one row, a ragged last workgroup, more than one
# workgroup; one frame, one 8-byte vector + a frame, Tp - T = 1 / 0 / 255; the model's row; all 8 vectors per lane live
ROW_SHAPES = [(B, C, T) for B, C in ((1, 1), (1, 7), (3, 5)) for T in (1, 5, 255, 256, 257)] + [(2, 64, 750), (1, 3, 2040)]


@pytest.fixture(scope="module")
def oh():
    from asvspoof2021_air_amd import ops_h
    return ops_h


def bits(r):
    return r.contiguous().cpu()


def sliced(oh, x, lo=1, extra=3, fill=SENT16):
    """x (B, C, Tp) resident -> (channel slice [lo, lo + C) of a (B, C + extra, Tp) tensor holding x, the wide tensor):
    every operand of the kernels under test is once a view with a batch stride; the other rows hold sentinels."""
    B, C, Tp = x.shape
    wide = torch.full((B, C + extra, Tp), fill, dtype=torch.int16, device="cuda")
    wide[:, lo:lo + C] = x
    return wide[:, lo:lo + C], wide


def untouched(wide, lo, C, what):
    assert bool((wide[:, :lo] == SENT16).all()) and bool((wide[:, lo + C:] == SENT16).all()), what + " wrote a neighbouring slice"


def bf16_sum(a_bits, b_bits):
    """torch on the CPU: bf16(a + b) of two int16-bit tensors (the sum of two bf16 values in fp32, rounded once)."""
    s = a_bits.view(torch.bfloat16).float() + b_bits.view(torch.bfloat16).float()
    return s.to(torch.bfloat16).view(torch.int16)


def make_variant(context=True, summed=False, enc="ECA"):
    from asvspoof2021_air_amd.ecapa_tdnn import Bottle2neck, Res2Net2
    m = Res2Net2(Bottle2neck, C=512, model_scale=8, nOut=2, n_mels=60, context=context, summed=summed, encoder_type=enc)
    fill_module_(m)
    return m.cuda()


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("shape", ROW_SHAPES)
def test_se_gate_with_sum_output(oh, shape):
    B, C, T = shape
    x, _ = res(oh, synth_feat(shape, 11))
    r, _ = res(oh, synth_feat(shape, 12))
    z = synth_feat((B, C), 15).cuda()
    want = oh.rows(B, C, T, "cuda")
    oh.se_scale_fwd(x, z, r, T, want)
    xs, _ = sliced(oh, x, lo=2)
    rs, _ = sliced(oh, r, lo=0)
    out, wide_o = sliced(oh, torch.full_like(x, SENT16), lo=1)   # sentinels in the rows AND behind T: all of it is written
    sm, wide_s = sliced(oh, torch.full_like(x, SENT16), lo=3, extra=4)
    oh.se_scale_fwd_sum(xs, z, rs, T, out, sm)
    assert torch.equal(out, want), "out differs from se_scale_fwd"
    val(out, T), val(sm, T)  # frames behind T are zero
    assert torch.equal(bits(sm)[:, :, :T], bf16_sum(bits(out), bits(r))[:, :, :T]), "sum != bf16(stored out + res)"
    untouched(wide_o, 1, C, "se_scale_fwd_sum (out)")
    untouched(wide_s, 3, C, "se_scale_fwd_sum (sum)")
    # dense operands give the same bits
    out2, sm2 = oh.rows(B, C, T, "cuda"), oh.rows(B, C, T, "cuda")
    oh.se_scale_fwd_sum(x, z, r, T, out2, sm2)
    assert torch.equal(out2, want) and torch.equal(sm2, sm)


@pytest.mark.parametrize("shape", ROW_SHAPES)
def test_resident_add_fresh_and_in_place(oh, shape):
    """d x_{k-1} = bf16(concat-gradient slice + d s_{k-1}): a row kernel on two stored tensors, also IN PLACE over the
    slice (the form the backward uses)."""
    B, C, T = shape
    a, _ = res(oh, synth_feat(shape, 31))
    b, _ = res(oh, 0.37 * synth_feat(shape, 32))
    want = bf16_sum(bits(a), bits(b))
    got = oh.add(a, b, T)
    assert torch.equal(bits(got), want)
    val(got, T)
    a_s, wide_a = sliced(oh, a, lo=1)          # a dcat123-style slice, overwritten
    b_s, _ = sliced(oh, b, lo=2)
    oh.add(a_s, b_s, T, out=a_s)
    assert torch.equal(bits(a_s), want)
    untouched(wide_a, 1, C, "add in place over a")
    b_s2, wide_b = sliced(oh, b, lo=0)
    oh.add(a, b_s2, T, out=b_s2)               # ... and over the second operand
    assert torch.equal(bits(b_s2), want)
    untouched(wide_b, 0, C, "add in place over b")
    # stale values behind T in the destination do not survive
    dst, wide_d = sliced(oh, torch.full_like(a, SENT16), lo=1)
    oh.add(a, b, T, out=dst)
    assert torch.equal(bits(dst), want)
    untouched(wide_d, 1, C, "add into a slice")


@pytest.mark.parametrize("shape", ROW_SHAPES)
def test_relu_mask_rowsum_equals_row_stats_bwd_with_zero_statistics_gradients(oh, shape):
    B, C, T = shape
    xf = F.relu(synth_feat(shape, 21))
    xf[:, 0] = 0.0                     # a dead channel behind the ReLU: a row that is zero everywhere
    if T > 4:
        xf[:, -1, 1:4] = 0.0
    x, _ = res(oh, xf)
    df = synth_feat(shape, 24)
    df[:, :, 1::3] = -0.0              # stored -0 leaves as +0 from 0 + dx in both kernels
    dx0, _ = res(oh, df)
    dx0[:, :, T:] = 0
    mean = oh.row_stats(x, T, want_std=False)[0]
    # (T = 1: a deviation of sqrt(clamp_min) is "clamped" to row_stats_bwd, which then forms no 0 / 0)
    std = torch.full((B, C), 0.5 if T > 1 else float(np.sqrt(np.float32(1e-4))), device="cuda")
    zero = torch.zeros((B, C), device="cuda")
    want, want_rs = dx0.clone(), torch.full((B, C), 7.0, device="cuda")
    oh.row_stats_bwd(x, T, mean, std, zero, zero.clone(), want, accumulate=True, relu_mask=True, rowsum=want_rs)
    xs, _ = sliced(oh, x, lo=2)
    got, wide = sliced(oh, dx0, lo=1)
    got_rs = torch.full((B, C), 7.0, device="cuda")
    oh.relu_mask_rowsum(xs, T, got, rowsum=got_rs)
    assert torch.equal(got, want), "dx differs from row_stats_bwd"
    assert torch.equal(got_rs, want_rs), "rowsum differs from row_stats_bwd"
    untouched(wide, 1, C, "relu_mask_rowsum")
    assert int(got[:, 0].abs().max()) == 0 and bool((got_rs[:, 0] == 0).all())
    val(got, T)
    dense = dx0.clone()
    oh.relu_mask_rowsum(x, T, dense)   # without the row sums
    assert torch.equal(dense, want)


def test_new_row_kernels_refuse_rows_longer_than_the_register_cache(oh):
    from asvspoof2021_air_amd import _hip
    B, C, T = 1, 3, 2049
    x = oh.rows(B, C, T, "cuda", zero=True)
    assert x.shape[2] == 2304 > oh.max_tp()
    f2 = torch.zeros((B, C), device="cuda")
    for call in (lambda: oh.se_scale_fwd_sum(x, f2, x.clone(), T, x.clone(), x.clone()), lambda: oh.add(x, x.clone(), T),
                 lambda: oh.relu_mask_rowsum(x, T, x.clone(), rowsum=f2)):
        with pytest.raises(_hip.AirError, match="AIR_EINVAL"):
            call()
    # add: an output that overlaps an operand other than element for element is refused, not raced
    wide = oh.rows(2, 8, 96, "cuda", zero=True)
    other = oh.rows(2, 4, 96, "cuda", zero=True)
    with pytest.raises(_hip.AirError, match="AIR_EINVAL"):
        oh.add(wide[:, 0:4], other, 96, out=wide[:, 2:6])
    oh.add(wide[:, 0:4], other, 96, out=wide[:, 0:4])


# ------------------------------------------------------------------ model
@pytest.mark.parametrize("B,T", [(3, 96), (2, 401)])
@pytest.mark.parametrize("tag,context,summed", VARIANTS)
def test_variants_train_mode_every_stored_tensor_teacher_forced(oh, tag, context, summed, B, T):
    """tests/test_ecapa_bf16_gpu.py::test_train_mode_every_stored_tensor_teacher_forced for the variants, at its slacks:
    every stored (B, C, T) tensor of ``_forward_h(save=True)`` within half a bf16 ulp (+ the fp32 evaluation's noise) of
    the fp64 evaluation of its formula on the STORED inputs.  summed: each block reads the running sum, and s_1 / s_2 are
    bit-exact bf16 sums of their two stored operands.  context=False: attention.0 is the context-free contraction and no
    statistics are saved."""
    m = make_variant(context, summed).train().set_compute_dtype("bf16", variants=True)
    x = synth_feat((B, 60, T), seed=900 + T)
    with torch.no_grad():
        feat, out, S = m._forward_impl(x.cuda(), save=True)
    torch.cuda.synchronize()
    assert S["resident"] and S["T"] == T
    assert ("s_1" in S and "s_2" in S) == summed
    assert all((k in S) == context for k in ("mean", "std", "ctx", "w_c"))
    d = lambda p: p.detach().cpu().double()
    rb = lambda t: t.to(torch.bfloat16).double()
    V = lambda r: val(r.contiguous(), T)
    checked = [0]

    def stored(got_rows, exact, name, slack=0.56, floor_frac=4e-3):
        ulp_ok(V(got_rows), exact, name, slack=slack, floor=float(exact.abs().max()) * floor_frac)
        checked[0] += 1

    def pw(xs, conv_w, bias, relu=True):
        y = F.conv1d(xs, rb(d(conv_w)).view(conv_w.shape[0], -1, 1)) + d(bias)[None, :, None]
        return F.relu(y) if relu else y

    c1 = F.conv1d(rb(x.double()), rb(d(m.conv1.weight)), None, 1, 2) + d(m.conv1.bias)[None, :, None]
    stored(S["r0"], F.relu(c1), "conv1 -> relu")
    stored(S["h"], _bn64(V(S["r0"]), m.bn1, S["st0"], "bn1"), "bn1", slack=0.53, floor_frac=BN_FLOOR)
    inp = S["h"]
    for k, (blk, SB) in enumerate(zip((m.layer1, m.layer2, m.layer3), S["blocks"])):
        nm = "layer%d." % (k + 1)
        w, dil, nums = blk.width, blk.dilation, blk.nums
        assert SB["inp"].data_ptr() == inp.data_ptr()
        xin = V(SB["inp"])
        stored(SB["r1"], pw(xin, blk.conv1.weight, blk.conv1.bias), nm + "conv1 -> relu")
        o1 = _bn64(V(SB["r1"]), blk.bn1, SB["st1"], nm + "bn1")
        cat = V(SB["cat"])
        stored(SB["t"][0], o1[:, :w], nm + "bn1 slice 0 (branch 0 input)", slack=0.53, floor_frac=BN_FLOOR)
        ulp_ok(cat[:, nums * w:], o1[:, nums * w:], nm + "bn1 pass-through slice", slack=0.53, floor=float(o1.abs().max()) * BN_FLOOR)
        for i in range(nums):
            ti = V(SB["t"][i])
            ri = F.relu(F.conv1d(ti, rb(d(blk.convs[i].weight)), None, 1, dil, dil) + d(blk.convs[i].bias)[None, :, None])
            stored(SB["r"][i], ri, nm + "convs.%d -> relu" % i)
            yi = _bn64(V(SB["r"][i]), blk.bns[i], SB["st"][i], nm + "bns.%d" % i)
            ulp_ok(cat[:, i * w:(i + 1) * w], yi, nm + "bns.%d (concat slice)" % i, slack=0.53, floor=float(yi.abs().max()) * BN_FLOOR)
            checked[0] += 1
            if i + 1 < nums:
                # (o1's slice is not kept: the exact slice stands in for it, half an ulp of ITS value on top)
                o1n = o1[:, (i + 1) * w:(i + 2) * w]
                tn = cat[:, i * w:(i + 1) * w] + o1n
                ulp = lambda v: 2.0 ** (torch.floor(torch.log2(v.abs().clamp(min=1e-30))) - 7)
                err = (V(SB["t"][i + 1]) - tn).abs()
                bound = 0.53 * ulp(tn.abs().clamp(min=float(tn.abs().max()) * 1e-5)) + 0.51 * ulp(o1n)
                assert bool((err <= bound).all()), "%sbranch %d input: worst %.3f of its bound" % (nm, i + 1, float((err / bound).max()))
                checked[0] += 1
        stored(SB["r3"], pw(cat, blk.conv3.weight, blk.conv3.bias), nm + "conv3 -> relu")
        stored(SB["o3"], _bn64(V(SB["r3"]), blk.bn3, SB["st3"], nm + "bn3"), nm + "bn3", slack=0.53, floor_frac=BN_FLOOR)
        o3 = V(SB["o3"])
        close32(SB["m"], o3.mean(2), nm + "SE squeeze")
        se = blk.se.se
        z1 = F.relu(F.linear(SB["m"].cpu().double(), d(se[1].weight).view(se[1].out_channels, -1), d(se[1].bias)))
        close32(SB["z1"], z1, nm + "se.1")
        z1n = _bn64(SB["z1"].cpu().double().unsqueeze(2), se[3], SB["stS"], nm + "se.3").squeeze(2)
        close32(SB["z1n"], z1n, nm + "se.3 apply", rtol=1e-4)
        z2 = F.linear(SB["z1n"].cpu().double(), d(se[4].weight).view(se[4].out_channels, -1), d(se[4].bias))
        close32(SB["z2"], z2, nm + "se.4")
        outk = S["cat123"][:, k * 512:(k + 1) * 512]
        stored(outk, o3 * torch.sigmoid(SB["z2"].cpu().double())[:, :, None] + xin, nm + "gate * o3 + x", slack=0.53, floor_frac=BN_FLOOR)
        if summed and k < 2:
            s_k = S["s_%d" % (k + 1)]
            V(s_k)  # zeros behind T
            assert torch.equal(bits(s_k)[:, :, :T], bf16_sum(bits(outk), bits(SB["inp"]))[:, :, :T]), \
                "s_%d is not the bf16 sum of the stored s_%d and x_%d" % (k + 1, k, k + 1)
            checked[0] += 1
            inp = s_k
        else:
            inp = outk
    stored(S["x4"], pw(V(S["cat123"]), m.layer4.weight, m.layer4.bias), "layer4 -> relu")
    x4 = V(S["x4"])
    w0 = d(m.attention[0].weight).view(128, -1)
    assert w0.shape[1] == (4608 if context else 1536)
    a1 = F.conv1d(x4, rb(w0[:, :1536]).unsqueeze(2)) + d(m.attention[0].bias)[None, :, None]
    if context:
        close32(S["mean"], x4.mean(2), "context mean")
        close32(S["std"], torch.sqrt(x4.var(2).clamp(min=1e-4)), "context std", rtol=1e-4)
        a1 = a1 + F.linear(torch.cat((S["mean"], S["std"]), 1).cpu().double(), w0[:, 1536:])[:, :, None]
    stored(S["a1"], F.relu(a1), "attention.0 -> relu")
    stored(S["a1n"], _bn64(V(S["a1"]), m.attention[2], S["stA"], "attention.2"), "attention.2", slack=0.53, floor_frac=BN_FLOOR)
    logits = pw(V(S["a1n"]), m.attention[3].weight, m.attention[3].bias, relu=False)
    wts64 = torch.softmax(rb(logits), dim=2)
    got_w = V(S["wts"])
    ulp_ok(got_w, wts64, "asp softmax weights", slack=1.6, floor=float(wts64.max()) * 1e-3)
    assert float((got_w.sum(2) - 1).abs().max()) <= 1e-2
    mu = (x4 * got_w).sum(2)
    sg = torch.sqrt((((x4 * x4) * got_w).sum(2) - mu * mu).clamp(min=1e-4))
    close32(S["pooled"], torch.cat((mu, sg), 1), "attentive statistics (mu | sg)", rtol=1e-4)
    p5 = _bn64(S["pooled"].cpu().double().unsqueeze(2), m.bn5, S["st5"], "bn5").squeeze(2)
    close32(S["p5"], p5, "bn5", rtol=1e-4)
    close32(feat, F.linear(S["p5"].cpu().double(), d(m.fc6.weight), d(m.fc6.bias)), "fc6", rtol=1e-4)
    assert checked[0] == 3 * (2 + 2 * 7 + 6 + 3) + 5 + (2 if summed else 0)  # the default graph's 80 (+ s_1, s_2)


@pytest.mark.parametrize("tag,context,summed", VARIANTS)
def test_variants_grads_vs_resident_oracle(tag, context, summed):
    """All gradients of one train step (AngularIsoLoss, (B, T) = (8, 64)) against the fp64 evaluation of
    tests/ecapa_resident_variants_oracle.py, inside the band of that oracle's own fp32-vs-fp64 spread on this input
    (``_budget.check_bf16_band``; the oracle's fp32 evaluation passes the same check at this seed:
    tests/test_ecapa_resident_variants_cpu.py); loss rtol 2e-3 as for the default options."""
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    m = make_variant(context, summed).train().set_compute_dtype("bf16", variants=True)
    lossm = AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)
    fill_module_(lossm)
    lossm = lossm.cuda()
    x = synth_feat(vo.GRAD_SHAPE, seed=vo.GRAD_SEED)
    labels = vo.grad_labels(vo.GRAD_SHAPE[0])
    feat, _ = m(x.cuda())
    loss, _ = lossm(feat, labels.cuda())
    loss.backward()
    got = {k: p.grad.cpu().double().numpy().ravel() for k, p in m.named_parameters() if p.grad is not None}
    assert tuple(m.attention[0].weight.grad.shape) == (128, 4608 if context else 1536, 1)
    band, errs = vo.gradient_band(x, labels, got, context, summed)
    print("%s: median rel L2 %.3g, max %.3g; oracle fp32-vs-fp64 band: median %.3g max %.3g; loss %.6f (fp64 %.6f)" % (
        tag, np.median([e for e, _ in errs.values()]), max(e for e, _ in errs.values()), band["median"], band["max"],
        loss.item(), band["loss64"]))
    np.testing.assert_allclose(loss.item(), band["loss64"], rtol=2e-3)
    check_bf16_band(errs, band)


def _trainer(m, feat_len):
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.train import Trainer
    lossm = AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)
    fill_module_(lossm)
    return Trainer(m, loss_module=lossm, feat_len=feat_len, ecapa=True)


def test_cfst_graphed_train_step_equals_eager():
    """Trainer.enable_graph() on context=False, summed=True: three steps (two eager warm-ups, then the capture and its
    first replay) end on the loss, the scores, the embedding, every gradient, the weights and the BatchNorm statistics of
    three eager steps, bit for bit."""
    batches = [(synth_pcm(4, 16000, seed=310 + i).cuda(), ((torch.arange(4) + i) % 3 != 0).long().cuda()) for i in range(3)]
    ends = []
    for graph in (False, True):
        m = make_variant(False, True).set_compute_dtype("bf16", variants=True)
        keep = {}
        m.register_forward_hook(lambda mod, inp, out: keep.__setitem__("feat", out[0]))  # the eager step: model(x)
        orig = m.forward_saved

        def forward_saved(x, orig=orig, keep=keep):  # the captured step calls this; the replay refills the same tensor
            feats, saved = orig(x)
            keep["feat"] = feats
            return feats, saved

        m.forward_saved = forward_saved
        tr = _trainer(m, 96)
        if graph:
            tr.enable_graph()
        for pcm, lab in batches:
            loss, neg = tr.step(pcm, lab)
        torch.cuda.synchronize()
        assert (tr._graph is not None) == graph
        ends.append((loss.item(), neg.clone(), keep["feat"].detach().clone(), m.arena().grad.clone(), m.arena().flat.clone(),
                     m.layer3.bn3.running_var.clone(), tr.loss.center.detach().clone()))
    for a, b in zip(*ends):
        assert (a == b) if isinstance(a, float) else torch.equal(a, b)
    assert float(ends[0][3].abs().max()) > 0


@pytest.mark.parametrize("tag,context,summed", VARIANTS)
def test_variants_gradient_accumulation_two_backwards(tag, context, summed):
    """tests/test_ecapa_gpu.py::test_gradient_accumulation_two_backwards on the variants: a second backward without
    zero_grad ends on the SUM of both gradients in the arena views."""
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.ecapa_tdnn import Bottle2neck, Res2Net2
    torch.manual_seed(688)
    m = Res2Net2(Bottle2neck, C=512, model_scale=8, nOut=2, n_mels=60, context=context, summed=summed).cuda().train()
    m.set_compute_dtype("bf16", variants=True)
    lossm = AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0).cuda()
    xa, xb = synth_feat((4, 60, 96), seed=1).cuda(), synth_feat((4, 60, 96), seed=2).cuda()
    labels = torch.tensor([0, 1, 1, 0]).cuda()

    def grads_of(x):
        for p in m.parameters():
            p.grad = None
        feat, _ = m(x)
        lossm(feat, labels)[0].backward()
        return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    ga, gb = grads_of(xa), grads_of(xb)
    for p in m.parameters():
        p.grad = None
    for x in (xa, xb):
        feat, _ = m(x)
        lossm(feat, labels)[0].backward()
    arena = m.arena()
    assert len(ga) == 142
    for k, p in m.named_parameters():
        if k not in ga:
            continue
        want = ga[k] + gb[k]
        assert p.grad.data_ptr() == arena.grad_view(k).data_ptr()
        tol = 1e-6 * float(want.abs().max()) + 1e-12
        assert float((p.grad - want).abs().max()) <= tol, k


def test_overlapped_weight_gradients_equal_the_single_stream():
    """overlap_wgrad (weight gradients on the side stream) on cfst: the same gradients, bit for bit, as one stream - the
    in-place d x_k add and the running sums are ordered against the side stream's readers."""
    x = synth_feat((4, 60, 96), seed=7).cuda()
    outs = []
    for overlap in (True, False):
        m = make_variant(False, True).train().set_compute_dtype("bf16", variants=True)
        m.overlap_wgrad = overlap
        feat, _ = m(x)
        feat.square().mean().backward()
        torch.cuda.synchronize()
        outs.append((feat.detach().clone(), m.arena().grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------ surface
def test_default_options_same_bits_with_the_keyword_on_and_off():
    x = synth_feat((4, 60, 96), seed=5).cuda()
    outs = []
    for variants in (False, True):
        m = make_variant().train().set_compute_dtype("bf16", variants=variants)
        assert m.bf16_variants == variants
        feat, out = m(x)
        (feat.square().mean() + out.sum()).backward()
        torch.cuda.synchronize()
        outs.append((feat.detach().clone(), out.detach().clone(), m.arena().grad.clone(), m.bn5.running_mean.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_surface_refusals_pickle_and_old_pickles(tmp_path):
    from asvspoof2021_air_amd import _hip
    from asvspoof2021_air_amd import ops_h as oh
    x = synth_feat((2, 60, 96), seed=496).cuda()
    m = make_variant(False, True).eval()
    with torch.no_grad():
        for dt in ("bf16", "bf16c"):  # the one-argument form keeps refusing, and now names the keyword
            with pytest.raises(_hip.AirError, match="fp32") as e:
                m.set_compute_dtype(dt)(x)
            assert "variants=True" in str(e.value)
        with pytest.raises(ValueError):
            m.set_compute_dtype("bf16c", variants=True)
        with pytest.raises(_hip.AirError, match="ASP"):
            make_variant(True, False, "ASP").eval().set_compute_dtype("bf16", variants=True)(x)
        # longer than the resident rows: no 'bf16c' to fall back on for these options - an error naming 'fp32', no warning
        long = synth_feat((1, 60, oh.max_tp() + 40), seed=31).cuda()
        m.set_compute_dtype("bf16", variants=True)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            with pytest.raises(_hip.AirError, match="fp32"):
                m(long)
        assert not w, [str(r.message) for r in w]
        want = m(x)[0]
        # eval-mode scoring (the resident path's bound against fp32 in tests/test_ecapa_gpu.py: 2e-2 relative L2)
        ref = make_variant(False, True).eval()(x)[0]
        assert float((want - ref).norm() / ref.norm()) <= 2e-2
        # the flag travels with a whole-module pickle ...
        torch.save(m, tmp_path / "cfst.pt")
        m2 = torch.load(tmp_path / "cfst.pt", weights_only=False)
        assert m2.bf16_variants is True and m2.compute_dtype == "bf16"
        assert torch.equal(m2.eval()(x)[0], want)
        # ... and a module pickled before the keyword existed loads with it off
        old = pickle.loads(pickle.dumps(m))
        assert old.__dict__.pop("bf16_variants") is True and "bf16_variants" not in old.__dict__
        with pytest.raises(_hip.AirError, match="fp32"):
            old(x)
        old = pickle.loads(pickle.dumps(old))  # (and stays loadable)
        assert not hasattr(type(old), "bf16_variants") and "bf16_variants" not in old.__dict__
