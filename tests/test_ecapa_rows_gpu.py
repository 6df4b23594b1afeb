"""GPU: the fp32 wave-per-row ECAPA kernels (csrc/ecapa_ops.hip) against the fp64 oracle of tests/ecapa_rows_oracle.py at
the shapes, lengths and clamp / softmax edges where such kernels go wrong.

* Row counts that leave the last workgroup (4 waves, one row each) ragged; lengths around the wave (63 / 64 / 65), the
  register-cached limit (1023 / 1024 / 1025) and the loop kernels behind it (1100).
* Tolerances are the project's (2e-5 forward, 1e-4 backward and reductions), applied PER ROW against the oracle's row
  scale - the summed magnitudes of the terms of an element - not against the tensor's maximum.
* Every output is a view into a larger allocation filled with a sentinel pattern, at least three rows' worth behind it;
  the sentinels must come back unchanged, so a broken row guard is reported instead of faulting.
* The pooling's deviation is compared through sg^2 = sum x^2 w - mu^2 at the kernel's own stored weights.  The formula
  (E[x^2] - mu^2, the reference model's own) cancels: what can be promised is relative to sum x^2 w + mu^2, not to sg.

What the fp32 arithmetic in kernel order costs by itself, as a fraction of each tolerance, on exactly these inputs
(tests/test_ecapa_rows_cpu.py, numpy fp32): row mean 0.005, row std 0.005, row sum 0.005, row_stats_bwd dx 0.001 /
rowsum 0.001, asp w 0.008, mu 0.006, sg^2 0.006, asp_bwd dx 0.001 / d logits 0.001 / rowsum 0.0004, se fwd 0.003 /
dx 0.006 / dz 0.0003, channel_sum 0.001; large-mean sg^2 0.054 of its n 2^-24 bound.

The bf16-copy side outputs of res2_bn_apply / add_strided are asserted by test_bf16_copies_gpu.py (T = 750, 101) and
are not repeated here; those of row_stats_bwd, asp_bwd and se_scale_fwd are checked here at ragged shapes."""
import ctypes

import numpy as np
import pytest
import torch

import ecapa_rows_oracle as eo
from ecapa_rows_oracle import BWD_TOL, FWD_TOL, rel_to_scale

pytestmark = pytest.mark.gpu

SENT_BITS = 0x4B3C614E  # a finite float32 (1.2345678e7) no kernel here produces
SENT16 = 0x4B3C         # ... and the bf16 it starts with
FILL = -7.0             # what an output holds before the call


@pytest.fixture(scope="module")
def ops():
    from asvspoof2021_air_amd import ops
    return ops


def hip():
    from asvspoof2021_air_amd import _hip
    return _hip


class Guard:
    """A tensor of ``shape`` inside a larger allocation: ``pad`` sentinel elements in front (plus ``shift`` that move it
    off its 8-byte alignment) and ``pad`` behind."""

    def __init__(self, shape, pad, dtype=torch.float32, shift=0):
        n = int(np.prod(shape))
        self.sent = SENT_BITS if dtype == torch.float32 else SENT16
        store = torch.int32 if dtype == torch.float32 else torch.int16
        self.lo, self.hi = pad + shift, pad + shift + n
        self.raw = torch.full((self.hi + pad,), self.sent, dtype=store, device="cuda")
        self.t = self.raw[self.lo:self.hi].view(dtype).view(shape)
        if dtype == torch.float32:
            self.t.fill_(FILL)

    def check(self, what):
        guard = torch.cat([self.raw[:self.lo], self.raw[self.hi:]])
        bad = (guard != self.sent).nonzero().flatten().tolist()
        assert not bad, "%s wrote outside its buffer: sentinel elements %s changed (buffer = %d..%d)" % (
            what, bad[:8], self.lo, self.hi)


def pad3(T):
    return max(64, 3 * T)


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def held(got, want, scale, tol, what, absolute=0.0):
    g = got.detach().cpu().numpy()
    assert np.isfinite(g).all(), what + ": not finite"
    r = rel_to_scale(g, want, scale, absolute)
    print("%-34s %.3g of its row scale (bound %.3g)" % (what, r, tol))
    assert r <= tol, "%s: %.3g of the row scale > %.3g" % (what, r, tol)


def bf16_copy_ok(bf, src, T, what):
    """bf (B, C, Tp) int16 in a Guard: frames < T = bf16(src) rounded to nearest even, frames >= T untouched."""
    assert torch.equal(bf.t[:, :, :T], src.to(torch.bfloat16).view(torch.int16)), what + ": bf16 copy"
    assert bool((bf.t[:, :, T:] == SENT16).all()), what + ": bf16 copy written behind T"
    bf.check(what + " bf16 copy")


# ---- row statistics --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(eo.rs_cases()))
def test_row_stats_and_bwd(ops, name):
    d = eo.rs_cases()[name]
    B, C, T = d["x"].shape
    c = d["clamp_min"]
    dmean, dstd = G(d["dmean"]), G(d["dstd"])
    for relu in (False, True):
        xn = np.maximum(d["x"], 0) if relu else d["x"]
        x = G(xn)
        st = eo.row_stats(xn, c)
        mean, std, mean_only = Guard((B, C), 64), Guard((B, C), 64), Guard((B, C), 64)
        ops.row_stats(x, clamp_min=c, mean_out=mean.t, std_out=std.t)
        ops.row_stats(x, want_std=False, mean_out=mean_only.t)
        for g_, n_ in ((mean, "mean"), (std, "std"), (mean_only, "mean (want_std=False)")):
            g_.check("row_stats " + n_)
        held(mean.t, st["mean"], st["mean_scale"], FWD_TOL, "row mean")
        held(mean_only.t, st["mean"], st["mean_scale"], FWD_TOL, "row mean, no std")
        held(std.t, st["std"], st["std_scale"], FWD_TOL, "row std")
        if T <= 1024:  # the register-cached path promises the loop's addition order
            assert torch.equal(mean.t, mean_only.t), "mean differs between want_std=True and False"
        rs = Guard((B, C), 64)
        hip().check(hip().lib().air_row_sum(hip().dptr(x), hip().ci(B), hip().ci(C), hip().ci(T), hip().dptr(rs.t),
                                            hip().stream()), "air_row_sum")
        rs.check("row_sum")
        held(rs.t, st["sum"], st["sum_scale"], FWD_TOL, "row sum")
        clamped = torch.from_numpy(st["clamped"])
        if name.startswith("clamp"):
            assert clamped.tolist() == [[True, True, True, False, False]]
            want_sd = torch.tensor(float(np.sqrt(np.float32(c))), dtype=torch.float32)
            assert bool((std.t.cpu()[clamped] == want_sd).all()), "a clamped row's std is not sqrt(float32(clamp_min))"
        # backward from the kernel's own statistics, as the model runs it
        dx = Guard((B, C, T), pad3(T))
        rowsum = Guard((B, C), 64)
        bf = Guard((B, C, T + 5), pad3(T + 5), torch.int16)
        if relu:
            dx.t.copy_(G(d["dx0"]))
        ops.row_stats_bwd(x, mean.t, std.t, dmean, dstd, dx.t, accumulate=relu, clamp_min=c, relu_mask=relu,
                          rowsum=rowsum.t if relu else None, dx_bf16=bf.t if relu else None)
        dx.check("row_stats_bwd dx")
        want = eo.row_stats_bwd(xn, d["dmean"], d["dstd"], c, d["dx0"] if relu else None, relu)
        held(dx.t, want["dx"], want["dx_scale"], BWD_TOL, "row_stats_bwd dx (relu_mask=%s)" % relu)
        if relu:
            rowsum.check("row_stats_bwd rowsum")
            held(rowsum.t, want["rowsum"], want["rowsum_scale"], BWD_TOL, "row_stats_bwd rowsum")
            bf16_copy_ok(bf, dx.t, T, "row_stats_bwd")
        else:
            assert bool((rowsum.t == FILL).all())
            # a clamped row carries no dstd term: dmean / T + 0 * (x - mean) is one value for the whole row
            rows = dx.t.cpu()[clamped]
            assert bool((rows == rows[:, :1]).all()), "a clamped row's dx varies over time: it carries a dstd term"
        if relu and name.startswith("clamp"):
            assert bool((dx.t[0, 0] == 0).all()) and float(rowsum.t[0, 0]) == 0.0, "dead channel under the ReLU mask"


# ---- attentive statistics pooling ------------------------------------------------------------------------------
def _asp_fwd(x, w_guard, out_guard):
    B, C, T = x.shape
    H = hip()
    H.check(H.lib().air_asp_fwd(H.dptr(x), H.dptr(w_guard.t), H.ci(B), H.ci(C), H.ci(T), H.dptr(out_guard.t), H.stream()),
            "air_asp_fwd")
    w_guard.check("asp_fwd weights")
    out_guard.check("asp_fwd out")


@pytest.mark.parametrize("name", list(eo.asp_cases()))
def test_asp_and_bwd(ops, name):
    d = eo.asp_cases()[name]
    B, C, T = d["x"].shape
    x = G(d["x"])
    w, out = Guard((B, C, T), pad3(T)), Guard((B, 2 * C), 64)
    w.t.copy_(G(d["a"]))
    _asp_fwd(x, w, out)
    f = eo.asp_fwd(d["x"], a=d["a"])
    held(w.t, f["w"], f["w_scale"], FWD_TOL, "asp weights")
    wn = w.t.cpu().numpy()
    fs = eo.asp_fwd(d["x"], w=wn)  # the stored weights define the pooled statistics
    held(out.t[:, :C], fs["mu"], fs["mu_scale"], FWD_TOL, "asp mu")
    held(out.t[:, C:].double() ** 2, fs["sg2"], fs["sg2_scale"], FWD_TOL, "asp sg^2")
    if name == "softmax-range":
        assert fs["clamped"].tolist() == [[False, True, False, True, True]]
        sg = out.t[0, C:].cpu()
        assert bool((sg[[1, 3, 4]] == torch.tensor(np.float32(0.01))).all()), "a cancelled sg^2 must store sqrt(1e-4f)"
        assert abs(float(w.t[0, 1, 40]) - 1.0) <= 1e-6 and abs(float(w.t[0, 2].max()) - 1.0 / T) <= 1e-7
    dout = G(d["dout"])
    stored_w = w.t.clone()
    for acc in (False, True):
        w.t.copy_(stored_w)
        dx, rowsum = Guard((B, C, T), pad3(T)), Guard((B, C), 64)
        bf = Guard((B, C, T + 3), pad3(T + 3), torch.int16)
        if acc:
            dx.t.copy_(G(d["dx0"]))
        ops.asp_bwd(x, w.t, out.t, dout, dx.t, accumulate=acc, rowsum=rowsum.t, dlogits_bf16=bf.t)
        for g_, n_ in ((dx, "dx"), (w, "d logits"), (rowsum, "rowsum"), (out, "out")):
            g_.check("asp_bwd " + n_)
        want = eo.asp_bwd(d["x"], wn, d["dout"][:, :C], d["dout"][:, C:], d["dx0"] if acc else None)
        held(dx.t, want["dx"], want["dx_scale"], BWD_TOL, "asp_bwd dx (accumulate=%s)" % acc)
        held(w.t, want["da"], want["da_scale"], BWD_TOL, "asp_bwd d logits")
        da = w.t.cpu().double().numpy()  # (analytically zero: judged on the summed magnitudes of the stored values)
        held(rowsum.t, da.sum(-1), np.abs(da).sum(-1), BWD_TOL, "asp_bwd rowsum of the stored d logits")
        bf16_copy_ok(bf, w.t, T, "asp_bwd")


def test_asp_large_mean(ops):
    """x = 10 + 0.1 noise, T = 750: sg^2 = sum x^2 w - mu^2 loses four digits.  Bound, relative to sum x^2 w + mu^2 at the
    kernel's stored w: n 2^-24 with n = 12 frames per lane + 6 tree levels + 2 (the kernel's longest rounding chain;
    errors do not all align - the kernel-order restatement on the CPU measures 0.054 of it).  The formula is the
    reference model's own; relative to sg itself (0.1) nothing better than ~1e-3 can be promised."""
    d = eo.large_mean_case()
    B, C, T = d["x"].shape
    w, out = Guard((B, C, T), pad3(T)), Guard((B, 2 * C), 64)
    w.t.copy_(G(d["a"]))
    _asp_fwd(G(d["x"]), w, out)
    fs = eo.asp_fwd(d["x"], w=w.t.cpu().numpy())
    assert not fs["clamped"].any()
    held(out.t[:, :C], fs["mu"], fs["mu_scale"], FWD_TOL, "asp mu, large mean")
    held(out.t[:, C:].double() ** 2, fs["sg2"], fs["s2"] + fs["mu"] ** 2, eo.large_mean_bound(T), "asp sg^2, large mean")


# ---- SE gate ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(eo.se_cases()))
def test_se_scale(ops, name):
    d = eo.se_cases()[name]
    B, C, T = d["x"].shape
    x, z = G(d["x"]), G(d["z"])
    res_big = torch.full((B, 3 * C, T), 3.0, device="cuda")
    res_big[:, C:2 * C] = G(d["res"])
    out_big = Guard((B, 2 * C + 1, T), pad3(T))
    bf_big = Guard((B, C + 2, T + 7), pad3(T + 7), torch.int16)
    ops.se_scale_fwd(x, z, res_big[:, C:2 * C], out_big.t[:, 1:C + 1], out_bf=bf_big.t[:, 1:C + 1])
    out_big.check("se_scale_fwd")
    f = eo.se_fwd(d["x"], d["z"], d["res"])
    held(out_big.t[:, 1:C + 1], f["out"], f["out_scale"], FWD_TOL, "se fwd")
    assert bool((out_big.t[:, :1] == FILL).all()) and bool((out_big.t[:, C + 1:] == FILL).all()), "neighbouring channels"
    assert torch.equal(bf_big.t[:, 1:C + 1, :T], out_big.t[:, 1:C + 1].to(torch.bfloat16).view(torch.int16))
    assert bool((bf_big.t[:, 1:C + 1, T:] == SENT16).all()) and bool((bf_big.t[:, :1] == SENT16).all()) and bool(
        (bf_big.t[:, C + 1:] == SENT16).all())
    bf_big.check("se_scale_fwd bf16 copy")
    # backward with dout a channel slice of a wider tensor
    dout_big = torch.full((B, 2 * C + 3, T), 5.0, device="cuda")
    dout_big[:, 2:C + 2] = G(d["dout"])
    dx, dz = Guard((B, C, T), pad3(T)), Guard((B, C), 64)
    H = hip()
    dp, db = ops.vptr(dout_big[:, 2:C + 2])
    H.check(H.lib().air_se_scale_bwd(H.dptr(x), H.dptr(z), dp, H.csz(db), H.ci(B), H.ci(C), H.ci(T), H.dptr(dx.t),
                                     H.dptr(dz.t), H.stream()), "air_se_scale_bwd")
    dx.check("se_scale_bwd dx")
    dz.check("se_scale_bwd dz")
    b = eo.se_bwd(d["x"], d["z"], d["dout"])
    held(dx.t, b["dx"], b["dx_scale"], FWD_TOL, "se dx", b["dx_abs"])
    held(dz.t, b["dz"], b["dz_scale"], BWD_TOL, "se dz", b["dz_abs"])
    dx2, dz2 = ops.se_scale_bwd(x, z, dout_big[:, 2:C + 2])  # the wrapper the model calls
    assert torch.equal(dx2, dx.t) and torch.equal(dz2, dz.t)
    if name == "gate-range":  # z = 0, 20, -20, 88, -88, 100, -100, 1e4, -1e4
        one, zero = [1, 3, 5, 7], [6, 8]
        do = G(d["dout"])
        assert torch.equal(dx.t[0, one], do[0, one]), "g must saturate to exactly 1"
        assert bool((dx.t[0, zero] == 0).all()), "g must saturate to exactly 0"
        assert bool((dz.t[0, one + zero] == 0).all()), "dz of a saturated gate"
        assert torch.equal(out_big.t[0, 1:C + 1][zero], G(d["res"])[0, zero])


# ---- channel sum -----------------------------------------------------------------------------------------------
def _splits(B, C):
    want = min(max(2048 // C, 1), B)
    per = -(-B // want)
    return -(-B // per), per


@pytest.mark.parametrize("shape", eo.CHANNEL_SUM_SHAPES + ["slice"])
def test_channel_sum(ops, shape):
    if shape == "slice":
        big = G(eo._n((4, 192, 33), 1450))
        x, xn = big[:, 64:128], big[:, 64:128].cpu().numpy()
    else:
        xn = eo.channel_sum_input(shape)
        x = G(xn)
    B, C, S = xn.shape
    nsplit, per = _splits(B, C)
    if shape in ((5, 512, 10), (7, 1024, 9), (3, 4096, 3)):
        assert (nsplit, per, B - (nsplit - 1) * per) == {5: (3, 2, 1), 7: (2, 4, 3), 3: (1, 3, 3)}[B]
    n = int(hip().lib().air_channel_sum_ws_bytes(hip().ci(B), hip().ci(C)))
    ws = ops.workspace(n, x.device)
    ws.fill_(0x5A)
    out = Guard((C,), 64)
    ops.channel_sum(x, out=out.t)
    out.check("channel_sum")
    want = eo.channel_sum(xn)
    held(out.t, want["out"], want["out_scale"], BWD_TOL, "channel_sum")
    used = nsplit * C * 8 if nsplit > 1 else 0
    assert bool((ws[used:] == 0x5A).all()), "workspace behind the %d partials" % (nsplit * C)


# ---- grid caps -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_b", [False, True])
def test_add_strided_beyond_the_grid_cap(ops, with_b):
    B, C, S = 2, 257, 1024  # 1028 workgroups of elements per utterance: the 1024-workgroup cap makes the loop stride
    a_big, b_big = G(eo._n((B, 2 * C, S), 1500)), G(eo._n((B, C + 5, S), 1501))
    out_big = Guard((B, C + 2, S), pad3(S))
    a, b = a_big[:, C:], b_big[:, 3:C + 3]
    ops.add_strided(out_big.t[:, 1:C + 1], a, b if with_b else None)
    out_big.check("add_strided")
    assert torch.equal(out_big.t[:, 1:C + 1], a + b if with_b else a)
    assert bool((out_big.t[:, :1] == FILL).all()) and bool((out_big.t[:, C + 1:] == FILL).all())


def test_relu_mask_beyond_the_grid_cap(ops):
    n = 8192 * 256 + 257
    y = G(eo._n((n,), 1510))
    y[5], y[8192 * 256 + 3] = -0.0, -0.0
    y[6], y[8192 * 256 + 4] = 1e-40, -1e-40  # subnormal: positive, however small
    y[7] = 0.0
    dx = Guard((n,), 1024)
    dx.t.copy_(G(eo._n((n,), 1511)))
    want = torch.where(y > 0, dx.t, torch.zeros((), device="cuda"))
    assert float(want[6]) != 0.0 and float(want[5]) == 0.0
    ops.relu_mask_(dx.t, y)
    dx.check("relu_mask")
    assert torch.equal(dx.t, want)


# ---- Res2 chain step -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,shift", [(33, 0), (34, 0), (34, 1), (1026, 0), (2051, 0)])
def test_res2_bn_apply(ops, S, shift):
    """Odd S: the slices start on 4-byte-only boundaries (scalar path, 3 blocks per plane at 2051); even S: the 16-byte
    path with its 2-float tail (S % 4 == 2), two blocks per plane at 1026; shift = 1 moves an even-S concat off its
    8-byte alignment, which must fall back to the scalar path."""
    B, C = 2, 3
    xn, addn = eo._n((B, C, S), 1600 + S), eo._n((B, C, S), 1601 + S)
    scn, shn = 1.0 + 0.2 * eo._n((C,), 1602), 0.3 * eo._n((C,), 1603)
    x = G(xn)
    cat = Guard((B, 3 * C, S), pad3(S), shift=shift)
    add_big = torch.full((B, 2 * C, S), 9.0, device="cuda")
    add_big[:, C:] = G(addn)
    y2 = Guard((B, C, S), pad3(S))
    ops.res2_bn_apply(x, G(scn), G(shn), cat.t[:, C:2 * C], add_big[:, C:], y2.t)
    cat.check("res2_bn_apply y1")
    y2.check("res2_bn_apply y2")
    sc, sh = scn.astype(np.float64)[None, :, None], shn.astype(np.float64)[None, :, None]
    v = xn.astype(np.float64) * sc + sh
    mag = np.abs(xn * sc) + np.abs(sh)
    held(cat.t[:, C:2 * C], v, mag.max(-1), FWD_TOL, "res2 y1")
    held(y2.t, v + addn, (mag + np.abs(addn)).max(-1), FWD_TOL, "res2 y2")
    assert torch.equal(y2.t, cat.t[:, C:2 * C] + add_big[:, C:]), "y2 = stored y1 + add"
    assert bool((cat.t[:, :C] == FILL).all()) and bool((cat.t[:, 2 * C:] == FILL).all()), "other channels of the concat"
    only1 = Guard((B, 3 * C, S), pad3(S), shift=shift)
    ops.res2_bn_apply(x, G(scn), G(shn), only1.t[:, C:2 * C])  # the last branch: no add, no y2
    only1.check("res2_bn_apply y1 alone")
    assert torch.equal(only1.t, cat.t)
