"""GPU: the small kernels every train step ends in, pinned to exact references.

* air_dropout_mask(_ctr) / air_randn(_ctr): the bits of Philox4x32-10 (tests/philox_oracle.py, itself pinned to the
  Random123 known-answer vectors in test_philox_cpu.py);
* air_adam_step / air_sgd_step: fp64 evaluation of the same step, elementwise bounds from fp32 rounding;
* air_softmax_ce_fwd / _bwd: torch fp64 log-softmax / cross-entropy on the same float32 logits;
* air_mask_relu_fwd / _bwd, air_scale, air_mul, air_copy_pad, air_add_inplace: numpy float32, bit for bit.

Every buffer a kernel writes is a slice of a larger allocation with >= 64 sentinel words on both sides, and the
sentinels must come back unchanged: a write past ``n`` fails the test that made it.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.filler import synth_feat

import philox_oracle as po
from adam_oracle import (ADAM_DEFAULT, ADAM_N, ADAM_POINT_N, ADAM_POINTS, BIG_N, EPS32, adam_inputs, adam_ref64,
                         assert_adam, f32)

pytestmark = pytest.mark.gpu

SENT = 64            # sentinel words on each side of a guarded buffer
SENT_BITS = 0x4B3C614E  # a finite float32 (1.2345678e7) no kernel here produces
FILL = -7.0          # what an output holds before a call: stale results of an earlier call cannot pass for fresh ones


@pytest.fixture(scope="module")
def ops():
    from asvspoof2021_air_amd import ops
    return ops


@pytest.fixture(scope="module")
def adv():
    from asvspoof2021_air_amd import adversarial
    return adversarial


@pytest.fixture(scope="module")
def L():
    from asvspoof2021_air_amd import _hip
    return _hip.lib()


def hip():
    from asvspoof2021_air_amd import _hip
    return _hip


class Guarded:
    """``n`` elements of ``dtype`` inside a larger allocation: SENT sentinel words in front (plus ``shift`` words that
    move the slice off its 16-byte alignment) and SENT behind.  ``.t`` is the slice, ``check()`` the sentinel test."""

    def __init__(self, n, shift=0, dtype=torch.float32, value=None):
        words = n * (2 if dtype == torch.int64 else 1)
        self.lo, self.hi = SENT + shift, SENT + shift + words
        self.raw = torch.full((self.hi + SENT,), SENT_BITS, dtype=torch.int32, device="cuda")
        self.t = self.raw[self.lo:self.hi].view(dtype)
        assert self.t.data_ptr() % 16 == 4 * (shift % 4)
        if value is None:
            if dtype == torch.float32:
                self.t.fill_(FILL)
        else:
            self.set(value)

    def set(self, value):
        if isinstance(value, np.ndarray):
            value = torch.from_numpy(value)
        if torch.is_tensor(value):
            self.t.copy_(value.reshape(-1))
        else:
            self.t.fill_(value)
        return self

    def check(self, what=""):
        guard = torch.cat([self.raw[:self.lo], self.raw[self.hi:]])
        bad = (guard != SENT_BITS).nonzero().flatten().tolist()
        assert not bad, "%s wrote outside its buffer: sentinel words %s changed (buffer = words %d..%d)" % (
            what, bad[:8], self.lo, self.hi)

    def np(self):
        return self.t.cpu().numpy()


def bits(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def assert_bits(got, want, what):
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d: got %r want %r" % (
        what, bad.size, g.size, bad[0], np.asarray(got.cpu() if torch.is_tensor(got) else got).reshape(-1)[bad[0]],
        np.asarray(want).reshape(-1)[bad[0]])


def u64(x):
    return ctypes.c_uint64(x)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return hip().stream()


def ok(rc, what):
    hip().check(rc, what)


# ---------------------------------------------------------------------------------------------- Philox draws
DRAW_N = [1, 2, 3, 4, 5, 1023, 1024, 1025, 4 * 256 * 3 + 2]  # every n % 4, one block, ragged last block, several blocks
DRAW_P = [0.0, 0.3, 0.7, 0.999]
DRAW_SEED = [0, 7, 2 ** 32 + 5, 2 ** 63 + 11]
DRAW_OFFSET = [0, 1, 2 ** 32 - 1, 2 ** 32 + 3]  # 2^32 - 1 with n >= 8 carries into the high counter word in one launch
CTR_START = 2 ** 32 - 2


@pytest.mark.parametrize("n", DRAW_N)
def test_dropout_mask_is_philox(L, adv, n):
    out = Guarded(n)
    for p, seed, offset in itertools.product(DRAW_P, DRAW_SEED, DRAW_OFFSET):
        what = "air_dropout_mask(n=%d, p=%g, seed=%d, offset=%d)" % (n, p, seed, offset)
        want = po.dropout_keep(n, p, seed, offset)
        out.set(FILL)
        ok(L.air_dropout_mask(ptr(out.t), ctypes.c_size_t(n), ctypes.c_float(p), u64(seed), u64(offset), stream()), what)
        out.check(what)
        assert_bits(out.t, want, what)
        assert_bits(adv.dropout_mask((n,), p, seed, offset, "cuda"), want, "adversarial.dropout_mask" + what[16:])
        if p == 0.0:
            assert bool((out.t == 1.0).all())


def test_dropout_first_quad_is_the_known_answer_block(adv):
    """Seed 0, offset 0: the first quad is the Random123 vector 6627e8d5 e169c58d bc57ac4c 9b00dbd8, i.e.
    u = .3990, .8805, .7357, .6055, thresholded."""
    kat = [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    for p in (0.5, 0.7, 0.75, 0.9):
        scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
        want = [scale if float(np.float32(w) * np.float32(2.0 ** -32)) >= float(np.float32(p)) else 0.0 for w in kat]
        assert adv.dropout_mask((4,), p, 0, 0, "cuda").tolist() == want, p
    assert adv.dropout_mask((4,), 0.7, 0, 0, "cuda").tolist()[0::3] == [0.0, 0.0]


@pytest.mark.parametrize("n", DRAW_N)
def test_dropout_mask_ctr_is_philox_and_advances(L, ops, n):
    out = Guarded(n)
    ctr = Guarded(1, dtype=torch.int64)
    quads = (n + 3) // 4
    for p, seed in itertools.product(DRAW_P, DRAW_SEED):
        what = "air_dropout_mask_ctr(n=%d, p=%g, seed=%d)" % (n, p, seed)
        ctr.set(CTR_START)
        for call in range(2):  # the second call continues the sequence where the first one stopped
            out.set(FILL)
            ok(L.air_dropout_mask_ctr(ptr(out.t), ctypes.c_size_t(n), ctypes.c_float(p), u64(seed), ptr(ctr.t),
                                      stream()), what)
            out.check(what)
            ctr.check(what + " counter")
            assert_bits(out.t, po.dropout_keep(n, p, seed, CTR_START + call * quads), "%s call %d" % (what, call))
            assert ctr.t.item() == CTR_START + (call + 1) * quads, (what, call)
        got = ops.dropout_mask_ctr((n,), p, seed, ctr.t, "cuda")
        assert_bits(got, po.dropout_keep(n, p, seed, CTR_START + 2 * quads), "ops.dropout_mask_ctr" + what[20:])
        assert ctr.t.item() == CTR_START + 3 * quads


# |got - ref| / scale over the whole n / seed / offset / scale set, air_randn and air_randn_ctr alike.  Device logf,
# sqrtf and sincosf carry ULP-level error, so this comparison cannot be bit-exact (r <= 6.7 has an ulp of 4.8e-7).
# Largest value measured on an MI355X: 3.91e-7.  The bound is four times that; it may never exceed 1e-4, and any
# structural error (wrong word, wrong lane, sin for cos, a dropped round) gives errors of order 1.
RANDN_MEASURED = 3.91e-7
RANDN_BOUND = 4 * RANDN_MEASURED
assert RANDN_BOUND <= 1e-4


def randn_err(got, n, seed, offset, scale):
    ref = po.randn_ref(n, seed, offset, scale)
    return np.abs(got.astype(np.float64) - ref) / float(np.float32(scale)), ref


@pytest.mark.parametrize("scale", [1.0, 1e-5])
@pytest.mark.parametrize("n", DRAW_N)
def test_randn_is_box_muller_of_philox(L, ops, n, scale):
    out = Guarded(n)
    for seed, offset in itertools.product(DRAW_SEED, DRAW_OFFSET):
        what = "air_randn(n=%d, seed=%d, offset=%d, scale=%g)" % (n, seed, offset, scale)
        out.set(FILL)
        ok(L.air_randn(ptr(out.t), ctypes.c_size_t(n), u64(seed), u64(offset), ctypes.c_float(scale), stream()), what)
        out.check(what)
        err, _ = randn_err(out.np(), n, seed, offset, scale)
        werr, _ = randn_err(ops.randn((n,), "cuda", seed, offset, scale).cpu().numpy(), n, seed, offset, scale)
        assert err.max() <= RANDN_BOUND, "%s: element %d off by %.3g scale" % (what, err.argmax(), err.max())
        assert werr.max() <= RANDN_BOUND, "ops.randn / %s: element %d off by %.3g scale" % (what, werr.argmax(), werr.max())


@pytest.mark.parametrize("scale", [1.0, 1e-5])
@pytest.mark.parametrize("n", DRAW_N)
def test_randn_ctr_is_box_muller_of_philox_and_advances(L, ops, n, scale):
    out = Guarded(n)
    ctr = Guarded(1, dtype=torch.int64)
    quads = (n + 3) // 4
    for seed in DRAW_SEED:
        what = "air_randn_ctr(n=%d, seed=%d, scale=%g)" % (n, seed, scale)
        ctr.set(CTR_START)
        for call in range(2):
            out.set(FILL)
            ok(L.air_randn_ctr(ptr(out.t), ctypes.c_size_t(n), u64(seed), ptr(ctr.t), ctypes.c_float(scale), stream()),
               what)
            out.check(what)
            ctr.check(what + " counter")
            err, _ = randn_err(out.np(), n, seed, CTR_START + call * quads, scale)
            assert err.max() <= RANDN_BOUND, "%s call %d: element %d off by %.3g scale" % (what, call, err.argmax(), err.max())
            assert ctr.t.item() == CTR_START + (call + 1) * quads, (what, call)
        got = ops.randn_ctr((n,), "cuda", seed, ctr.t, scale).cpu().numpy()
        err, _ = randn_err(got, n, seed, CTR_START + 2 * quads, scale)
        assert err.max() <= RANDN_BOUND, "ops.randn_ctr / %s: element %d off by %.3g scale" % (what, err.argmax(), err.max())
        assert ctr.t.item() == CTR_START + 3 * quads


def test_randn_element_to_quad_lane_mapping(ops):
    """out[4q + j] is lane j of quad q: one element in the second block, named, so that a failure says which."""
    n, seed, offset = 4 * 256 * 3 + 2, 7, 2 ** 32 - 1
    q, j = 256, 1  # first quad of block 1 (counter offset + 256: the high counter word is 1 here), its sine lane
    got = ops.randn((n,), "cuda", seed, offset, 1.0).cpu().numpy()
    w = [int(x) for x in po.philox4x32_10((offset + q) & 0xFFFFFFFF, (offset + q) >> 32, seed)[0]]
    f32 = np.float32
    u1, u2 = (f32(w[0]) + f32(1.0)) * f32(2.0 ** -32), f32(w[1]) * f32(2.0 ** -32)
    want = np.sqrt(-2.0 * np.log(float(u1))) * np.sin(float(f32(6.283185307179586) * u2))
    assert abs(want - po.randn_ref(n, seed, offset, 1.0)[4 * q + j]) <= 1e-14
    assert abs(got[4 * q + j] - want) <= RANDN_BOUND, "out[4*%d + %d] = %r, want %r (quad %d lane %d)" % (
        q, j, got[4 * q + j], want, q, j)


# ---------------------------------------------------------------------------------------------- Adam / SGD
class AdamBuffers:
    SHIFTS = {"aligned": (0, 0, 0, 0), "all+1": (1, 1, 1, 1), "g+1": (0, 1, 0, 0)}

    def __init__(self, n, align, p, m, v):
        s = self.SHIFTS[align]
        self.p, self.g, self.m, self.v = (Guarded(n, shift=s[i], value=a) for i, a in
                                          enumerate((p, np.zeros(n, np.float32), m, v)))

    def step(self, ops, g, step, **hyper):
        self.g.set(g)
        before = tuple(b.np() for b in (self.p, self.m, self.v))
        ops.adam_step(self.p.t, self.g.t, self.m.t, self.v.t, step, **hyper)
        for b, name in ((self.p, "p"), (self.g, "g"), (self.m, "m"), (self.v, "v")):
            b.check("air_adam_step / %s" % name)
        assert_bits(self.g.t, g, "air_adam_step must not write g")
        return before, tuple(b.np() for b in (self.p, self.m, self.v))


def run_adam(ops, n, align, hyper, steps=(1, 2, 3), moments=False, twin=None):
    """Consecutive steps; after each one p, m and v are held against the fp64 step from the state the kernel started
    that step with (the same float32 values).  ``twin``: a second alignment that must give the same bits."""
    p, _, m, v = adam_inputs(n, 1, moments)
    bufs = AdamBuffers(n, align, p, m, v)
    other = AdamBuffers(n, twin, p, m, v) if twin else None
    for k in steps:
        g = adam_inputs(n, k)[1]
        (p0, m0, v0), got = bufs.step(ops, g, k, **hyper)
        ref, tol = adam_ref64(p0, g, m0, v0, k, **hyper)
        assert_adam(got, ref, tol, "air_adam_step(n=%d, %s, step %d, %s)" % (n, align, k, hyper))
        if other:
            _, got2 = other.step(ops, g, k, **hyper)
            for name, a, b in zip("pmv", got, got2):
                assert_bits(b, a, "air_adam_step(n=%d, step %d): %s of the %s layout against %s" % (n, k, name, twin, align))


@pytest.mark.parametrize("align", ["aligned", "all+1", "g+1"])
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_sizes_and_alignments(ops, n, align):
    # "all+1" runs the scalar branch and, next to it, the float4 branch on the same values: same bits
    run_adam(ops, n, align, ADAM_DEFAULT, twin="aligned" if align == "all+1" else None)


@pytest.mark.parametrize("point", ADAM_POINTS, ids=lambda d: ",".join("%s=%g" % kv for kv in d.items()))
@pytest.mark.parametrize("align", ["aligned", "all+1"])
def test_adam_hyper_parameters(ops, point, align):
    run_adam(ops, ADAM_POINT_N, align, dict(ADAM_DEFAULT, **point))


@pytest.mark.parametrize("step", [1, 2, 1000, 100000])
def test_adam_step_count_with_nonzero_moments(ops, step):
    run_adam(ops, ADAM_POINT_N, "aligned", ADAM_DEFAULT, steps=(step,), moments=True)


def test_adam_edges(L, ops):
    n = 1027
    p = synth_feat((n,), 1).numpy()
    zero = np.zeros(n, np.float32)
    b = AdamBuffers(n, "aligned", p, zero, zero)
    _, (p1, m1, v1) = b.step(ops, zero, 1, **dict(ADAM_DEFAULT, weight_decay=0.0))
    assert_bits(p1, p, "g = 0, wd = 0, zero moments: p")  # m / (sqrt(v) + eps) = 0 / eps: nothing moves
    assert not m1.any() and not v1.any()
    # n = 0 is a no-op, step < 1 is refused - and neither touches memory
    g = synth_feat((n,), 2).numpy()
    b.g.set(g)
    ok(L.air_adam_step(ptr(b.p.t), ptr(b.g.t), ptr(b.m.t), ptr(b.v.t), ctypes.c_size_t(0), 1, *(
        ctypes.c_float(ADAM_DEFAULT[k]) for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "grad_scale")), stream()),
       "air_adam_step(n=0)")
    for step in (0, -1):
        with pytest.raises(hip().AirError, match="AIR_EINVAL"):
            ops.adam_step(b.p.t, b.g.t, b.m.t, b.v.t, step)
    assert_bits(b.p.t, p, "p after the no-op and the refused calls")
    assert not b.m.np().any() and not b.v.np().any()
    for buf in (b.p, b.g, b.m, b.v):
        buf.check("air_adam_step edge cases")


SGD_N = ADAM_N + [4096 * 256 + 77]  # blocks are capped at 4096 x 256 threads: the last size walks the stride loop


def sgd_ref64(p, g, lr, grad_scale):
    p, g = p.astype(np.float64), g.astype(np.float64)
    p1 = p - f32(lr) * (g * f32(grad_scale))
    return p1, 2.0 * EPS32 * (np.abs(p1) + np.abs(f32(lr) * g))


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("n", SGD_N)
def test_sgd_sizes(L, ops, n, grad_scale):
    p, g = synth_feat((n,), 1).numpy(), synth_feat((n,), 2).numpy()
    for shift in (0, 1):
        pb, gb = Guarded(n, shift=shift, value=p), Guarded(n, value=g)
        ops.sgd_step(pb.t, gb.t, 5e-4, grad_scale=grad_scale)
        pb.check("air_sgd_step / p")
        gb.check("air_sgd_step / g")
        assert_bits(gb.t, g, "air_sgd_step must not write g")
        want, tol = sgd_ref64(p, g, 5e-4, grad_scale)
        got = pb.np()
        d = np.abs(got.astype(np.float64) - want)
        bad = np.flatnonzero(~(d <= tol))
        assert bad.size == 0, "air_sgd_step(n=%d, grad_scale=%g): p[%d] = %r, fp64 %r" % (
            n, grad_scale, bad[0], got[bad[0]], want[bad[0]])
    ok(L.air_sgd_step(ptr(pb.t), ptr(gb.t), ctypes.c_size_t(0), ctypes.c_float(5e-4), ctypes.c_float(1.0), stream()),
       "air_sgd_step(n=0)")  # a no-op
    assert_bits(pb.t, got, "p after the n = 0 call")


def test_fused_sgd_noncontiguous_grad(ops):
    """FusedSGD.step with a transposed view as .grad gives the update of the same gradient laid out densely."""
    from asvspoof2021_air_amd.optim import FusedSGD
    w0 = synth_feat((5, 7), 1)
    gt = synth_feat((7, 5), 2).cuda()  # .t() of this is the (5, 7) gradient, non-contiguous
    res = []
    for grad in (gt.t(), gt.t().contiguous()):
        mod = torch.nn.Module()
        mod.w = torch.nn.Parameter(w0.clone().cuda())
        mod.w.grad = grad
        assert mod.w.grad.is_contiguous() == (len(res) == 1)
        FusedSGD(mod, lr=1e-2).step(grad_scale=0.5)
        res.append(mod.w.data.cpu())
    assert torch.equal(res[0], res[1])
    want, tol = sgd_ref64(w0.numpy().ravel(), gt.t().cpu().numpy().ravel(), 1e-2, 0.5)
    assert np.all(np.abs(res[0].numpy().ravel().astype(np.float64) - want) <= tol)
    assert_bits(gt.t().contiguous(), synth_feat((7, 5), 2).t().contiguous(), "the gradient is left alone")


# ---------------------------------------------------------------------------------------------- softmax cross-entropy
CE_SHAPES = [(1, 1), (1, 2), (7, 10), (255, 3), (256, 2), (257, 2), (700, 128), (33, 31)]
CE_SETS = ["synth", "shifted", "span", "ties"]
CE_PROBS_ATOL = 4 * EPS32
CE_LOSS_RTOL = 1e-6


def ce_case(B, C, kind):
    """float32 logits (B, C) and int64 labels (B,) that include 0 and C - 1."""
    gen = torch.Generator().manual_seed(1000 * B + C)
    x = 2.0 * torch.randn(B, C, generator=gen)
    labels = (torch.arange(B) * 5 + 1) % C
    if kind == "shifted":  # a shift-free exp overflows (+1e4) or underflows to 0 / 0 (-1e4)
        x = x + torch.tensor([1e4, -1e4, 0.0])[torch.arange(B) % 3][:, None]
    elif kind == "span":
        x = torch.rand(B, C, generator=gen) * 180.0 - 90.0
        x[:, 0] = 90.0 - 180.0 * (torch.arange(B) % 2)  # every row reaches an end of [-90, 90]
        if C > 1:
            x[:, C - 1] = -x[:, 0]
    elif kind == "ties":  # the row maximum sits at two known, different positions (C = 1 has only one)
        x = torch.round(x * 2.0) / 2.0
        top = x.max(dim=1).values + 1.0
        first = torch.arange(B) % C
        second = (first + 1 + (torch.arange(B) // C) % max(C - 1, 1)) % C
        x[torch.arange(B), first] = top
        x[torch.arange(B), second] = top
        lo, hi = torch.minimum(first, second), torch.maximum(first, second)
        # three rows in four are labelled with the first of the two, one with the last: "last maximum wins" counts
        # differently
        labels = torch.where(torch.arange(B) % 4 == 3, hi, lo)
    labels[0] = 0 if B > 1 else C - 1
    labels[-1] = C - 1
    return x.float().contiguous(), labels.to(torch.int64)


def first_maximum_hits(x, labels, last=False):
    """#rows whose FIRST maximum is the label, written out (no argmax: its tie rule is what is under test).
    ``last``: the count under the wrong rule, to show that the case tells the two apart."""
    hits = 0
    for row, lab in zip(x.tolist(), labels.tolist()):
        best, at = row[0], 0
        for c in range(1, len(row)):
            if row[c] > best or (last and row[c] == best):
                best, at = row[c], c
        hits += at == lab
    return hits


@pytest.mark.parametrize("kind", CE_SETS)
@pytest.mark.parametrize("B,C", CE_SHAPES)
def test_softmax_ce(L, B, C, kind):
    x, labels = ce_case(B, C, kind)
    what = "air_softmax_ce(B=%d, C=%d, %s)" % (B, C, kind)
    x64 = x.double().requires_grad_(True)
    loss64 = F.cross_entropy(x64, labels)
    loss64.backward()
    probs64 = torch.log_softmax(x64.detach(), dim=1).exp().numpy()
    if kind == "ties":
        assert int((x == x.max(dim=1, keepdim=True).values).sum(dim=1).max()) == min(2, C)
        assert C == 1 or first_maximum_hits(x, labels) != first_maximum_hits(x, labels, last=True)

    xg, lg = x.cuda(), labels.cuda()
    probs, loss, correct = Guarded(B * C), Guarded(1), Guarded(1, dtype=torch.int32)
    correct.set(-5)
    ok(L.air_softmax_ce_fwd(ptr(xg), ptr(lg), B, C, ptr(probs.t), ptr(loss.t), ptr(correct.t), stream()), what)
    for buf, name in ((probs, "probs"), (loss, "loss"), (correct, "correct")):
        buf.check("%s / %s" % (what, name))
    got = probs.np().reshape(B, C)
    assert np.isfinite(got).all() and np.isfinite(loss.t.item()), what
    err = np.abs(got.astype(np.float64) - probs64).max()
    lerr = abs(loss.t.item() - loss64.item())
    assert err <= CE_PROBS_ATOL, "%s: probs off by %.3g" % (what, err)
    assert lerr <= CE_LOSS_RTOL * abs(loss64.item()), "%s: loss %r, fp64 %r" % (what, loss.t.item(), loss64.item())
    assert correct.t.item() == first_maximum_hits(x, labels), what

    # correct = NULL: the same probs and loss, nothing else
    probs2, loss2 = Guarded(B * C), Guarded(1)
    ok(L.air_softmax_ce_fwd(ptr(xg), ptr(lg), B, C, ptr(probs2.t), ptr(loss2.t), ctypes.c_void_p(0), stream()), what)
    probs2.check(what + " / probs, correct = NULL")
    loss2.check(what + " / loss, correct = NULL")
    assert_bits(probs2.t, probs.t, what + ": probs with correct = NULL")
    assert_bits(loss2.t, loss.t, what + ": loss with correct = NULL")

    # backward from the kernel's own probs: gscale = NULL, then a device scalar 0.25
    d1, d2 = Guarded(B * C), Guarded(B * C)
    quarter = torch.full((1,), 0.25, device="cuda")
    ok(L.air_softmax_ce_bwd(ptr(probs.t), ptr(lg), B, C, ctypes.c_void_p(0), ptr(d1.t), stream()), what + " bwd")
    ok(L.air_softmax_ce_bwd(ptr(probs.t), ptr(lg), B, C, ptr(quarter), ptr(d2.t), stream()), what + " bwd")
    d1.check(what + " / dlogits")
    d2.check(what + " / dlogits, gscale = 0.25")
    g1, g2 = d1.np(), d2.np()
    derr = np.abs(g1.astype(np.float64) - x64.grad.numpy().ravel()).max()
    assert derr <= 4 * EPS32 / B, "%s: dlogits off by %.3g" % (what, derr)
    quarter_of_g1 = np.float32(0.25) * g1
    assert np.all(np.abs(g2 - quarter_of_g1) <= np.spacing(np.abs(quarter_of_g1))), what + ": gscale = 0.25"


def test_cross_entropy_module(adv):
    """The nn.Module in front of the two kernels: loss, gradient and the accuracy counter."""
    B, C = 33, 31
    x, labels = ce_case(B, C, "ties")
    x64 = x.double().requires_grad_(True)
    loss64 = F.cross_entropy(x64, labels)
    loss64.backward()
    crit = adv.CrossEntropyLoss()
    xg = x.cuda().requires_grad_(True)
    loss = crit(xg, labels.cuda())
    (loss * 0.25).backward()
    assert abs(loss.item() - loss64.item()) <= CE_LOSS_RTOL * abs(loss64.item())
    assert np.abs(xg.grad.cpu().double().numpy() - 0.25 * x64.grad.numpy()).max() <= 4 * EPS32 / B
    assert crit.last_correct.item() == first_maximum_hits(x, labels)


# ---------------------------------------------------------------------------------------------- elementwise helpers
EW_N = [1, 255, 256, 257, 70001]


def ew_inputs(n):
    """x with -0.0 and 0.0 in it, and a dropout keep-mask (0 or 1 / 0.7), so that x * keep covers negative * keep,
    negative * 0 = -0.0 and 0 * keep."""
    x = synth_feat((n,), 21).numpy().copy()
    x[0::7] = -0.0
    x[3::11] = 0.0
    if n > 5:
        x[5] = -abs(x[5]) - 1.0
    keep = po.dropout_keep(n, 0.3, 5, 0)
    if n > 5:
        keep[5] = keep.max() if keep.max() > 0 else np.float32(1.0) / np.float32(0.7)  # negative * keep
    return x, keep


def relu32(a):
    return np.where(a > 0, a, np.float32(0.0)).astype(np.float32)


@pytest.mark.parametrize("masked", [True, False], ids=["keep", "nokeep"])
@pytest.mark.parametrize("n", EW_N)
def test_mask_relu_fwd_bwd(L, adv, n, masked):
    x, keep = ew_inputs(n)
    xg, kg = torch.from_numpy(x).cuda(), (torch.from_numpy(keep).cuda() if masked else None)
    kp = ptr(kg) if masked else ctypes.c_void_p(0)
    want_y = relu32(x * keep if masked else x)
    y = Guarded(n)
    ok(L.air_mask_relu_fwd(ptr(xg), kp, ctypes.c_size_t(n), ptr(y.t), stream()), "air_mask_relu_fwd")
    y.check("air_mask_relu_fwd(n=%d)" % n)
    assert_bits(y.t, want_y, "air_mask_relu_fwd(n=%d, %s)" % (n, "keep" if masked else "no keep"))
    assert_bits(adv._mask_relu_fwd(xg, kg), want_y, "adversarial._mask_relu_fwd(n=%d)" % n)

    dy = synth_feat((n,), 22).numpy()
    dyg = torch.from_numpy(dy).cuda()
    for alpha in (1.0, -0.05):
        what = "air_mask_relu_bwd(n=%d, alpha=%g, %s)" % (n, alpha, "keep" if masked else "no keep")
        prod = (np.float32(alpha) * dy) * (keep if masked else np.float32(1.0))  # two fp32 products, in this order
        want = np.where(want_y > 0, prod, np.float32(0.0)).astype(np.float32)
        dx = Guarded(n)
        ok(L.air_mask_relu_bwd(ptr(dyg), ptr(y.t), kp, ctypes.c_size_t(n), ctypes.c_float(alpha), ptr(dx.t), stream()), what)
        dx.check(what)
        assert_bits(dx.t, want, what)
        assert not bits(dx.t)[want_y == 0].any(), what + ": dx must be exactly +0 where y == 0"
        assert_bits(adv._mask_relu_bwd(dyg, y.t, kg, alpha), want, "adversarial._mask_relu_bwd" + what[17:])


@pytest.mark.parametrize("n", EW_N)
def test_scale_and_mul(ops, adv, n):
    x, keep = ew_inputs(n)
    for alpha in (-0.05, 0.3):
        buf = Guarded(n, value=x)
        assert adv.scale_(buf.t, alpha) is buf.t
        buf.check("air_scale(n=%d)" % n)
        assert_bits(buf.t, x * np.float32(alpha), "air_scale(n=%d, alpha=%g)" % (n, alpha))
    b = synth_feat((n,), 23).numpy()
    out = Guarded(n)
    xg, bg = torch.from_numpy(x).cuda(), torch.from_numpy(b).cuda()
    assert ops.mul(xg, bg, out=out.t) is out.t
    out.check("air_mul(n=%d)" % n)
    assert_bits(out.t, x * b, "air_mul(n=%d)" % n)
    assert_bits(ops.mul(xg, bg), x * b, "ops.mul(n=%d) without out=" % n)
    assert_bits(xg, x, "air_mul must not write a")
    assert_bits(bg, b, "air_mul must not write b")


@pytest.mark.parametrize("n", EW_N)
def test_copy_pad(L, ops, n):
    for n_src in sorted({n // 2, max(n - 1, 0), n, n + 5, 2 * n + 1}):
        what = "air_copy_pad(n_dst=%d, n_src=%d)" % (n, n_src)
        src = synth_feat((n_src + 1,), 24).numpy()[:n_src]
        sb = Guarded(n_src, value=src)
        dst = Guarded(n, value=synth_feat((n,), 25).numpy() + 100.0)  # garbage: the zero fill must be seen
        if n_src:
            assert ops.copy_pad(dst.t, sb.t) is dst.t
        else:  # (an empty tensor has no pointer to hand over: the C symbol with a live one)
            ok(L.air_copy_pad(ptr(dst.t), ctypes.c_size_t(n), ptr(sb.raw), ctypes.c_size_t(0), stream()), what)
        dst.check(what)
        sb.check(what + " / src")
        want = np.zeros(n, np.float32)
        want[:min(n, n_src)] = src[:min(n, n_src)]
        assert_bits(dst.t, want, what)
        assert_bits(sb.t, src, what + " must not write src")


ADD_BIG = 8192 * 256 + 257  # the grid is capped at 8192 blocks: the stride loop takes a second trip over 257 elements


@pytest.mark.parametrize("n", EW_N + [ADD_BIG])
def test_add_inplace(L, ops, n):
    x, _ = ew_inputs(n)
    y = synth_feat((n,), 26).numpy()
    yb, xb = Guarded(n, shift=1, value=y), Guarded(n, value=x)
    assert ops.add_(yb.t, xb.t) is yb.t
    yb.check("air_add_inplace(n=%d) / y" % n)
    xb.check("air_add_inplace(n=%d) / x" % n)
    assert_bits(yb.t, y + x, "air_add_inplace(n=%d)" % n)
    assert_bits(xb.t, x, "air_add_inplace must not write x")
    ok(L.air_add_inplace(ptr(yb.t), ptr(xb.t), ctypes.c_size_t(0), stream()), "air_add_inplace(n=0)")  # a no-op
    assert_bits(yb.t, y + x, "y after the n = 0 call")
