"""GPU: the fused classifier heads (air_adv_heads, csrc/adv_head.hip) against oracle.adversarial in fp64, the in-kernel
dropout draw against air_dropout_mask, and the exactness / hygiene properties of the call."""
import functools

import numpy as np
import pytest
import torch

from oracle import adversarial as o_adv
from oracle.filler import fill_state, synth_feat

pytestmark = pytest.mark.gpu

LAMBDA = 0.7
NAMES = ("classifier.0.weight", "classifier.0.bias", "classifier.3.weight", "classifier.3.bias")
# (B, D, classes, seed of the masked run, seed of the unmasked run).  The seeds are the first (from 13 upwards) at
# which the fp64 oracle meets twice the margins asserted in reference() and keeps the all-zero rows: found on the CPU
# from the oracle alone, never from the kernel's output.
SHAPES = [
    (1, 256, (2,), 13, 13),
    (7, 256, (61,), 13, 13),
    (64, 256, (28, 11), 13, 14),
    (5, 6, (3,), 13, 13),
    (300, 256, (5,), 14, 23),
    (64, 2, (3,), 13, 13),
]
MARGIN = 1e-5
ZERO_ROWS = {(5, 6, (3,)), (300, 256, (5,))}  # shapes that must keep a row whose logits are all zero


def make_inputs(B, D, Cs, seed, masked):
    feats = synth_feat((B, D), seed)
    heads = []
    for k, C in enumerate(Cs):
        params = fill_state(o_adv.classifier_shapes(D, C))
        targets = (torch.arange(B) * 7 + seed) % C
        keep = None
        if masked:
            g = torch.Generator().manual_seed(seed * 100 + k)
            keep = (torch.rand(B, D // 2, generator=g) >= 0.3).float() / 0.7
        heads.append((params, targets, keep))
    return feats, heads


def margins(feats, heads):
    """On the fp64 oracle: the smallest distance of a live pre-activation from zero and of a row's top two logits from
    each other, both relative to their tensor's largest magnitude; and the number of all-zero rows per head."""
    worst, zero_rows = np.inf, []
    x = feats.double()
    for params, _, keep in heads:
        p = {k: v.double() for k, v in params.items()}
        pre1 = x @ p[NAMES[0]].T + p[NAMES[1]]
        live = torch.ones_like(pre1, dtype=torch.bool)
        if keep is not None:
            pre1 = pre1 * keep.double()
            live = keep > 0
        worst = min(worst, float(pre1[live].abs().min() / pre1.abs().max()))
        pre2 = torch.relu(pre1) @ p[NAMES[2]].T + p[NAMES[3]]
        worst = min(worst, float(pre2.abs().min() / pre2.abs().max()))
        o = torch.relu(pre2)
        allzero = (o == 0).all(1)
        zero_rows.append(int(allzero.sum()))
        if o.shape[1] > 1 and bool((~allzero).any()):
            top = o[~allzero].topk(2, dim=1).values
            worst = min(worst, float((top[:, 0] - top[:, 1]).min() / o.abs().max()))
    return worst, zero_rows


@functools.lru_cache(maxsize=None)
def reference(B, D, Cs, seed, masked):
    """fp64 oracle of one case, computed once and shared: (feats, heads, per-head (loss, grads, correct), dx)."""
    feats, heads = make_inputs(B, D, Cs, seed, masked)
    worst, zero_rows = margins(feats, heads)
    # no value is excluded from the comparison below, so no ReLU or argmax decision may be within rounding
    assert worst >= MARGIN, ("pick another seed", (B, D, Cs, seed, masked), worst)
    if (B, D, Cs) in ZERO_ROWS:
        assert min(zero_rows) >= 1, ("pick a seed that keeps an all-zero row", zero_rows)
    per_head, dx = [], torch.zeros(B, D, dtype=torch.float64)
    for params, targets, keep in heads:
        loss, logits, df, gr = o_adv.loss_and_grads({k: v.double() for k, v in params.items()}, feats.double(), targets,
                                                    LAMBDA, None if keep is None else keep.double())
        correct = int((logits.argmax(1) == targets).sum())  # torch: the first maximum; an all-zero row predicts 0
        zero = (logits == 0).all(1)
        assert correct == int(((logits.argmax(1) == targets) & ~zero).sum() + ((targets == 0) & zero).sum())
        per_head.append((float(loss), gr, correct))
        dx += df
    return feats, heads, per_head, dx


def gpu_heads(D, heads, p=0.0, seeds=None, counters=None):
    from asvspoof2021_air_amd import ops
    out = []
    for k, (params, _, _) in enumerate(heads):
        flat = torch.cat([params[n].reshape(-1) for n in NAMES]).cuda()
        grad = torch.full_like(flat, float("nan"))
        out.append(ops.AdvHead(flat, grad, params[NAMES[3]].numel(), p=p, seed=0 if seeds is None else seeds[k],
                               counter=None if counters is None else counters[k]))
    return out


def split(grad, D, C):
    H = D // 2
    sizes = (H * D, H, C * H, C)
    shapes = ((H, D), (H,), (C, H), (C,))
    return [t.view(s) for t, s in zip(grad.split(sizes), shapes)]


def close(got, ref, what):
    ref = ref.numpy() if torch.is_tensor(ref) else ref
    got = got.detach().cpu().double().numpy()
    bound = 5e-6 * np.abs(ref).max()
    err = np.abs(got - ref).max()
    print("%s: max err %.3g, bound %.3g" % (what, err, bound))
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("want_dx", [True, False])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("B,D,Cs,seed_m,seed_u", SHAPES)
def test_fused_heads_against_fp64_oracle(B, D, Cs, seed_m, seed_u, masked, want_dx):
    from asvspoof2021_air_amd import ops
    feats, heads, per_head, dx_ref = reference(B, D, Cs, seed_m if masked else seed_u, masked)
    hs = gpu_heads(D, heads)
    keeps = [h[2].cuda() for h in heads] if masked else None
    losses, correct, dx = ops.adv_heads(feats.cuda(), hs, [h[1].cuda() for h in heads], LAMBDA, want_dx, keeps=keeps)
    assert (dx is None) == (not want_dx)
    for k, (loss, gr, n_ok) in enumerate(per_head):
        np.testing.assert_allclose(float(losses[k]), loss, rtol=1e-5)
        assert int(correct[k]) == n_ok
        for got, name in zip(split(hs[k].grad, D, Cs[k]), NAMES):
            close(got, gr[name], "head %d %s" % (k, name))
    if want_dx:
        close(dx, dx_ref, "dx")


@pytest.mark.parametrize("B,D,Cs", [(5, 6, (3,)), (64, 256, (28, 11))])
def test_in_kernel_draw_is_the_dropout_mask(B, D, Cs):
    from asvspoof2021_air_amd import ops
    from asvspoof2021_air_amd.adversarial import dropout_mask
    feats, heads = make_inputs(B, D, Cs, 13, False)
    H, quads = D // 2, (B * (D // 2) + 3) // 4
    start, seeds = [1000 + 77 * k for k in range(len(Cs))], [4242 + k for k in range(len(Cs))]
    counters = [torch.tensor([c], dtype=torch.int64, device="cuda") for c in start]
    x, tg = feats.cuda(), [h[1].cuda() for h in heads]
    drawn = gpu_heads(D, heads, p=0.3, seeds=seeds, counters=counters)
    a = ops.adv_heads(x, drawn, tg, LAMBDA, True)
    assert [int(c) for c in counters] == [c + quads for c in start]
    given = gpu_heads(D, heads)
    keeps = [dropout_mask((B, H), 0.3, s, c, "cuda") for s, c in zip(seeds, start)]
    b = ops.adv_heads(x, given, tg, LAMBDA, True, keeps=keeps)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for u, v in zip(drawn, given):
        assert torch.equal(u.grad, v.grad)
    first = [h.grad.clone() for h in drawn]
    ops.adv_heads(x, drawn, tg, LAMBDA, True)  # the counters moved on: another mask
    assert [int(c) for c in counters] == [c + 2 * quads for c in start]
    assert all(not torch.equal(u, h.grad) for u, h in zip(first, drawn))


def test_dx_composition_is_exact_and_run_correct_accumulates():
    from asvspoof2021_air_amd import ops
    B, D, Cs = 64, 256, (28, 11)
    feats, heads = make_inputs(B, D, Cs, 13, True)
    x, tg, keeps = feats.cuda(), [h[1].cuda() for h in heads], [h[2].cuda() for h in heads]
    both = ops.adv_heads(x, gpu_heads(D, heads), tg, 1.0, True, keeps=keeps)[2]
    half = ops.adv_heads(x, gpu_heads(D, heads), tg, 0.5, True, keeps=keeps)[2]
    assert torch.equal(half, both * 0.5) and float(both.abs().max()) > 0
    singles = [ops.adv_heads(x, gpu_heads(D, heads[k:k + 1]), tg[k:k + 1], 1.0, True, keeps=keeps[k:k + 1])[2]
               for k in range(2)]
    assert torch.equal(both, singles[0] + singles[1])
    run = torch.tensor([5, 0], dtype=torch.int64, device="cuda")
    total = torch.tensor([5, 0], dtype=torch.int64)
    for i in range(3):
        tgi = [(t + i) % C for t, C in zip(tg, Cs)]
        _, correct, _ = ops.adv_heads(x, gpu_heads(D, heads), tgi, 1.0, False, keeps=keeps, run_correct=run)
        total += correct.cpu().long()
    assert torch.equal(run.cpu(), total) and int(total.sum()) > 5


def guarded(n, dtype=torch.float32, fill=float("nan")):
    """A buffer of n values between two rows of sentinels (the pattern of guarded_f32 in test_ecapa_bf16_gpu.py)."""
    sentinel = 1.2345678e7 if dtype.is_floating_point else 1234567
    raw = torch.full((n + 128,), sentinel, dtype=dtype, device="cuda")
    raw[64:64 + n] = fill

    def check(what):
        assert bool((raw[:64] == sentinel).all()), what + " wrote in front of its buffer"
        assert bool((raw[64 + n:] == sentinel).all()), what + " wrote behind its buffer"
    return raw[64:64 + n], check


@pytest.mark.parametrize("B,D,Cs", [(5, 6, (3,)), (64, 256, (28, 11)), (300, 256, (5,))])
def test_outputs_are_written_in_bounds_and_repeatable(B, D, Cs, monkeypatch):
    from asvspoof2021_air_amd import ops
    feats, heads = make_inputs(B, D, Cs, 13, True)
    x, tg, keeps = feats.cuda(), [h[1].cuda() for h in heads], [h[2].cuda() for h in heads]
    checks, real_empty = [], torch.empty

    def guarded_empty(*shape, device=None, dtype=torch.float32):
        if dtype == torch.uint8:  # (a scratch buffer, not an output)
            return real_empty(*shape, device=device, dtype=dtype)
        shape = tuple(shape[0]) if len(shape) == 1 and not isinstance(shape[0], int) else shape
        buf, check = guarded(int(np.prod(shape)), dtype, float("nan") if dtype.is_floating_point else -7)
        checks.append(check)
        return buf.view(shape)

    def run():
        hs = gpu_heads(D, heads)
        for h in hs:  # NaN-filled gradient blocks between sentinels
            buf, check = guarded(h.grad.numel())
            checks.append(check)
            h.grad = buf
        with monkeypatch.context() as mp:
            mp.setattr(torch, "empty", guarded_empty)  # losses, correct and dx of the call
            out = ops.adv_heads(x, hs, tg, LAMBDA, True, keeps=keeps)
        return out, hs

    (l1, c1, dx1), h1 = run()
    n_guards = len(checks)
    assert n_guards == 3 + len(Cs)
    (l2, c2, dx2), h2 = run()
    for check in checks:
        check("air_adv_heads")
    for t in (l1, dx1) + tuple(h.grad for h in h1):
        assert bool(torch.isfinite(t).all())
    assert bool((c1 >= 0).all())
    assert torch.equal(l1, l2) and torch.equal(c1, c2) and torch.equal(dx1, dx2)
    assert all(torch.equal(u.grad, v.grad) for u, v in zip(h1, h2))
