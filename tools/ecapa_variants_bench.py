"""Times the bf16-resident train step of the four ``Res2Net2(context=, summed=)`` combinations in one process
(profiles/ecapa_variants_bf16.md).

  python tools/ecapa_variants_bench.py [--rounds 12] [--reps 40] [--out profiles/ecapa_variants_bf16.md]

bench.py's ECAPA leg for each of them: B = 128 utterances of 4 s, LFCC -> repeat-pad to feat_len 750 -> ECAPA-TDNN-512
-> OC-Softmax -> backward -> Adam, ``set_compute_dtype("bf16", variants=True)``, hipGraph replay.  A-B-A against the
default options: every round times ctsf, one variant, ctsf again, the next variant, ... so each variant sits between
two readings of the default taken seconds apart, and the figure reported is the variant's step time over the mean of its
two neighbours, median over the rounds.  Device events around ``reps`` back-to-back steps (0.3 s per window); the first
round only warms up (with four captured steps side by side the next four rounds were disturbed too, for all models
alike: hence twelve rounds and medians, and every window is printed).  One clock / power sample of the part (bench.smi_sample) in front of and behind the timed rounds.
The four models (4 x 25 MB of parameters, 4 captured graphs with their private pools) live side by side."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, L, FEAT_LEN = 128, 64000, 750
TAGS = [("ctsf", True, False), ("cfsf", False, False), ("ctst", True, True), ("cfst", False, True)]
TENSOR_MB = 128 * 512 * 768 * 2 / 1e6  # one (128, 512, Tp = 768) bf16 tensor


def events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps  # ms per step


def make(context, summed, pcm, lab):
    from asvspoof2021_air_amd.ecapa_tdnn import Bottle2neck, Res2Net2
    from asvspoof2021_air_amd.train import Trainer
    torch.manual_seed(688)
    model = Res2Net2(Bottle2neck, C=512, model_scale=8, nOut=2, n_mels=60, context=context, summed=summed)
    model.set_compute_dtype("bf16", variants=True)
    tr = Trainer(model, enc_dim=256, lr=5e-4, r_real=0.9, r_fake=0.2, alpha=20.0, feat_len=FEAT_LEN, ecapa=True)
    tr.enable_graph()
    for _ in range(5):  # two eager steps, the capture, two replays
        loss = tr.step(pcm, lab)[0]
    assert tr._graph is not None and bool(torch.isfinite(loss)), "no captured step"
    return tr


def kernel_rows(reps=50):
    """The row passes the options add or replace, alone, at the step's shapes: us per call (median of 5 windows) and the
    bytes each must move (operands read once, outputs written once) over that time."""
    from asvspoof2021_air_amd import ops_h as oh
    T, C = FEAT_LEN, 512
    new = lambda c: torch.randint(-2 ** 14, 2 ** 14, (B, c, oh.tp(T)), dtype=torch.int16, device="cuda")
    x, r, o, s2 = new(C), new(C), new(C), new(C)
    wide = new(3 * C)
    z = torch.zeros((B, C), device="cuda")
    x4, dx4 = new(1536), new(1536)
    f4 = torch.zeros((B, 1536), device="cuda")
    one4, rs4 = f4 + 1, f4.clone()
    one = B * C * oh.tp(T) * 2
    cases = [("se_scale_fwd (default)", lambda: oh.se_scale_fwd(x, z, r, T, wide[:, :C]), 3 * one),
             ("se_scale_fwd_sum (summed: + the running sum)", lambda: oh.se_scale_fwd_sum(x, z, r, T, wide[:, :C], s2), 4 * one),
             ("add in place over a concat slice (summed backward)", lambda: oh.add(wide[:, C:2 * C], o, T, out=wide[:, C:2 * C]), 3 * one),
             ("row_stats_bwd + mask + row sums (default)", lambda: oh.row_stats_bwd(x4, T, f4, one4, f4, f4, dx4, relu_mask=True, rowsum=rs4), 9 * one),
             ("relu_mask_rowsum (context=False)", lambda: oh.relu_mask_rowsum(x4, T, dx4, rowsum=rs4), 9 * one)]
    out = ["| row pass, B = 128, T = 750 | us / call | GB moved | TB/s |", "|---|---|---|---|"]
    for name, fn, nbytes in cases:
        events(fn, reps)
        us = statistics.median([events(fn, reps) for _ in range(5)]) * 1e3
        out.append("| %s | %.1f | %.3f | %.2f |" % (name, us, nbytes / 1e9, nbytes / us / 1e6))
    return out


def main(args):
    import bench
    g = torch.Generator().manual_seed(10)
    pcm = (0.1 * torch.randn(B, L, generator=g)).cuda()
    lab = (torch.rand(B, generator=g) < 0.9).long().cuda()
    tr = {tag: make(c, s, pcm, lab) for tag, c, s in TAGS}
    step = {tag: (lambda t=t: t.step(pcm, lab)) for tag, t in tr.items()}
    smi = [bench.smi_sample()]
    base, var, ratio = [], {t: [] for t, _, _ in TAGS[1:]}, {t: [] for t, _, _ in TAGS[1:]}
    raw = []
    for r in range(args.rounds + 1):
        a = events(step["ctsf"], args.reps)
        if r >= 1:
            raw.append([a])
        for tag, _, _ in TAGS[1:]:
            v = events(step[tag], args.reps)
            a2 = events(step["ctsf"], args.reps)
            if r >= 1:
                var[tag].append(v)
                ratio[tag].append(v / (0.5 * (a + a2)))
                base.append(a)
                raw[-1] += [v, a2]
            a = a2
        if r >= 1:
            base.append(a)
    smi.append(bench.smi_sample())
    med = statistics.median
    lines = ["| options | ms / step (median, min - max) | utt/s | step time over the default's (A-B-A, median, min - max) |",
             "|---|---|---|---|",
             "| ctsf (context=True, summed=False: the default) | %.2f (%.2f - %.2f) | %.0f | 1 (spread of its own readings: %.2f %%) |" % (
                 med(base), min(base), max(base), B * 1e3 / med(base), 100.0 * (max(base) - min(base)) / med(base))]
    for tag, c, s in TAGS[1:]:
        lines.append("| %s (context=%s, summed=%s) | %.2f (%.2f - %.2f) | %.0f | %.4f (%.4f - %.4f) |" % (
            tag, c, s, med(var[tag]), min(var[tag]), max(var[tag]), B * 1e3 / med(var[tag]), med(ratio[tag]),
            min(ratio[tag]), max(ratio[tag])))
    lines += ["", "B = %d, %d samples, feat_len %d, hipGraph replay, %d rounds of %d steps per window behind one warm-up round; one "
              "(128, 512, 768) bf16 tensor = %.1f MB." % (B, L, FEAT_LEN, args.rounds, args.reps, TENSOR_MB),
              "", "Clock / power samples of the part (in front of the timed rounds, behind them):", ""]
    lines += ["    " + json.dumps(s) for s in smi]
    lines += ["", "Every window, ms / step, in the order timed (a round = ctsf, cfsf, ctsf, ctst, ctsf, cfst, ctsf):", ""]
    lines += ["    " + " ".join("%.2f" % v for v in row) for row in raw]
    lines += [""] + kernel_rows()
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default="", help="also write the table to this file")
    if not torch.cuda.is_available():
        sys.exit("ecapa_variants_bench.py needs a GPU: there is nothing to measure without one")
    main(ap.parse_args())
