"""Times the RawBoost augmentation (augment.rawboost, profiles/rawboost.md) in one process.

  python tools/bench_rawboost.py [--windows 5] [--calls 32] [--no-step]

B = 64 rows of 64 000 samples (4 s), fp32 and int16, every row on the same algorithm: the design launch alone, then
algorithms 0 - 7 and the default mix (0, 1, 2).  Two yardsticks from the same run on the same batch: ir_convolve (1024
taps, ragged entry point, peak rescale) and g711_codec.  Then the ResNet-18 train step (B = 64, feat_len 750, hipGraph
replay) without an augmenter - the step's code is the one of the commit before RawBoost - and with RawBoostAugment in
front of it.  Protocol of profiles/device_corpus.md: per figure one warm-up window, then ``--windows`` windows of
``--calls`` back-to-back calls between two device events, median (min .. max) per call; the figures of one group
alternate window by window."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asvspoof2021_air_amd.augment import (RawBoostAugment, g711_codec, ir_convolve, rawboost, rawboost_design,  # noqa: E402
                                          synthetic_ir_bank)

B, L = 64, 64000


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3  # us per call


def measure(variants, args):
    times = {k: [] for k in variants}
    for w in range(args.windows + 1):
        for k, fn in variants.items():
            us = window(fn, args.calls)
            if w >= 1:
                times[k].append(us)
    for k, us in times.items():
        print("%-46s median %9.1f us  (%9.1f .. %9.1f)" % (k, statistics.median(us), min(us), max(us)), flush=True)
    return {k: statistics.median(us) for k, us in times.items()}


def trainers():
    from asvspoof2021_air_amd.resnet import ResNet
    from asvspoof2021_air_amd.train import Trainer
    out = {}
    for name, aug in (("ResNet-18 step, no augmenter", None),
                      ("ResNet-18 step + RawBoostAugment(0, 1, 2)", RawBoostAugment(seed=1)),
                      ("ResNet-18 step + RawBoostAugment(3)", RawBoostAugment(algos=(3,), seed=1))):
        torch.manual_seed(688)
        tr = Trainer(ResNet(3, 256, resnet_type="18", nclasses=2), enc_dim=256, lr=5e-4, r_real=0.9, r_fake=0.2, alpha=20.0,
                     feat_len=750, augment=aug)
        tr.enable_graph()
        out[name] = tr
    return out


def main(args):
    g = torch.Generator().manual_seed(1)
    x = (0.1 * torch.randn(B, L, generator=g)).cuda()
    x16 = (x * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
    full = torch.full((B,), L, dtype=torch.int32, device="cuda")
    y = torch.empty(B, L, device="cuda")
    tables = {}
    for a in list(range(8)) + ["mix"]:
        aug = RawBoostAugment(algos=(0, 1, 2) if a == "mix" else (a,), seed=2)
        tables[a] = torch.from_numpy(aug.params(aug.draw(B))).cuda()
    lens = rawboost_design(tables[3])[1].cpu().numpy()
    print("B = %d, L = %d; cascade lengths of algorithm 3's table: mean %.0f, max %d taps" % (
        B, L, lens[lens > 0].mean(), lens.max()), flush=True)
    variants = {"air_rawboost_design (6 B filters)": lambda: rawboost_design(tables[3])}
    for tname, t in (("fp32", x), ("int16", x16)):
        for a, tab in tables.items():
            variants["rawboost %-5s algo %s" % (tname, a)] = lambda t=t, tab=tab: rawboost(t, tab, out=y)
    irs = synthetic_ir_bank().cuda()
    idx = (torch.arange(B, device="cuda", dtype=torch.int32) % irs.shape[0])
    law = (torch.arange(B, device="cuda", dtype=torch.int32) % 2)
    variants["ir_convolve int16 (1024 taps, ragged entry)"] = lambda: ir_convolve(x16, irs, idx, True, out=y, lengths=full)
    variants["ir_convolve fp32  (1024 taps, ragged entry)"] = lambda: ir_convolve(x, irs, idx, True, out=y, lengths=full)
    variants["g711_codec  int16"] = lambda: g711_codec(x16, law, lengths=full, out=y)
    variants["g711_codec  fp32"] = lambda: g711_codec(x, law, lengths=full, out=y)
    measure(variants, args)
    if args.no_step:
        return
    lab = (torch.arange(B) % 2).cuda()
    trs = trainers()
    for tr in trs.values():
        for _ in range(5):  # two eager steps, the capture, two replays
            loss = tr.step(x, lab)[0]
        assert tr._graph is not None and bool(torch.isfinite(loss))
    measure({k: (lambda tr=tr: tr.step(x, lab)) for k, tr in trs.items()}, args)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=32)
    ap.add_argument("--no-step", action="store_true")
    if not torch.cuda.is_available():
        sys.exit("bench_rawboost.py needs a GPU: there is nothing to measure without one")
    main(ap.parse_args())
