#!/usr/bin/env python3
"""What one sort for all groups buys (profiles/eval_groups.md).  At each (n trials, G groups), both score polarities:

  grouped    ops.eval_det_min_grouped: pooled + G group records from one sort per polarity
  per_group  the alternative on the device: G + 1 ungrouped ops.eval_det_min calls per polarity on subsets that were
             compacted BEFORE the clock started (a lower bound: the compaction, with its synchronising size read, is
             not counted)
  host       eval_metrics.compute_eer_by_group on both polarities (numpy, scores already on the host)

The device sides are timed with events around windows of back-to-back calls (workspaces and records preallocated, the
window long enough for ``--window-ms``), after a warm-up of every shape, the two sides alternating window by window; the
figure is the median window with min .. max.  Modes: "attack" (bona fide trials belong to every group) at G = 13,
"partition" (codec x attack conditions) otherwise.  The grouped records are checked against the per-group ones first.

Usage: python tools/bench_eval_groups.py [--windows 7] [--window-ms 250] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from asvspoof2021_air_amd import eval_metrics as em, ops  # noqa: E402


def make(n, G, mode):
    rng = np.random.default_rng(n + G)
    lab = (rng.random(n) < 0.9).astype(np.int64)
    s = (rng.normal(0, 1, n) + np.where(lab == 0, 1.0, -1.0)).astype(np.float32)
    grp = rng.integers(0, G, n).astype(np.int64)
    if mode == "attack":
        grp[lab == 0] = -1
    return s, lab, grp


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def timed(args, **variants):
    reps = {}
    for k, fn in variants.items():  # warm-up, and a pilot window to size the timed ones
        fn()
        torch.cuda.synchronize()
        reps[k] = max(2, min(2000, int(args.window_ms / max(window_ms(fn, 2), 1e-3))))
    out = {k: [] for k in variants}
    for _ in range(args.windows):
        for k, fn in variants.items():
            out[k].append(window_ms(fn, reps[k]))
    return {k: {"median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v), "calls_per_window": reps[k]}
            for k, v in out.items()}


def bench(n, G, mode, args):
    s, lab, grp = make(n, G, mode)
    ds, dl, dg = (torch.from_numpy(a).cuda() for a in (s, lab, grp))
    recs = torch.empty(2, G + 1, ops.EVAL_RECORD_WORDS, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.eval_workspace_bytes_grouped(n, G), dtype=torch.uint8, device="cuda")
    subsets = [(ds, dl)]
    for g in range(G):
        m = torch.from_numpy((grp == g) | (grp == -1)).cuda()
        subsets.append((ds[m].contiguous(), dl[m].contiguous()))
    recs1 = torch.empty(2, G + 1, ops.EVAL_RECORD_WORDS, dtype=torch.int32, device="cuda")
    ws1 = torch.empty(ops.eval_workspace_bytes(n), dtype=torch.uint8, device="cuda")

    def grouped():
        for p in (0, 1):
            ops.eval_det_min_grouped(ds, dl, dg, G, recs[p], ws, negate=bool(p))

    def per_group():
        for p in (0, 1):
            for r, (sub_s, sub_l) in enumerate(subsets):
                ops.eval_det_min(sub_s, sub_l, recs1[p, r], ws1, negate=bool(p))

    grouped()
    per_group()
    a, b = recs.cpu().numpy()[..., :14], recs1.cpu().numpy()[..., :14]  # (the two reserved words aside)
    assert np.array_equal(a, b), "the grouped records differ from the per-group ones"
    s64 = s.astype(np.float64)
    t0 = time.perf_counter()
    host = [em.compute_eer_by_group(sg * s64, lab, grp, G) for sg in (1.0, -1.0)]
    host_ms = (time.perf_counter() - t0) * 1e3
    got = em.DeviceGroupedMinima(ds, dl, dg, G, (False, True))
    assert [[got.eer(p, g) for g in range(G)] for p in (0, 1)] == host
    row = dict(n=n, G=G, mode=mode, host_ms=host_ms, **timed(args, grouped=grouped, per_group=per_group))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    rows = [bench(n, G, mode, args) for n, G, mode in ((71237, 13, "attack"), (611829, 91, "partition"),
                                                       (1 << 20, ops.EVAL_MAX_GROUPS, "partition"))]
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
