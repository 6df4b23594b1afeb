#!/usr/bin/env python3
"""What fusing on the device and scoring K systems in one pass cost (profiles/score_fusion.md).  One process on one GPU;
every section first asserts that its sides give the same result (bits of the fused scores, bytes of the files).

  fuse      K = 3 systems, N = 71,237 trials (the 2019 LA evaluation set), scores resident on the GPU:
            ops.score_fuse alone (device events over ``--iters`` back-to-back launches) and score_fusion.fuse_device -
            fusion, the K systems' and the fused EERs, result on the host - for "avg", "wght" with given EERs (one copy)
            and "wght" from the systems' own EERs (two copies); beside them the host port on the same scores
            (score_fusion.avg_fuse over ScoreFrames: the join and the numpy accumulation) plus host eer_both_polarities.
  ensemble  generate_score.test_on_dataset_ensemble over a loader of N trials in batches of ``--batch`` host feature
            tensors (B, 1, 750, 60) against what a user ran before: K separate test_on_dataset(..., sync="end") passes over
            the same loader (that function is unchanged by the ensemble pass) followed by score_fusion.avg_fuse over the K
            files.  The three systems are the ECAPA-TDNN-512 variants of the reference's shipped score files
            (context / summed), bf16-resident, with OC-softmax heads.

Median of ``--runs`` timed runs (min .. max), the sides alternating run by run behind one warm-up each; a host clock
around work that ends in a device synchronise.

Usage: python tools/bench_fusion.py [--what fuse,ensemble] [--runs 5] [--trials 71237] [--batch 64] [--iters 200] [--json out.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from asvspoof2021_air_amd import eval_metrics as em, ops, score_fusion as sf  # noqa: E402

K = 3


def timed(runs, **variants):
    for fn in variants.values():
        fn()
    out = {k: [] for k in variants}
    for _ in range(runs):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[k].append(time.perf_counter() - t0)
    return {k: {"median_s": float(np.median(v)), "min_s": min(v), "max_s": max(v)} for k, v in out.items()}


def bench_fuse(args):
    n = args.trials
    rng = np.random.default_rng(n)
    lab = (rng.random(n) < 0.9).astype(np.int64)
    host = (rng.normal(0, 1, (K, n)) + np.where(lab == 0, 1.0, -1.0)).astype(np.float32)
    names = ["LA_E_%07d" % i for i in rng.permutation(10 ** 7)[:n]]
    keys = ["spoof" if x else "bonafide" for x in lab]
    frames = [sf.ScoreFrame(names, ["-"] * n, keys, host[k]) for k in range(K)]
    dev, dlab = torch.from_numpy(host).cuda(), torch.from_numpy(lab).cuda()
    eers = [0.228, 0.237, 0.197]
    want = sf.avg_fuse(frames)
    got = sf.fuse_device(dev, dlab, "avg")
    order = np.argsort(names)
    assert np.array_equal(got.scores.cpu().numpy()[order].view(np.uint32), want.score.view(np.uint32))
    assert got.eer == sf.fused_eer(want.key, want.score)

    def host_side():
        f = sf.avg_fuse(frames)
        return sf.fused_eer(f.key, f.score), [em.eer_both_polarities(fr.score.astype(np.float64), lab) for fr in frames]

    row = dict(what="fuse", K=K, n=n, **timed(
        args.runs, host_avg_fuse_and_eers=host_side,
        fuse_device_avg=lambda: sf.fuse_device(dev, dlab, "avg"),
        fuse_device_wght_given_eers=lambda: sf.fuse_device(dev, dlab, "wght", eers),
        fuse_device_wght_own_eers=lambda: sf.fuse_device(dev, dlab, "wght")))
    out = torch.empty(n, device="cuda")
    weights = torch.tensor(eers, device="cuda")
    for name, kw in (("kernel_sum_us", dict(mode="sum")), ("kernel_weighted_mean_us", dict(mode="mean", weights=weights))):
        for _ in range(10):
            ops.score_fuse(dev, out=out, **kw)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            ops.score_fuse(dev, out=out, **kw)
        b.record()
        torch.cuda.synchronize()
        row[name] = a.elapsed_time(b) * 1e3 / args.iters  # (back-to-back launches: launch rate or kernel, whichever is longer)
    print(json.dumps(row), flush=True)
    return [row]


def bench_ensemble(args):
    from asvspoof2021_air_amd.ecapa_tdnn import Bottle2neck, Res2Net2
    from asvspoof2021_air_amd.generate_score import test_on_dataset, test_on_dataset_ensemble
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    n, B = args.trials, args.batch
    models, heads = [], []
    for i, (context, summed) in enumerate(((False, True), (True, False), (True, True))):  # cfst, ctsf, ctst
        torch.manual_seed(688 + i)
        m = Res2Net2(Bottle2neck, C=512, model_scale=8, nOut=2, n_mels=60, context=context, summed=summed).cuda()
        models.append(m.set_compute_dtype("bf16", variants=True).eval())
        heads.append(AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0).cuda())
    g = torch.Generator().manual_seed(3)
    pool = [torch.randn(B, 1, 750, 60, generator=g) for _ in range(8)]  # host tensors, as a DataLoader yields them
    labels = torch.from_numpy((np.random.default_rng(4).random(n) < 0.9).astype(np.int64))
    names = ["LA_E_%07d" % i for i in range(n)]
    data = [(pool[(i // B) % 8][:min(B, n - i)], names[i:i + B], None, labels[i:i + B]) for i in range(0, n, B)]
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        single = [os.path.join(tmp, "single%d.txt" % k) for k in range(K)]
        ens = [os.path.join(tmp, "ens%d.txt" % k) for k in range(K)]
        fused = os.path.join(tmp, "fused.txt")

        def separate():
            for k in range(K):
                test_on_dataset(models[k], data, single[k], heads[k], "ocsoftmax", task="19eval", ecapa=True,
                                keep_dataset_labels=True, sync="end")
            f = sf.avg_fuse(single, tmp + os.sep + "host_")
            return sf.fused_eer(f.key, f.score)

        def ensemble():
            return test_on_dataset_ensemble(models, data, ens, fused, "avg", loss_models=heads, add_loss="ocsoftmax",
                                            task="19eval", ecapa=True, keep_dataset_labels=True)[1].eer

        assert separate() == ensemble()
        for a, b in zip(single + [tmp + os.sep + "host_" + sf.OUTPUT_NAME], ens + [fused]):
            assert open(a, "rb").read() == open(b, "rb").read(), (a, b)
        rows.append(dict(what="ensemble", K=K, n=n, B=B, batches=len(data),
                         **timed(args.runs, separate_passes_then_avg_fuse=separate, ensemble_pass=ensemble)))
    print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="fuse,ensemble")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--trials", type=int, default=71237)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    rows = []
    for what in args.what.split(","):
        rows += {"fuse": bench_fuse, "ensemble": bench_ensemble}[what](args)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
