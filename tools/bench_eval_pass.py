#!/usr/bin/env python3
"""What the sync-free dev / eval pass buys (profiles/eval_pass.md).  Three comparisons, each the median of
``--runs`` timed runs with their spread (min .. max), the two sides alternating run by run, in one process on one GPU:

  pass     Trainer.evaluate over ``--batches`` batches against the per-batch loop it replaces (eval_batch + .item() per
           batch, np.nanmean, host eer_both_polarities - main_train.py:526-575, :662-671), ResNet-18 B = 64 and
           ECAPA-TDNN (bf16) B = 128 on 4 s of PCM
  score    generate_score.test_on_dataset at batch size 1 under use_graph=True, sync="end" against sync="batch"
  metric   eer_both_polarities_device (upload of host scores included / scores already on the device) against host
           eer_both_polarities at the sizes of the 2019 LA dev / eval and the 2021 LA / DF evaluation sets (the DF
           set, 611,829 trials, is inside the device limit of 2^20)

Usage: python tools/bench_eval_pass.py [--what pass,score,metric] [--runs 5] [--batches 128] [--utts 2000] [--json out.json]
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

from asvspoof2021_air_amd import eval_metrics as em  # noqa: E402
from asvspoof2021_air_amd.train import Trainer  # noqa: E402


def timed(runs, **variants):
    """{name: median / min / max seconds of ``runs`` runs}; the variants alternate run by run behind one warm-up each
    (workspaces, lazy module loads, graph captures), every run ends in a device synchronise."""
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
    return {k: {"median_s": float(np.median(v)), "min_s": min(v), "max_s": max(v), "runs": v} for k, v in out.items()}


def make_trainer(kind):
    torch.manual_seed(688)
    if kind == "resnet":
        from asvspoof2021_air_amd.resnet import ResNet
        m = ResNet(3, 256, resnet_type="18", nclasses=2)
        m.set_attention_noise(None)  # (fresh noise per call otherwise: the two sides could not be compared for equality)
        return Trainer(m), 64
    from asvspoof2021_air_amd.ecapa_tdnn import Bottle2neck, Res2Net2
    m = Res2Net2(Bottle2neck, C=512, model_scale=8, nOut=2, n_mels=60).cuda().set_compute_dtype("bf16")
    return Trainer(m, ecapa=True), 128


def per_batch_loop(tr, batches):
    losses, scores, labels = [], [], []
    for pcm, lab in batches:
        loss, score = tr.eval_batch(pcm, lab)
        losses.append(loss.item())
        scores.append(score.cpu().numpy())
        labels.append(lab.cpu().numpy())
    return np.nanmean(losses), em.eer_both_polarities(np.concatenate(scores), np.concatenate(labels))


def bench_pass(args):
    rows = []
    for kind in ("resnet", "ecapa"):
        tr, B = make_trainer(kind)
        g = torch.Generator().manual_seed(1)
        pool = [(0.1 * torch.randn(B, 64000, generator=g)).cuda() for _ in range(4)]  # 4 s of PCM; the pass cycles 4 batches
        labs = [((torch.arange(B) + i) % 3 != 0).long().cuda() for i in range(4)]
        batches = [(pool[i % 4], labs[i % 4]) for i in range(args.batches)]
        want = per_batch_loop(tr, batches)
        got = tr.evaluate(batches)
        assert (got.loss, got.eer) == want, (got.loss, got.eer, want)
        rows.append(dict(what="pass", model=kind, B=B, batches=args.batches,
                         **timed(args.runs, loop=lambda: per_batch_loop(tr, batches), evaluate=lambda: tr.evaluate(batches))))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def bench_score(args):
    from asvspoof2021_air_amd.generate_score import test_on_dataset
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.resnet import ResNet
    torch.manual_seed(688)
    model = ResNet(3, 256, resnet_type="18", nclasses=2).cuda()
    model.set_attention_noise(None)
    lossm = AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0).cuda()
    g = torch.Generator().manual_seed(2)
    feats = [torch.randn(1, 1, 750, 60, generator=g).cuda() for _ in range(8)]
    data = [(feats[i % 8], ["LA_E_%07d" % i]) for i in range(args.utts)]
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        fa, fb = os.path.join(tmp, "a.txt"), os.path.join(tmp, "b.txt")
        run = lambda path, sync: test_on_dataset(model, data, path, lossm, "ocsoftmax", task="LA", use_graph=True, sync=sync)
        run(fa, "batch")
        run(fb, "end")
        assert open(fa, "rb").read() == open(fb, "rb").read()
        rows.append(dict(what="score", utts=args.utts,
                         **timed(args.runs, batch=lambda: run(fa, "batch"), end=lambda: run(fb, "end"))))
    print(json.dumps(rows[-1]), flush=True)
    return rows


def bench_metric(args):
    rows = []
    for n in (24844, 71237, 181566, 611829):
        rng = np.random.default_rng(n)
        lab = (rng.random(n) < 0.9).astype(np.int64)
        s = (rng.normal(0, 1, n) + np.where(lab == 0, 1.0, -1.0)).astype(np.float32)
        ds, dl = torch.from_numpy(s).cuda(), torch.from_numpy(lab).cuda()
        s64 = s.astype(np.float64)
        assert em.eer_both_polarities_device(ds, dl).result() == em.eer_both_polarities(s64, lab)
        rows.append(dict(what="metric", n=n, **timed(
            args.runs, host=lambda: em.eer_both_polarities(s64, lab),
            device_resident=lambda: em.eer_both_polarities_device(ds, dl).result(),
            device_with_upload=lambda: em.eer_both_polarities_device(torch.from_numpy(s).cuda(),
                                                                     torch.from_numpy(lab).cuda()).result())))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="pass,score,metric")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batches", type=int, default=128)
    ap.add_argument("--utts", type=int, default=2000)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    rows = []
    for what in args.what.split(","):
        rows += {"pass": bench_pass, "score": bench_score, "metric": bench_metric}[what](args)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
