#!/usr/bin/env python3
"""Times the LCNN train step (model.py:511-610 + OC-Softmax + Adam, main_train.py:310-409 with -m lcnn) at B = 64,
4 s utterances, feat_len 750: eager and hipGraph-replayed (train.Trainer.enable_graph).  Device-synchronised windows
of --steps steps; prints the median and spread per mode, and the step's FLOPs and algorithmic HBM bytes computed from
the layer shapes (not measured).  --pad-cost: times conv3's and conv4's forward + data + weight gradient on 128 and on
64 weight rows and reports what the 32 zero rows beyond 96 cost per step, assuming the time is linear in the rows.
Usage: python tools/kbench_lcnn.py [--batch 64] [--steps 10] [--windows 5] [--pad-cost]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

# (Cin, Cout, k, H, W of the conv output, pool after MFM, BatchNorm) of conv1 .. conv9 at feat_len 750
SHAPES = ((1, 64, 5, 60, 750, True, False), (32, 64, 1, 30, 375, False, True), (32, 96, 3, 30, 375, True, True),
          (48, 96, 1, 15, 187, False, True), (48, 128, 3, 15, 187, True, False), (64, 128, 1, 7, 93, False, True),
          (64, 64, 3, 7, 93, False, True), (32, 64, 1, 7, 93, False, True), (32, 64, 3, 7, 93, True, False))


def cost(B):
    """(forward FLOPs, train-step FLOPs, algorithmic bytes per step) from the shapes: every conv's 2 MACs x 3 passes
    (forward, data and weight gradient; conv1 has no data gradient), each tensor read / written once per pass."""
    f_fwd = f_step = 0.0
    byt = 0.0
    for i, (ci, co, k, H, W, pool, bn) in enumerate(SHAPES):
        fl = 2.0 * B * co * ci * k * k * H * W
        f_fwd += fl
        f_step += fl * (2 if i == 0 else 3)
        xin = B * ci * H * W * 4
        post = B * co // 2 * (H // 2 if pool else H) * (W // 2 if pool else W) * 4
        pre = 0 if i == 0 else B * co * H * W * 4  # conv1's pre-MFM map is never written
        # forward: read input, write pre, read pre, write post (+ BN: read post twice, write once)
        byt += xin + 2 * pre + post + (3 * post if bn else 0)
        # backward: BN backward (read post, dpost; write dpost), route backward (read dpost, write dpre),
        # dgrad (read dpre, write dx), wgrad (read input, dpre)
        byt += (3 * post if bn else 0) + post + pre + (pre + xin if i else 0) + xin + pre
    head = 2.0 * B * (4416 * 160 + 80 * 256 + 256 * 2)
    return f_fwd + head, f_step + 3 * head, byt


def pad_cost(B, reps=20):
    """ms per step of conv3 + conv4 (fwd, dgrad, wgrad) with 128 and with 64 weight rows; the 96-row layers run on
    128 zero-padded rows, so (t128 - t64) / 2 estimates the 32 padded rows' cost."""
    from asvspoof2021_air_amd import ops
    res = {}
    for rows in (128, 64):
        layers = []
        for cin, k, pad, H, W in ((32, 3, 1, 30, 375), (48, 1, 0, 15, 187)):
            x = torch.randn(B, cin, H, W, device="cuda")
            w = torch.randn(rows, cin, k, k, device="cuda") * 0.05
            dy = torch.randn(B, rows, H, W, device="cuda")
            layers.append((x, w, dy, pad))

        def one():
            for x, w, dy, pad in layers:
                ops.conv2d_fwd(x, w, 1, pad)
                ops.conv2d_dgrad(dy, w, x.shape, 1, pad)
                ops.conv2d_wgrad(x, dy, w.shape, 1, pad)
        for _ in range(3):
            one()
        torch.cuda.synchronize()
        per = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(reps):
                one()
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) / reps)
        res[rows] = float(np.median(per))
    print("conv3 + conv4 fwd+dgrad+wgrad: %.3f ms on 128 rows, %.3f ms on 64 rows -> the 32 padded rows cost ~%.3f ms "
          "per step (linear estimate)" % (res[128] * 1e3, res[64] * 1e3, (res[128] - res[64]) / 2 * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--pad-cost", action="store_true")
    a = ap.parse_args()
    if a.pad_cost:
        pad_cost(a.batch)
        return
    from asvspoof2021_air_amd.lcnn import LCNN
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.train import Trainer
    from oracle.filler import fill_module_, synth_pcm
    B = a.batch
    f_fwd, f_step, byt = cost(B)
    print("B=%d: forward %.1f GFLOP, train step %.1f GFLOP, algorithmic %.2f GB per step (from shapes)" % (
        B, f_fwd / 1e9, f_step / 1e9, byt / 1e9))
    pcm = synth_pcm(B, 64000, seed=1).cuda()
    labels = (torch.arange(B) % 2).cuda()
    out = {}
    for mode in ("eager", "graph"):
        m = fill_module_(LCNN(60, 256))
        tr = Trainer(m, loss_module=fill_module_(AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)), feat_len=750)
        if mode == "graph":
            tr.enable_graph(True)
        for _ in range(4):
            tr.step(pcm, labels)
        torch.cuda.synchronize()
        per = []
        for _ in range(a.windows):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss, _ = tr.step(pcm, labels)
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) / a.steps)
        per = np.array(per)
        med = float(np.median(per))
        out[mode] = med
        print("%-5s step %.3f ms (min %.3f, max %.3f over %d windows of %d)  %.0f utt/s  %.1f TFLOP/s  %.2f TB/s alg  loss %.4f" % (
            mode, med * 1e3, per.min() * 1e3, per.max() * 1e3, a.windows, a.steps, B / med, f_step / med / 1e12,
            byt / med / 1e12, loss.item()))
        del tr, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
