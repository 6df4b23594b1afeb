#!/usr/bin/env python3
"""Times the SE-Res2Net-50 train step (model.py:256-509 + OC-Softmax + Adam, main_train.py:310-409 with -m res2net)
at B = 64, 4 s utterances, feat_len 750: eager and hipGraph-replayed (train.Trainer.enable_graph).  Device-synchronised
windows of --steps steps; prints the median and spread per mode.  --shapes: the narrow-channel convolutions of one
step, grouped by kernel (conv_narrow.hip template instance), with the FLOPs and algorithmic HBM bytes their shapes need
per step (every operand read once, every result written once; computed, not measured) - the numerators of the
achieved rates in profiles/res2net_b64_kernel_stats.md.
Usage: python tools/kbench_res2net.py [--batch 64] [--steps 10] [--windows 5] [--shapes]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np


def narrow_convs(B, H=60, W=750):
    """(Cin, Cout, k, stride, H, W, prologue, count) of every narrow-kernel convolution of the model at (B, 1, H, W)."""
    import res2net_oracle as o
    from asvspoof2021_air_amd.res2net import _generic_1x1
    out = {}

    def add(*s):
        out[s] = out.get(s, 0) + 1
    add(1, 16, 3, 1, H, W, False)
    add(16, 16, 3, 1, H, W, True)
    add(16, 16, 3, 1, H, W, True)
    h, w_ = H, W
    for _, cin, planes, stride, width, stage, ds in o.blocks():
        if not _generic_1x1(cin, 4 * width):
            add(cin, 4 * width, 1, 1, h, w_, False)
        for _ in range(3):
            add(width, width, 3, stride, h, w_, False)
        ho, wo = (h - 1) // stride + 1, (w_ - 1) // stride + 1
        if not _generic_1x1(4 * width, 2 * planes):
            add(4 * width, 2 * planes, 1, 1, ho, wo, False)
        if ds is not None and not _generic_1x1(cin, 2 * planes):
            add(cin, 2 * planes, 1, 1, -(-h // ds), -(-w_ // ds), False)
        h, w_ = ho, wo
    return [k + (v,) for k, v in out.items()]


def _tile(c):
    return 8 if c <= 8 else (16 if c <= 16 else 32)


def kernel_table(B):
    """{kernel instance: [launches, FLOPs, bytes]} per train step of the narrow kernels."""
    t = {}
    for ci, co, k, s, H, W, pro, n in narrow_convs(B):
        Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
        fl = 2.0 * B * ci * co * k * k * Ho * Wo
        xb, yb, wb = 4.0 * B * ci * H * W, 4.0 * B * co * Ho * Wo, 4.0 * ci * co * k * k
        rows = [("narrow_fwd_kernel<%d, %d, %d>" % (_tile(co), k, s), fl, xb + yb + wb),
                ("narrow_wgrad_partial_kernel<%d, %d>" % (k, s), fl, xb + yb)]
        if ci > 1:
            rows.append(("narrow_dgrad_kernel<%d, %d, %d>" % (_tile(ci), k, s), fl, xb + yb + wb))
        for name, f, b in rows:
            e = t.setdefault(name, [0, 0.0, 0.0])
            e[0] += n
            e[1] += f * n
            e[2] += b * n
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--shapes", action="store_true")
    a = ap.parse_args()
    B = a.batch
    if a.shapes:
        tot_f = tot_b = 0.0
        print("%-40s %9s %10s %9s %12s %12s" % ("kernel", "launches", "GFLOP", "GB", "t_flop us", "t_byte us"))
        for name, (n, f, b) in sorted(kernel_table(B).items()):
            tot_f += f
            tot_b += b
            # lower bounds at 157.3 TFLOP/s (f32) and 6.29 TB/s (measured HBM copy), MI355X_MICROARCH.md
            print("%-40s %9d %10.2f %9.3f %12.1f %12.1f" % (name, n, f / 1e9, b / 1e9, f / 157.3e12 * 1e6,
                                                            b / 6.29e12 * 1e6))
        print("narrow convolutions per step: %.1f GFLOP, %.2f GB" % (tot_f / 1e9, tot_b / 1e9))
        return
    import torch
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.res2net import Res2Net, SEBottle2neck
    from asvspoof2021_air_amd.train import Trainer
    from oracle.filler import fill_module_, synth_pcm
    pcm = synth_pcm(B, 64000, seed=1).cuda()
    labels = (torch.arange(B) % 2).cuda()
    for mode in ("eager", "graph"):
        m = fill_module_(Res2Net(SEBottle2neck, [3, 4, 6, 3], baseWidth=26, scale=4, pretrained=False, num_classes=2))
        tr = Trainer(m, loss_module=fill_module_(AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)), feat_len=750)
        if mode == "graph":
            tr.enable_graph(True)
        for _ in range(3):
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
        print("%-5s step %.2f ms (min %.2f, max %.2f over %d windows of %d)  %.0f utt/s  loss %.4f" % (
            mode, med * 1e3, per.min() * 1e3, per.max() * 1e3, a.windows, a.steps, B / med, loss.item()), flush=True)
        del tr, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
