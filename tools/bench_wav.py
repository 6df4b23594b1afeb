#!/usr/bin/env python3
"""What converting a batch of WAV payloads on the device costs (profiles/wav_resample.md).  One process on one GPU.

B = 64 utterances of 4 s at the source rate, seeded noise plus a tone, for
    24 kHz s16 mono, 48 kHz s24 stereo, 44.1 kHz f32 mono and the 16 kHz s16 mono identity.

  decode    WavDecoder.decode over the packed batch already on the GPU, float32 out, Lcap = 64,000: ``--warmup`` calls,
            then ``--iters`` back-to-back calls between two device events; repeated ``--runs`` times: median (min .. max)
            per batch.  Once with the rate's coefficient table in LDS where it fits (option RESAMPLE_TABLE_LDS = 1, the
            default) and once with every table read through L2 (0).  The first call is checked: every status OK.
  host      scipy.signal.resample_poly(x, L, M) over the same batch as float32 mono on the host, one pass - another
            filter, there as context for what the host would spend, not as a reference.

The figure to hold this against is the 17.4 ms ResNet step at B = 64 (README).  These are records, not gates.

Usage: python tools/bench_wav.py [--batch 64] [--seconds 4] [--iters 50] [--runs 5] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEP_MS = 17.4  # README: the ResNet train step at B = 64, 4 s
CASES = [("24 kHz s16 mono", "s16", 1, 24000), ("48 kHz s24 stereo", "s24", 2, 48000), ("44.1 kHz f32 mono", "f32", 1, 44100),
         ("16 kHz s16 mono (identity)", "s16", 1, 16000)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import torch
    from scipy.signal import resample_poly
    import wav_cases as wc
    from asvspoof2021_air_amd import _hip, resample, wav

    dec = wav.WavDecoder("cuda")
    Lcap = int(a.seconds * 16000)
    out = {"batch": a.batch, "seconds": a.seconds, "step_ms": STEP_MS, "cases": []}
    for name, kind, C, sr in CASES:
        k, n = wc.KINDS[kind], int(a.seconds * sr)
        raws = [wc.quantise(wc.signal(n, 7 * b + 1, C, sr=sr), k) for b in range(a.batch)]
        items = [(torch.from_numpy(np.frombuffer(wc.encode(r, k), dtype=np.uint8).copy()),
                  wav.WavInfo(k, C, sr, 8 * wc.BYTES[k], C * wc.BYTES[k], n, 0)) for r in raws]
        by, off, fr, fm, rate, ln = wav.pack(items)
        by, off, fr, fm = by.cuda(), off.cuda(), fr.cuda(), fm.cuda()
        L, M, K = resample.geometry(sr)
        rec = {"case": name, "L": L, "M": M, "K": K, "payload_mb": int(off[-1]) / 1e6, "table_floats": L * K}
        for lds in (1, 0):
            with _hip.options(RESAMPLE_TABLE_LDS=lds):
                pcm, status = dec.decode(by, off, fr, fm, rate, Lcap=Lcap, check=True)
                ms = []
                for _ in range(a.runs):
                    for _ in range(a.warmup):
                        dec.decode(by, off, fr, fm, rate, Lcap=Lcap)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        dec.decode(by, off, fr, fm, rate, Lcap=Lcap)
                    e1.record()
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1) / a.iters)
            rec["decode_ms_table_%s" % ("lds" if lds else "l2")] = {"median": float(np.median(ms)), "min": min(ms), "max": max(ms)}
        mono = [wc.mono(wc.to_float(r, k)) for r in raws]
        t0 = time.perf_counter()
        for x in mono:
            if L != M:
                resample_poly(x, L, M)
        rec["host_resample_poly_ms"] = 1e3 * (time.perf_counter() - t0) if L != M else 0.0
        out["cases"].append(rec)
        print("%-28s L/M %3d/%-3d K %3d  decode %.3f ms (table in LDS) %.3f ms (through L2)  host resample_poly %.1f ms  step %.1f ms" % (
            name, L, M, K, rec["decode_ms_table_lds"]["median"], rec["decode_ms_table_l2"]["median"], rec["host_resample_poly_ms"], STEP_MS),
            flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
