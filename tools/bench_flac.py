#!/usr/bin/env python3
"""What decoding a batch of FLAC files on the device costs (profiles/flac_decode.md).  One process on one GPU.

B = 64 utterances of 4 s (64,000 samples at 16 kHz) of the synthetic corpus (synth.py), quantised to int16 and written by
the oracle encoder (tests/flac_oracle.py) the way an encoder at its default level writes speech: block size 4096, LPC
order 8 with 12-bit coefficients fitted per frame (autocorrelation method, Hann window), partition order 3 with the
cheapest Rice parameter per partition.  ``--streams FILE.npz`` keeps the encoded streams (the encoder is pure Python:
~20 s for 64 utterances) and reads them back on the next run.

  decode    FlacDecoder.decode over the packed batch already on the GPU, int16 out: ``--warmup`` calls, then ``--iters``
            back-to-back calls between two device events; repeated ``--runs`` times: median (min .. max) per batch.
            The first run also checks every row against the samples that were encoded, and the status.
  split     (``--split``) the same calls in a child process under ``rocprofv3 --kernel-trace``: per kernel of the chain
            (tail, scan, compact, prefix, parse, chain, decode) the mean duration per batch.
  bytes     compressed bytes over PCM bytes of the batch.

The figure to hold this against is the 17.4 ms ResNet step at B = 64 (README): a decoder slower than the step it feeds
would make the loader set the rate.

Usage: python tools/bench_flac.py [--batch 64] [--seconds 4] [--iters 50] [--runs 5] [--split] [--streams f.npz] [--json out.json]
"""
import argparse
import glob
import json
import os
import re
import sqlite3
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEP_MS = 17.4  # README: the ResNet train step at B = 64, 4 s


def lpc_frame_spec(x, order=8, precision=12):
    """LPC coefficients of one frame by the autocorrelation method, quantised as an encoder does."""
    w = x.astype(np.float64) * np.hanning(len(x))
    r = np.array([np.dot(w[:len(w) - k], w[k:]) for k in range(order + 1)])
    if r[0] <= 0:
        return dict(type="fixed", order=0, partition_order=3)
    a, e = np.zeros(order), r[0]
    for i in range(order):  # Levinson-Durbin
        k = (r[i + 1] - np.dot(a[:i], r[i:0:-1])) / e
        a[:i + 1] = np.concatenate((a[:i] - k * a[:i][::-1], [k]))
        e *= 1 - k * k
    shift = min(precision - 1 - int(np.floor(np.log2(max(np.abs(a).max(), 1e-9)))) - 1, 15)
    shift = max(shift, 0)
    q = np.clip(np.round(a * (1 << shift)), -(1 << (precision - 1)), (1 << (precision - 1)) - 1).astype(int)
    return dict(type="lpc", coefs=[int(c) for c in q], precision=precision, shift=shift, partition_order=3, params=None)


def make_streams(batch, samples, path=None):
    import flac_oracle as fo
    from asvspoof2021_air_amd import synth
    if path and os.path.exists(path):
        z = np.load(path)
        if int(z["batch"]) == batch and int(z["samples"]) == samples:
            return [bytes(z["s%d" % i]) for i in range(batch)], [z["x%d" % i] for i in range(batch)]
    streams, waves = [], []
    for i in range(batch):
        x = np.clip(np.round(synth.utterance(2021, i, samples)[0] * 32768.0), -32768, 32767).astype(np.int16)
        specs = [lpc_frame_spec(x[at:at + 4096]) for at in range(0, samples, 4096)]
        streams.append(fo.encode(x, 4096, specs))
        waves.append(x)
    if path:
        np.savez(path, batch=batch, samples=samples, **{"s%d" % i: np.frombuffer(s, dtype=np.uint8) for i, s in enumerate(streams)},
                 **{"x%d" % i: x for i, x in enumerate(waves)})
    return streams, waves


def kernel_means(db_path, batches):
    db = sqlite3.connect(db_path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    agg = {}
    for name, s, e in db.execute("select %s, start, end from kernels" % name_col):
        m = re.search(r"flac_(\w+?)_kernel", name)
        if m:
            a = agg.setdefault(m.group(1), [0, 0])
            a[0] += 1
            a[1] += e - s
    return {k: {"launches_per_batch": n / batches, "us_per_batch": ns / 1e3 / batches} for k, (n, ns) in agg.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--streams", default=None)
    ap.add_argument("--encode-only", action="store_true", help="write --streams and stop (needs no GPU)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    samples = int(round(args.seconds * 16000))
    streams, waves = make_streams(args.batch, samples, args.streams)
    comp = sum(len(s) for s in streams)
    ratio = comp / (2.0 * samples * args.batch)
    print("batch %d x %d samples: %d compressed bytes, %.3f of the PCM bytes" % (args.batch, samples, comp, ratio))
    if args.encode_only:
        return

    import torch
    from asvspoof2021_air_amd import flac
    if not torch.cuda.is_available():
        raise SystemExit("bench_flac.py measures on the GPU: none found")
    items = []
    for s in streams:
        info = flac.parse_stream(s)
        items.append((torch.from_numpy(np.frombuffer(s, dtype=np.uint8, offset=info.audio_offset).copy()), info))
    by, off, ln, bs = flac.pack(items)
    by, off, ln, bs = by.cuda(), off.cuda(), ln.cuda(), bs.cuda()
    dec = flac.FlacDecoder("cuda")
    cap = -(-samples // 16000) * 16000

    def call():
        return dec.decode(by, off, ln, bs, Lcap=cap)

    pcm, status = call()
    dec.check(status)
    want = torch.from_numpy(np.stack(waves))
    assert torch.equal(pcm[:, :samples].cpu(), want) and int(torch.count_nonzero(pcm[:, samples:])) == 0
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    if args.child:  # under the profiler: the calls alone
        for _ in range(args.iters):
            call()
        torch.cuda.synchronize()
        return
    per_batch = []
    for _ in range(args.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            call()
        e1.record()
        e1.synchronize()
        per_batch.append(e0.elapsed_time(e1) / args.iters)
    out = {"batch": args.batch, "samples": samples, "compressed_bytes": comp, "compressed_over_pcm": ratio,
           "decode_ms_per_batch": {"median": float(np.median(per_batch)), "min": min(per_batch), "max": max(per_batch)},
           "iters": args.iters, "runs": args.runs, "resnet_step_ms": STEP_MS,
           "audio_seconds_per_second": args.batch * args.seconds / (float(np.median(per_batch)) * 1e-3)}
    print("decode: %.3f ms per batch (%.3f .. %.3f), %d iterations x %d runs; the ResNet step it feeds: %.1f ms" % (
        out["decode_ms_per_batch"]["median"], min(per_batch), max(per_batch), args.iters, args.runs, STEP_MS))
    if args.split:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "-d", tmp, "-o", "k", "--", sys.executable, os.path.abspath(__file__), "--child",
                   "--batch", str(args.batch), "--seconds", str(args.seconds), "--iters", str(args.iters), "--warmup", str(args.warmup)]
            if args.streams:
                cmd += ["--streams", args.streams]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            dbs = glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True)
            if r.returncode != 0 or not dbs:
                raise SystemExit("the profiled child failed (rc %d):\n%s" % (r.returncode, r.stderr[-2000:]))
            out["kernels"] = kernel_means(dbs[0], args.iters + args.warmup + 1)
        total = sum(v["us_per_batch"] for v in out["kernels"].values())
        for k, v in sorted(out["kernels"].items(), key=lambda kv: -kv[1]["us_per_batch"]):
            print("  flac_%-8s %9.1f us per batch  %5.1f %%" % (k, v["us_per_batch"], 100.0 * v["us_per_batch"] / total))
        print("  kernels together %.1f us per batch" % total)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
