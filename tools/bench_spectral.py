"""Times the STFT and Melspec front-ends (csrc/spectral.hip, profiles/spectral_frontends.md) in one process.

  python tools/bench_spectral.py [--rounds 7] [--reps 1000] [--json PATH]

B = 64 rows of 64 000 samples (4 s), fp32.  Per kind: the dense call, (B, T, D) with T = 401 (STFT) / 501 (Melspec), and
the padded call, those frames repeat-padded into (B, D, 750).  Beside them the LFCC padded call at the same shape
(csrc/lfcc.hip) and each launch's write floor: its output bytes over the 6.29 TB/s a float4 copy
reaches on an MI355X (MI355X_MICROARCH.md).  These are CALL times: device events around ``reps`` back-to-back module
calls (each allocates its output from the caching allocator and launches one kernel), windows of 20 - 30 ms; the
variants alternate round by round, the first two rounds only warm up; median and min .. max of the rest.  Kernel times:
run it under a kernel trace with fewer repetitions (profiles/spectral_frontends.md)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asvspoof2021_air_amd.feature_extraction import LFCC, STFT, Melspec  # noqa: E402

B, L, FEAT_LEN = 64, 64000, 750
HBM_COPY_TBS = 6.29  # measured float4 copy, MI355X_MICROARCH.md


def events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3  # us per call


def main(args):
    g = torch.Generator().manual_seed(1)
    x = (0.1 * torch.randn(B, L, generator=g)).cuda()
    stft = STFT(320, 160, 512, 16000).cuda()
    stft.mutate_input = False
    mel = Melspec().cuda()
    lfcc = LFCC(320, 160, 512, 16000, 20).cuda()
    lfcc.mutate_input = False
    variants = {
        "STFT dense (64, 401, 257)": (lambda: stft(x), B * 401 * 257 * 4),
        "STFT padded (64, 257, 750)": (lambda: stft.forward_padded(x, FEAT_LEN), B * 257 * FEAT_LEN * 4),
        "Melspec dense (64, 501, 128)": (lambda: mel.forward_frames(x), B * 501 * 128 * 4),
        "Melspec padded (64, 128, 750)": (lambda: mel.forward_padded(x, FEAT_LEN), B * 128 * FEAT_LEN * 4),
        "LFCC padded (64, 60, 750)": (lambda: lfcc.forward_padded(x, FEAT_LEN), B * 60 * FEAT_LEN * 4),
    }
    times = {k: [] for k in variants}
    for r in range(args.rounds + 2):
        for k, (fn, _) in variants.items():
            t = events(fn, args.reps)
            if r >= 2:
                times[k].append(t)
    out = {}
    for k, v in times.items():
        med, nbytes = statistics.median(v), variants[k][1]
        floor = nbytes / (HBM_COPY_TBS * 1e12) * 1e6
        print("%-32s %8.1f us  (min %.1f, max %.1f)   output %5.1f MB, write floor %5.1f us, %4.1f x the floor" % (
            k, med, min(v), max(v), nbytes / 1e6, floor, med / floor), flush=True)
        out[k] = {"median_us": med, "min_us": min(v), "max_us": max(v), "output_bytes": nbytes, "write_floor_us": floor}
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "B": B, "L": L, "feat_len": FEAT_LEN, "rounds": args.rounds,
                       "reps": args.reps, "results": out}, fh, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--json", default=None)
    main(ap.parse_args())
