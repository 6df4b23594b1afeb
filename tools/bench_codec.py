"""Times the G.711 codec augmentation (augment.g711_codec, profiles/codec_augment.md) in one process.

  python tools/bench_codec.py [--rounds 7] [--reps 20] [--no-step]

B = 128 rows of 64 000 samples (4 s), fp32 and int16, dense and ragged (lengths uniform in 1 - 4 s), with and without the
peak rescale.  Three yardsticks from the same run: ir_convolve (1024 taps) on the same batch, the HBM floor of the bytes
the stage has to move (rows read once, y written once; with the rescale y is read and written once more) at the measured
float4-copy rate of the part, and the ECAPA-TDNN-512 bf16 train step the stage precedes (B = 128, hipGraph replay).
Device events around back-to-back calls; the variants alternate round by round, the first two rounds only warm up."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asvspoof2021_air_amd.augment import g711_codec, ir_convolve, synthetic_ir_bank  # noqa: E402

B, L = 128, 64000
HBM_BYTES_PER_S = 6.29e12  # measured float4 copy (8.0e12 by the data sheet)


def events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3  # us per call


def floor_us(live, in_bytes, normalize):
    """Bytes the stage must move: the live samples in, every sample of y out, the live samples of y in and out again."""
    n = live * in_bytes + B * L * 4 + (2 * live * 4 if normalize else 0)
    return n / HBM_BYTES_PER_S * 1e6, n


def step_us(args):
    from asvspoof2021_air_amd.ecapa_tdnn import Bottle2neck, Res2Net2
    from asvspoof2021_air_amd.train import Trainer
    torch.manual_seed(688)
    model = Res2Net2(Bottle2neck, C=512, model_scale=8, nOut=2, n_mels=60)
    model.set_compute_dtype("bf16")
    tr = Trainer(model, enc_dim=256, lr=5e-4, r_real=0.9, r_fake=0.2, alpha=20.0, feat_len=400, ecapa=True)
    tr.enable_graph()
    g = torch.Generator().manual_seed(10)
    pcm = (0.1 * torch.randn(B, L, generator=g)).cuda()
    lab = (torch.arange(B) % 2).cuda()
    for _ in range(5):  # two eager steps, the capture, two replays
        loss = tr.step(pcm, lab)[0]
    assert tr._graph is not None and bool(torch.isfinite(loss))
    return [events(lambda: tr.step(pcm, lab), args.reps) for _ in range(args.rounds)]


def main(args):
    g = torch.Generator().manual_seed(1)
    x = (0.1 * torch.randn(B, L, generator=g)).cuda()
    x16 = (x * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
    ln = np.random.RandomState(0).randint(16000, L + 1, size=B).astype(np.int32)
    lengths = torch.from_numpy(ln).cuda()
    law = (torch.arange(B, device="cuda", dtype=torch.int32) % 2)
    irs = synthetic_ir_bank().cuda()
    idx = (torch.arange(B, device="cuda", dtype=torch.int32) % irs.shape[0])
    y = torch.empty(B, L, device="cuda")
    variants, floors = {}, {}
    for tname, t, nb in (("fp32", x, 4), ("int16", x16, 2)):
        for rname, ld, live in (("dense", None, B * L), ("ragged 1-4 s", lengths, int(ln.sum()))):
            for nz in (True, False):
                name = "g711 %-5s %-12s %s" % (tname, rname, "normalize" if nz else "raw")
                variants[name] = (lambda t=t, ld=ld, nz=nz: g711_codec(t, law, lengths=ld, normalize=nz, out=y))
                floors[name] = floor_us(live, nb, nz)
    variants["ir_convolve fp32 dense normalize (1024 taps)"] = lambda: ir_convolve(x, irs, idx, True, out=y)
    variants["ir_convolve int16 ragged normalize (1024 taps)"] = lambda: ir_convolve(x16, irs, idx, True, out=y, lengths=lengths)
    print("B = %d, L = %d, 63-tap low-pass; ragged: %d of %d samples live (%.1f %%)" % (
        B, L, int(ln.sum()), B * L, 100.0 * ln.sum() / (B * L)), flush=True)
    times = {k: [] for k in variants}
    for r in range(args.rounds + 2):
        for k, fn in variants.items():
            us = events(fn, args.reps)
            if r >= 2:
                times[k].append(us)
    for k, us in times.items():
        extra = ""
        if k in floors:
            extra = "  HBM floor %6.1f us (%.1f MB) -> %4.1f x floor" % (floors[k][0], floors[k][1] / 1e6,
                                                                        statistics.median(us) / floors[k][0])
        print("%-48s median %8.1f us  min %8.1f  max %8.1f%s" % (k, statistics.median(us), min(us), max(us), extra), flush=True)
    if not args.no_step:
        us = step_us(args)
        print("%-48s median %8.1f us  min %8.1f  max %8.1f" % ("ECAPA-TDNN-512 bf16 step, B = 128, graph replay", statistics.median(us),
                                                              min(us), max(us)), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    if not torch.cuda.is_available():
        sys.exit("bench_codec.py needs a GPU: there is nothing to measure without one")
    main(ap.parse_args())
