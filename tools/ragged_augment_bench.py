"""Times the IR channel augmentation on ragged batches (profiles/ragged_augment.md).

  python tools/ragged_augment_bench.py kernel [--parent-lib PATH]
      air_ir_convolve_ragged at B = 64, Lcap = 13 s, H = 1024 (int16 and fp32 rows; corpus-like lengths of 1 - 13 s, and all
      rows full) beside the dense air_ir_convolve at (64, 13 * 16000); --parent-lib: the dense call of another build of the
      library (the parent commit's) in the same process, the variants alternating round by round.
  python tools/ragged_augment_bench.py step
      ECAPA-TDNN-512 bf16, B = 128, ragged int16 batches on hipGraph replay: the step with ChannelAugment beside the same
      step without it, alternating window by window.
Median and minimum over the rounds; device events around back-to-back calls, clocks warmed by the rounds before."""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asvspoof2021_air_amd import _hip  # noqa: E402
from asvspoof2021_air_amd.augment import ChannelAugment, ir_convolve, synthetic_ir_bank  # noqa: E402

SR, CAP_S = 16000, 13


def corpus_lengths(B, seed=0):
    """Uniform in 1 .. 13 s, like tools/ragged_lfcc_profile.py."""
    return np.random.RandomState(seed).randint(1 * SR, CAP_S * SR + 1, size=B).astype(np.int32)


def events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3  # us per call


def report(name, us, extra=""):
    print("%-34s median %8.1f us  min %8.1f us  max %8.1f us  (%d rounds)%s" % (
        name, statistics.median(us), min(us), max(us), len(us), extra), flush=True)


def kernel(args):
    B, L = 64, CAP_S * SR
    g = torch.Generator().manual_seed(1)
    x = (0.1 * torch.randn(B, L, generator=g)).cuda()
    x16 = (x * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
    irs = synthetic_ir_bank().cuda()
    n_ir, H = irs.shape
    idx = (torch.arange(B, device="cuda", dtype=torch.int32) % n_ir)
    ln = corpus_lengths(B)
    full = torch.full((B,), L, dtype=torch.int32, device="cuda")
    corpus = torch.from_numpy(ln).cuda()
    y = torch.empty(B, L, device="cuda")
    variants = {
        "dense (this build)": lambda: ir_convolve(x, irs, idx, True, out=y),
        "ragged fp32, all rows full": lambda: ir_convolve(x, irs, idx, True, out=y, lengths=full),
        "ragged int16, all rows full": lambda: ir_convolve(x16, irs, idx, True, out=y, lengths=full),
        "ragged fp32, 1 - 13 s": lambda: ir_convolve(x, irs, idx, True, out=y, lengths=corpus),
        "ragged int16, 1 - 13 s": lambda: ir_convolve(x16, irs, idx, True, out=y, lengths=corpus),
    }
    if args.parent_lib:
        old = ctypes.CDLL(args.parent_lib)
        old.air_ir_convolve_ws_bytes_ex.restype = ctypes.c_size_t
        n = old.air_ir_convolve_ws_bytes_ex(_hip.ci(B), _hip.ci(n_ir), _hip.ci(H))
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        y_old = torch.empty(B, L, device="cuda")

        def dense_old():
            _hip.check(old.air_ir_convolve(_hip.dptr(x), _hip.ci(B), _hip.ci(L), _hip.dptr(irs), _hip.ci(n_ir), _hip.ci(H),
                                           _hip.dptr(idx, torch.int32), _hip.ci(1), _hip.dptr(y_old), _hip.dptr(ws, torch.uint8),
                                           _hip.csz(n), _hip.stream()), "air_ir_convolve (parent)")
        variants["dense (parent build)"] = dense_old
        dense_old()
        variants["dense (this build)"]()
        torch.cuda.synchronize()
        print("dense, parent build against this build: bit-identical = %s" % torch.equal(y, y_old))
    print("B = %d, Lcap = %d, H = %d, IR_FFT = %d; corpus-like lengths: mean %.2f s, %d of %d samples live (%.1f %%)" % (
        B, L, H, _hip.get_option("IR_FFT"), ln.mean() / SR, int(ln.sum()), B * L, 100.0 * ln.sum() / (B * L)))
    times = {k: [] for k in variants}
    for r in range(args.rounds + 2):
        for k, fn in variants.items():
            us = events(fn, args.reps)
            if r >= 2:  # the first two rounds warm code objects, workspaces and clocks
                times[k].append(us)
    for k, us in times.items():
        report(k, us)


def step(args):
    from asvspoof2021_air_amd.ecapa_tdnn import Bottle2neck, Res2Net2
    from asvspoof2021_air_amd.train import Trainer
    B, L = 128, CAP_S * SR
    trainers = {}
    for name in ("ragged", "ragged + augment"):
        torch.manual_seed(688)
        model = Res2Net2(Bottle2neck, C=512, model_scale=8, nOut=2, n_mels=60)
        model.set_compute_dtype("bf16")
        tr = Trainer(model, enc_dim=256, lr=5e-4, r_real=0.9, r_fake=0.2, alpha=20.0, feat_len=750, ecapa=True)
        tr.enable_graph()
        if name != "ragged":
            tr.augment = ChannelAugment(p=1.0, seed=688)
        trainers[name] = tr
    batches = []
    for i in range(3):
        g = torch.Generator().manual_seed(10 + i)
        pcm = (0.1 * torch.randn(B, L, generator=g) * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
        ln = corpus_lengths(B, seed=i)
        for b, n in enumerate(ln):
            pcm[b, n:] = 0
        T = 1 + ln // 160
        st = np.array([np.random.RandomState(i).randint(t - 750) if t > 750 else 0 for t in T], dtype=np.int32)
        batches.append((pcm.cuda(), (torch.arange(B) % 2).cuda(), torch.from_numpy(st).cuda(), torch.from_numpy(ln).cuda()))
    n = [0]

    def one(tr):
        pcm, lab, st, ln = batches[n[0] % 3]
        n[0] += 1
        return tr.step(pcm, lab, start=st, lengths=ln)

    for tr in trainers.values():  # two eager steps, the capture, two replays
        for _ in range(5):
            loss = one(tr)[0]
        assert tr._graph is not None and "ragged" in tr._graph["key"] and bool(torch.isfinite(loss))
    torch.cuda.synchronize()
    times = {k: [] for k in trainers}
    for r in range(args.rounds + 1):
        for k, tr in trainers.items():
            us = events(lambda: one(tr), args.reps)
            if r >= 1:
                times[k].append(us)
    print("ECAPA-TDNN-512 bf16, B = %d, int16 rows of %d s, lengths 1 - 13 s, feat_len 750, hipGraph replay; %d steps per window" % (
        B, CAP_S, args.reps))
    for k, us in times.items():
        report(k, us, "  -> %.0f utterances/s" % (B / (statistics.median(us) * 1e-6)))
    for tr in trainers.values():
        assert len(tr._graph["graphs"]) == 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernel", "step"])
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    (kernel if a.what == "kernel" else step)(a)
