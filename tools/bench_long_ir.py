"""Times the bank form of the impulse-response augmentation (air_ir_bank_convolve, profiles/long_ir.md) in one process.

  python tools/bench_long_ir.py [--rounds 7] [--reps 10] [--no-step] [--no-direct]

B = 128 rows of 64 000 samples (4 s), fp32, all rows full, peak rescale on.  Per Hmax in {2048, 4096, 16384}: the only route
the dense call has for such a response - air_ir_convolve_ragged on a (n_ir, Hmax) table, the direct FIR - beside the bank
call with every row on a response of Hmax taps.  Then the reference's mix (27 responses of 1024 taps + 3 of 16 000, indices
cycling through the bank: 10 % of the rows long) beside the same call with every row on a 16 000-tap response and beside the
dense 1024-tap bank through the existing call.  Last, the ECAPA-TDNN-512 bf16 train step (B = 128, hipGraph replay) with
either bank as its augmentation.  Device events around back-to-back calls; the variants alternate round by round, the
first two rounds only warm up; median and min .. max of the remaining windows."""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asvspoof2021_air_amd import _hip  # noqa: E402
from asvspoof2021_air_amd.augment import ChannelAugment, IRBank, ir_convolve, synthetic_ir_bank  # noqa: E402

B, L = 128, 64000
PART = 2048  # the long form's partition


def events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3  # us per call


def response(taps, rng):
    h = rng.standard_normal(taps) * np.exp(-6.907755 * np.arange(taps) / taps)
    return (h / np.sqrt((h ** 2).sum())).astype(np.float32)


def partitions(bank, idx):
    """Partitions the long form runs for these rows (rows of at most 1025 taps run the short form: none)."""
    t = bank.taps.cpu().numpy()[idx.cpu().numpy()]
    return int(np.where(t > 1025, -(-t // PART), 0).sum())


def step_us(args, irs):
    from asvspoof2021_air_amd.ecapa_tdnn import Bottle2neck, Res2Net2
    from asvspoof2021_air_amd.train import Trainer
    torch.manual_seed(688)
    model = Res2Net2(Bottle2neck, C=512, model_scale=8, nOut=2, n_mels=60)
    model.set_compute_dtype("bf16")
    tr = Trainer(model, enc_dim=256, lr=5e-4, r_real=0.9, r_fake=0.2, alpha=20.0, feat_len=400, ecapa=True,
                 augment=ChannelAugment(irs=irs, p=1.0, seed=1))
    tr.enable_graph()
    g = torch.Generator().manual_seed(10)
    pcm = (0.1 * torch.randn(B, L, generator=g)).cuda()
    lab = (torch.arange(B) % 2).cuda()
    for _ in range(5):  # two eager steps, the capture, two replays
        loss = tr.step(pcm, lab)[0]
    assert tr._graph is not None and bool(torch.isfinite(loss))
    return [events(lambda: tr.step(pcm, lab), args.reps) for _ in range(args.rounds)]


def report(name, v):
    med = statistics.median(v)
    print("%-58s %9.1f us  (min %.1f, max %.1f, spread %.1f %%)" % (name, med, min(v), max(v), 100.0 * (max(v) - min(v)) / med),
          flush=True)
    return med


def main(args):
    rng = np.random.default_rng(1)
    g = torch.Generator().manual_seed(1)
    x = (0.1 * torch.randn(B, L, generator=g)).cuda()
    full = torch.full((B,), L, dtype=torch.int32).cuda()
    y = torch.empty(B, L, device="cuda")
    variants = {}
    for H in (2048, 4096, 16384):
        bank = IRBank([response(H, rng) for _ in range(3)]).to("cuda")
        idx = (torch.arange(B, device="cuda", dtype=torch.int32) % 3)
        if not args.no_direct:
            variants["direct FIR (dense table), all rows %5d taps" % H] = (
                lambda bank=bank, idx=idx: ir_convolve(x, bank.irs, idx, True, out=y, lengths=full))
        variants["bank, all rows %5d taps (%d partitions)" % (H, partitions(bank, idx))] = (
            lambda bank=bank, idx=idx: ir_convolve(x, bank, idx, True, out=y, lengths=full))
    dense = synthetic_ir_bank().cuda()
    mix = IRBank(list(dense[:27]) + [response(16000, rng) for _ in range(3)]).to("cuda")
    idx30 = (torch.arange(B, device="cuda", dtype=torch.int32) % 30)
    idx_long = 27 + (torch.arange(B, device="cuda", dtype=torch.int32) % 3)
    n_mix, n_long = partitions(mix, idx30), partitions(mix, idx_long)
    k_mix = "bank 27 x 1024 + 3 x 16000, indices cycling (%d partitions)" % n_mix
    k_long = "bank 27 x 1024 + 3 x 16000, all rows long (%d partitions)" % n_long
    k_old = "existing call, dense 30 x 1024 bank"
    variants[k_mix] = lambda: ir_convolve(x, mix, idx30, True, out=y, lengths=full)
    variants[k_long] = lambda: ir_convolve(x, mix, idx_long, True, out=y, lengths=full)
    variants[k_old] = lambda: ir_convolve(x, dense, idx30, True, out=y, lengths=full)
    lib = _hip.lib()
    for name, bank in (("all rows 16384 taps", (3, 16384)), ("the mix", tuple(mix.irs.shape))):
        n = lib.air_ir_bank_ws_bytes(ctypes.c_int(B), ctypes.c_int(L), ctypes.c_int(bank[0]), ctypes.c_int(bank[1]))
        print("workspace, B = %d, L = %d, %s: %.1f MiB" % (B, L, name, n / 2.0 ** 20), flush=True)
    times = {k: [] for k in variants}
    for r in range(args.rounds + 2):
        for k, fn in variants.items():
            slow = k.startswith("direct")
            t = events(fn, max(1, args.reps // 5) if slow else args.reps)
            if r >= 2:
                times[k].append(t)
    med = {k: report(k, v) for k, v in times.items()}
    print("mix / all-long: time %.3f, partitions %.3f; mix / existing 1024-tap call: %.2f" % (
        med[k_mix] / med[k_long], n_mix / n_long, med[k_mix] / med[k_old]), flush=True)
    if not args.no_step:
        report("ECAPA-512 bf16 step, augment = dense 30 x 1024 bank", step_us(args, dense))
        report("ECAPA-512 bf16 step, augment = 27 x 1024 + 3 x 16000 bank", step_us(args, mix))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-direct", action="store_true")
    main(ap.parse_args())
