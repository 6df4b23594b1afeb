"""Times the CQCC front-end (csrc/cqcc.hip, profiles/cqcc.md) in one process.

  python tools/bench_cqcc.py [--rounds 5] [--reps 20] [--only dense,ragged] [--no-step] [--no-cpu] [--json PATH]

B = 64 rows of 64 000 samples (4 s), fp32, nine octaves.  CALL times (device events around ``reps`` back-to-back
calls, variants alternating round by round, the first round only warms up; median and min .. max of the rest):

  dense            CQCC.forward_padded(x, 750)                                        pyramid + products + tail
  ragged           CQCC.forward_ragged(x, lengths, 750), lengths uniform in [16 000, 64 000]
  spectrum         CQCC.forward_spectrum(x): pyramid + products; dense minus this is the tail
  top octaves      CQCC(n_octaves=2).forward_spectrum(x): no pyramid; products of two of the nine octaves
  LFCC             LFCC.forward_padded(x, 750), the launch the CQCC call stands beside
  bare MFMA loop   air_cqcc_mfma_loop: the product kernel's MFMA stream (3 independent v_mfma_f32_32x32x2_f32 per
                   wave, 4 waves per workgroup, 2 workgroups per CU) with nothing around it

The product kernel's share of the bare loop's rate is (MFMA flop it issues, zero rows of the tables included) /
(spectrum time) over the loop's TF - an underestimate of the kernel's own share by the pyramid's time.  The kernel-by-
kernel split comes from a kernel trace of this tool with --only dense (or ragged) --reps 2 --rounds 1 --no-step --no-cpu,
summarised by tools/prof_summary.py (profiles/cqcc.md).  --only names the variants to run by their first word; the
derived lines need all of them.

Unless --no-step: the replayed ResNet-18 train step (B = 64, feat_len 750) with frontend=CQCC() beside the LFCC step,
two trainers alternating.  Unless --no-cpu: the figure to beat - the same formulas in numpy complex64 on this host's
threads for 4 rows, scaled to 64."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from asvspoof2021_air_amd import _hip  # noqa: E402
from asvspoof2021_air_amd.feature_extraction import CQCC, LFCC  # noqa: E402

B, L, FEAT_LEN = 64, 64000, 750
T = 1 + L // 160


def events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps  # ms per call


def product_flops(n_octaves):
    """MFMA flop of the product kernel at (B, L): per (row, octave) ceil(T / 64) workgroups of 64 frames x 192 columns x
    KP rows (576 for the top octave, 1120 for the others), 2 flop per multiply-add."""
    tiles = -(-T // 64)
    return sum(B * tiles * 64 * 192 * (576 if o == 0 else 1120) * 2 for o in range(n_octaves))


def cpu_fp32(rows):
    """The oracle's formulas in fp32 numpy (complex64 products on the BLAS threads of this host), seconds per row."""
    import cqcc_oracle as co
    x = co.make_signal(rows, L, 7)
    h = co.fir().astype(np.float32)
    tabs = {r: (co.atom_table(r)[0].astype(np.complex64), co.atom_table(r)[1]) for r in (4.0, 8.0)}
    proj = co.projection().astype(np.float32)
    t0 = time.perf_counter()
    for b in range(rows):
        levels = [x[b]]
        for _ in range(7):
            levels.append(co.decimate(levels[-1], h).astype(np.float32))
        S = np.empty((T, 864), np.float32)
        for o in range(9):
            s = co.level_of(o)
            tab, H = tabs[4.0 if o == 0 else 8.0]
            F = co._frames(levels[s], (np.arange(T) * 160) >> s, H).astype(np.float32)
            X = F @ tab
            S[:, (8 - o) * 96:(9 - o) * 96] = np.log(X.real ** 2 + X.imag ** 2 + np.float32(co.EPS))
        c = S @ proj.T
        d1 = co.delta(c)
        np.concatenate([c, d1, co.delta(d1)], axis=1)
    return (time.perf_counter() - t0) / rows


def step_times(x, rounds):
    from asvspoof2021_air_amd.resnet import ResNet
    from asvspoof2021_air_amd.train import Trainer
    labels = (torch.arange(B) % 2).cuda()
    trainers = {}
    for name, fe in (("LFCC", None), ("CQCC", CQCC())):
        torch.manual_seed(0)
        tr = Trainer(ResNet(3, 256, resnet_type="18", nclasses=2), add_loss=None, frontend=fe, feat_len=FEAT_LEN)
        tr.enable_graph(True)
        for _ in range(4):  # two eager steps, the capture, one replay
            tr.step(x, labels)
        torch.cuda.synchronize()
        assert tr._graph is not None
        trainers[name] = tr
    times = {k: [] for k in trainers}
    for r in range(rounds + 1):
        for k, tr in trainers.items():
            t = events(lambda: tr.step(x, labels), 10)
            if r >= 1:
                times[k].append(t)
    return times


def main(args):
    g = torch.Generator().manual_seed(1)
    x = (0.1 * torch.randn(B, L, generator=g)).cuda()
    lengths = torch.randint(16000, L + 1, (B,), generator=g).to(torch.int32)
    ln = lengths.cuda()
    cq, cq2 = CQCC().cuda(), CQCC(n_octaves=2).cuda()
    lfcc = LFCC(320, 160, 512, 16000, 20).cuda()
    lfcc.mutate_input = False
    lib = _hip.lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sink = torch.zeros(4, device="cuda")
    blocks, iters = 2 * cus, 20000
    loop_flops = blocks * 4 * 3 * iters * 4096.0
    variants = {
        "dense (64, 60, 750)": lambda: cq.forward_padded(x, FEAT_LEN),
        "ragged (64, 60, 750)": lambda: cq.forward_ragged(x, ln, FEAT_LEN),
        "spectrum (64, 401, 864)": lambda: cq.forward_spectrum(x),
        "top octaves (64, 401, 192)": lambda: cq2.forward_spectrum(x),
        "LFCC padded (64, 60, 750)": lambda: lfcc.forward_padded(x, FEAT_LEN),
        "bare MFMA loop": lambda: _hip.check(lib.air_cqcc_mfma_loop(blocks, iters, _hip.dptr(sink), _hip.stream()), "loop"),
    }
    if args.only:
        variants = {k: v for k, v in variants.items() if k.split()[0] in args.only.split(",")}
    times = {k: [] for k in variants}
    for r in range(args.rounds + 1):
        for k, fn in variants.items():
            t = events(fn, args.reps if "loop" not in k else 2)
            if r >= 1:
                times[k].append(t)
    out = {}
    for k, v in times.items():
        out[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
        print("%-28s %9.3f ms  (min %.3f, max %.3f)" % (k, out[k]["median_ms"], min(v), max(v)), flush=True)
    if args.only:
        return
    loop_tf = loop_flops / (out["bare MFMA loop"]["median_ms"] * 1e9)
    spec_tf = product_flops(9) / (out["spectrum (64, 401, 864)"]["median_ms"] * 1e9)
    top_tf = product_flops(2) / (out["top octaves (64, 401, 192)"]["median_ms"] * 1e9)
    ragged_frames = int((1 + lengths // 160).sum())
    print("bare loop %.1f TF; products + pyramid at %.1f TF issued = %.0f %% of it; top two octaves alone %.1f TF = %.0f %%" % (
        loop_tf, spec_tf, 100 * spec_tf / loop_tf, top_tf, 100 * top_tf / loop_tf))
    print("MFMA flop issued %.3e (%.2f Mflop per frame); ragged batch holds %d of %d frames" % (
        product_flops(9), product_flops(9) / (B * T) / 1e6, ragged_frames, B * T))
    out["derived"] = {"loop_tf": loop_tf, "spectrum_tf": spec_tf, "top_octaves_tf": top_tf,
                      "product_flops": product_flops(9), "ragged_frames": ragged_frames, "frames": B * T, "cus": cus}
    if not args.no_step:
        st = step_times(x, args.rounds)
        for k, v in st.items():
            out["step " + k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
            print("replayed ResNet-18 step, %s: %8.3f ms  (min %.3f, max %.3f)" % (k, statistics.median(v), min(v), max(v)),
                  flush=True)
    if not args.no_cpu:
        per_row = cpu_fp32(4)
        out["cpu_fp32"] = {"s_per_row": per_row, "ms_per_batch": per_row * B * 1e3, "threads": torch.get_num_threads()}
        print("numpy fp32 on this host: %.3f s per row, %.0f ms per batch of 64" % (per_row, per_row * B * 1e3), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "B": B, "L": L, "feat_len": FEAT_LEN,
                       "rounds": args.rounds, "reps": args.reps, "results": out}, fh, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--json", default=None)
    main(ap.parse_args())
