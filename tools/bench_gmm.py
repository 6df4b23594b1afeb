"""Times the GMM back-end's kernels (gmm.DiagGMM, profiles/gmm_backend.md) in one process.

  python tools/bench_gmm.py [--windows 5] [--calls 8] [--no-host] [--out FILE.json]
  rocprofv3 --kernel-trace --pmc FETCH_SIZE -d DIR -o pmc -- python tools/bench_gmm.py --counter-pass

K = 512, D = 60 on a training batch's worth of frames ((64, 60, 401), the front-ends' layout) and on 2^20 frames
((N, 60)): time per accumulate (passes A + B + C), loglik (pass A + row means) and mstep (+ the operand repack).  The
fp64 matrix peak is in no guide, so the same run measures it: a bare loop of v_mfma_f64_16x16x4_f64
(air_debug_mfma_f64_probe) at 1, 2 and 4 workgroups of four waves per CU; the kernels' achieved rate is the MFMA flop they
issue (padding included, computed from the shapes below) over their time, held against the best probe figure.  The
algorithmic bytes and the bytes the kernels request are computed from the shapes as well; the HBM counters come from
profiler runs of their own over ``--counter-pass`` (tools/pmc_query.py reads the database; FETCH_SIZE is in KB and
counts a 128-byte request as 64, so it is doubled).  Reference point: one scikit-learn GaussianMixture EM iteration
(_e_step + _m_step) on the same frames on the host, at the thread count the environment sets (16 on the GPU hosts).
Protocol of profiles/device_corpus.md: one warm-up window, then ``--windows`` windows of ``--calls`` back-to-back
calls between two device events, median (min .. max) per call."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asvspoof2021_air_amd import _hip, gmm  # noqa: E402

K, D = 512, 60
DP, KT, TILE = 64, 32, 64  # D padded as the kernels pad it, 16-component tiles, frames per tile


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3  # us per call


def measure(variants, windows, calls):
    times = {k: [] for k in variants}
    for w in range(windows + 1):
        for k, fn in variants.items():
            us = window(fn, calls)
            if w >= 1:
                times[k].append(us)
    out = {}
    for k, us in times.items():
        out[k] = statistics.median(us)
        print("%-44s median %11.1f us  (%11.1f .. %11.1f)" % (k, out[k], min(us), max(us)), flush=True)
    return out


def frames(n_rows, n_cols, seed):
    """LFCC-like frames (coefficient 0 at 25, deviations from 1 down to 1e-2), (rows, D, cols) or (N, D) for one row."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    std = torch.logspace(0.0, -2.0, D, device="cuda")
    x = torch.randn(n_rows * n_cols, D, generator=g, device="cuda") * std
    x[:, 0] += 25.0
    return x if n_rows == 1 else x.view(n_rows, n_cols, D).transpose(1, 2).contiguous()


def mfma_flop(n, passes):
    """MFMA flop the kernels issue over n frame slots: per pass tiles x 16-component tiles x 4 row tiles x 2 Dp / 4
    k-steps (logits) or Dp / 8 column tiles x 4 (sums) - both 2 Dp / 4 x 4 MFMAs of 2048 flop."""
    return passes * (-(-n // TILE)) * KT * 4 * (2 * DP // 4) * 2048.0


def counter_pass():
    """The launches a counter run reads (rocprofv3 --pmc FETCH_SIZE, then WRITE_SIZE, each a run of its own): per
    frame set two warm-up calls, then three accumulate and three loglik calls; no timing, no host work."""
    init = frames(1, 4096, 3)
    for x in (frames(64, 401, 1), frames(1, 1 << 20, 2)):
        m = gmm.DiagGMM(K, D).init_from_frames(init, seed=0)
        m.begin()
        for _ in range(5):
            m.accumulate(x)
        for _ in range(5):
            m.score_rows(x)
        torch.cuda.synchronize()


def main(args):
    if args.counter_pass:
        return counter_pass()
    lib = _hip.lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    result = {"K": K, "D": D, "cus": cus}
    # ---- the measured fp64 matrix peak
    probe_out = torch.empty(4 * cus * 256, dtype=torch.float64, device="cuda")
    iters = 2000
    probes = {}
    for per_cu in (1, 2, 4):
        nb = per_cu * cus
        probes["bare f64 MFMA loop, %d workgroup(s) / CU" % per_cu] = (nb, lambda nb=nb: _hip.check(
            lib.air_debug_mfma_f64_probe(_hip.ci(nb), _hip.ci(iters), _hip.dptr(probe_out, torch.float64), _hip.stream()), "probe"))
    t = measure({k: v[1] for k, v in probes.items()}, args.windows, 2)
    rates = {k: probes[k][0] * 4 * iters * 4 * 2048.0 / (t[k] * 1e-6) / 1e12 for k in probes}
    for k, r in rates.items():
        print("%-44s %8.2f TFLOP/s" % (k, r), flush=True)
    peak = max(rates.values())
    result["probe_tflops"] = rates
    result["peak_tflops"] = peak
    # ---- the kernels
    sets = {"batch 64 x 401": frames(64, 401, 1), "2^20 frames": frames(1, 1 << 20, 2)}
    init = frames(1, 4096, 3)
    for name, x in sets.items():
        n = x.shape[0] * (x.shape[2] if x.dim() == 3 else 1)
        m = gmm.DiagGMM(K, D).init_from_frames(init, seed=0)
        m.begin().accumulate(x)
        m.m_step()  # one EM step: parameters a fit would actually see
        m.begin()
        calls = args.calls if n < 1 << 18 else max(1, args.calls // 4)
        t = measure({"accumulate  %s" % name: lambda: m.accumulate(x),
                     "loglik      %s" % name: lambda: m.score_rows(x),
                     "mstep+pack  %s" % name: lambda: (m.m_step(), m._operand())}, args.windows, calls)
        acc_us, lik_us = t["accumulate  %s" % name], t["loglik      %s" % name]
        issued = mfma_flop(n, 3)
        algo = 3 * 2.0 * n * K * 2 * D
        algo_bytes = n * D * 4 + 2 * (K + 2 * K * D) * 8           # the frames once, the model in, the statistics out
        asked = n * D * 4 * (1 + KT // 4) + n * 8 * (1 + KT // 4)  # pass A once, pass B once per 64-component chunk, + lse
        rec = {"frames": n, "accumulate_us": acc_us, "loglik_us": lik_us, "mstep_pack_us": t["mstep+pack  %s" % name],
               "accumulate_issued_tflops": issued / (acc_us * 1e-6) / 1e12,
               "accumulate_algorithmic_tflops": algo / (acc_us * 1e-6) / 1e12,
               "loglik_issued_tflops": mfma_flop(n, 1) / (lik_us * 1e-6) / 1e12,
               "algorithmic_bytes": algo_bytes, "requested_bytes": asked,
               "algorithmic_bytes_time_us_at_8TBs": algo_bytes / 8e12 * 1e6}
        rec["accumulate_share_of_measured_peak"] = rec["accumulate_issued_tflops"] / peak
        rec["loglik_share_of_measured_peak"] = rec["loglik_issued_tflops"] / peak
        for k, v in rec.items():
            print("    %-40s %s" % (k, ("%.4g" % v) if isinstance(v, float) else v), flush=True)
        if not args.no_host:
            gm = m.to_sklearn()
            xh = (x if x.dim() == 2 else x.transpose(1, 2).reshape(-1, D)).double().cpu().numpy()
            t0 = time.perf_counter()
            _, log_resp = gm._e_step(xh)
            gm._m_step(xh, log_resp)
            rec["sklearn_em_iteration_s"] = time.perf_counter() - t0
            rec["host_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count()
            print("    %-40s %.3f s at %d threads" % ("sklearn _e_step + _m_step", rec["sklearn_em_iteration_s"],
                                                    rec["host_threads"]), flush=True)
            del log_resp, xh
        result[name] = rec
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--counter-pass", action="store_true", help="only the launches a rocprofv3 --pmc run reads")
    if not torch.cuda.is_available():
        sys.exit("bench_gmm.py needs a GPU: there is nothing to measure without one")
    main(ap.parse_args())
