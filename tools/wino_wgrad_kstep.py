"""Winograd weight gradient (wino_wgrad_kernel): per-shape timing and the k-step cycle trace.

  AIR_HIP_LIB=<variant .so> python tools/wino_wgrad_kstep.py time   [reps]   # us per conv2d_wgrad call, 4 ResNet shapes
  AIR_HIP_LIB=<W2_TRACE .so> python tools/wino_wgrad_kstep.py trace          # cycle buckets, layer1 and layer3

`time` brackets `reps` back-to-back calls (the kernel and its reduce_partials_kernel) with events, five times, and
prints the median.  `trace` needs a library built with -DW2_TRACE=1 (build.py --variant): workgroup w's wave 0 adds
the cycles between consecutive stamps into trace[16 w + bucket]; the medians over the workgroups that ran a stage are
printed per stage and per k-step.  See profiles/wino_wgrad_kstep.md.
"""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asvspoof2021_air_amd import _hip, ops  # noqa: E402

SHAPES = {"layer1": (64, 64, 18, 750), "layer2": (64, 128, 9, 375), "layer3": (64, 256, 5, 188),
          "layer4": (64, 512, 3, 94)}
BUCKETS = ["prologue", "stage head", "k0", "k1", "k2", "k3", "k4", "k5", "k6", "k7", "dma_wait", "barrier", "epilogue",
           "stages"]


def tensors(shape):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(*shape, generator=g).cuda()
    dy = torch.randn(*shape, generator=g).cuda()
    return x, dy, (shape[1], shape[1], 3, 3)


def time_shapes(reps):
    for name, shape in SHAPES.items():
        x, dy, ws = tensors(shape)
        for _ in range(5):
            ops.conv2d_wgrad(x, dy, ws, 1, 1)
        runs = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                ops.conv2d_wgrad(x, dy, ws, 1, 1)
            e1.record()
            torch.cuda.synchronize()
            runs.append(e0.elapsed_time(e1) * 1e3 / reps)
        print("time %s %s: median %.2f us  (min %.2f max %.2f)" % (name, shape, statistics.median(runs), min(runs),
                                                                   max(runs)), flush=True)


def trace_shapes():
    lib = _hip.lib()
    if not hasattr(lib, "air_dbg_wino_wgrad_trace"):
        sys.exit("this library has no wgrad trace: build conv_wino.hip with -DW2_TRACE=1")
    lib.air_dbg_wino_wgrad_trace.argtypes = [ctypes.c_void_p]
    for name in ("layer1", "layer3"):
        x, dy, ws = tensors(SHAPES[name])
        for _ in range(3):
            ops.conv2d_wgrad(x, dy, ws, 1, 1)
        tr = torch.zeros(16 * 4096, dtype=torch.int64, device="cuda")
        lib.air_dbg_wino_wgrad_trace(ctypes.c_void_p(tr.data_ptr()))
        ops.conv2d_wgrad(x, dy, ws, 1, 1)
        torch.cuda.synchronize()
        lib.air_dbg_wino_wgrad_trace(ctypes.c_void_p(0))
        t = tr.cpu().view(-1, 16)
        t = t[t[:, 13] > 0].double()
        ns = t[:, 13].median().item()
        print("trace %s %s: %d workgroups, median %d stages each" % (name, SHAPES[name], t.shape[0], ns))
        per = {}
        for i, b in enumerate(BUCKETS[:13]):
            once = b in ("prologue", "epilogue")
            per[b] = (t[:, i] / (1.0 if once else t[:, 13])).median().item()
            print("  %-10s %9.0f cycles %s" % (b, per[b], "per launch" if once else "per stage"))
        ks = sum(per["k%d" % i] for i in range(8))
        stage = ks + per["stage head"] + per["dma_wait"] + per["barrier"]
        print("  k-step mean %.0f cycles; stage %.0f = 8 k-steps %.0f + boundary %.0f (%.1f %%)" % (
            ks / 8, stage, ks, stage - ks, 100.0 * (stage - ks) / stage), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    if mode == "trace":
        trace_shapes()
    else:
        time_shapes(int(sys.argv[2]) if len(sys.argv) > 2 else 50)
