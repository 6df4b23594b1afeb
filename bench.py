#!/usr/bin/env python3
"""Headline benchmark: utterances/sec through ONE full train step of the hot path
(BASELINE.json configs[1]): fused HIP LFCC on 4 s @ 16 kHz synthetic PCM (already
resident in HBM) -> repeat-pad to feat_len 750 -> ResNet-18 forward -> OC-Softmax
(ang_iso) -> backward -> [RCCL all-reduce] -> Adam + SGD, fp32, batch 64 per GPU.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    (N > 1: python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...)

A plain run sets up, runs W warm-up steps, times ONE window of exactly K steps (value and
ms_per_step come from it), writes the last timed step's results with --dump-outputs, and
prints ONE JSON line on rank 0.  --full adds the other measurements:
  "windowed":     the same configuration again under the stability protocol (10-step windows
                  until steady, then --windows windows of max(K, 50) steps, median) with
                  clock / power samples
  "roofline":     dominant kernel (f32-MFMA implicit-GEMM conv) timed with HIP events on
                  its launch stream: algorithmic FLOPs / time vs the 157.3 TFLOP/s f32 peak,
                  HBM traffic from rocprofv3 --pmc child passes
  "configs":      ECAPA-TDNN-512 bf16, both models at T = 401, the Dataset-fed pipeline
  "cpu_baseline": the CPU oracle (a PyTorch-CPU port of the reference path, pinned to the
                  reference by tests/golden) timed on this box's host cores on a bounded
                  sample of BASELINE.json configs[0].
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch
import torch.distributed as td

BATCH = 64          # per-GPU batch (the reference's --batch_size, main_train.py:54)
LENGTH = 64000      # 4 s @ 16 kHz
FEAT_LEN = 750      # reference default --feat_len (main_train.py:43), padding='repeat'
PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_BF16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: v_mfma_f32_32x32x16_bf16 dense peak
PEAK_HBM_GBS = 8000.0
# Winograd kernels that do not report their issued MFMA FLOPs themselves (air_prof_collect2): F(2x2,3x3) and
# F(3x3,2x2) multiply 16 transformed values per 2x2 tile where the direct algorithm multiplies 36.  wino4_conv_kernel
# reports the exact count (30 or 36 positions per 3x4 / 4x4 tile, padded tiles included).
WINO_ISSUE = {"wino_conv_kernel": 16.0 / 36.0, "wino_wgrad_kernel": 16.0 / 36.0}
# kernel-name prefix (rocprofv3) of every template instance of a profiling family (csrc/air_prof.h)
PMC_FAMILY = {"wino4_conv_kernel": "wino4_conv_kernel", "wino_conv_kernel": "wino_conv_kernel",
              "wino_wgrad_kernel": "wino_wgrad_kernel", "c1b_gemm_kernel": "c1b_gemm", "c1b_fwd_kernel": "c1b_fwd",
              "c1b_tap_kernel": "c1b_tap"}


def smi_sample(device_index=0):
    """One clock / power / temperature sample of the GPU (amd-smi, else rocm-smi), so that a slow headline can be
    attributed from the record.  Never raises; {"error": ...} when no tool answers."""
    import shutil
    import subprocess
    out = {"t": round(time.time(), 1)}
    tool = shutil.which("amd-smi")
    try:
        if tool:
            r = subprocess.run([tool, "metric", "-g", str(device_index), "--clock", "--power", "--temperature", "--json"],
                               capture_output=True, text=True, timeout=20)
            if r.returncode == 0 and r.stdout.strip():
                j = json.loads(r.stdout)
                g = j[0] if isinstance(j, list) else (j.get("gpu_data", [j])[0] if isinstance(j, dict) else {})
                clk = g.get("clock", {})
                pick = {}
                for name in ("gfx_0", "mem_0"):
                    c = clk.get(name, {})
                    if isinstance(c, dict) and "clk" in c:
                        v = c["clk"]
                        pick[name + "_mhz"] = v.get("value") if isinstance(v, dict) else v
                pw = g.get("power", {})
                for name in ("socket_power", "current_socket_power", "average_socket_power"):
                    if name in pw:
                        v = pw[name]
                        pick["socket_power_w"] = v.get("value") if isinstance(v, dict) else v
                        break
                tp = g.get("temperature", {})
                for name in ("hotspot", "edge"):
                    if name in tp:
                        v = tp[name]
                        pick[name + "_c"] = v.get("value") if isinstance(v, dict) else v
                if pick:
                    out.update(pick, tool="amd-smi")
                    return out
        tool = shutil.which("rocm-smi")
        if tool:
            r = subprocess.run([tool, "-d", str(device_index), "-c", "-P", "-t", "--json"], capture_output=True, text=True,
                               timeout=20)
            if r.returncode == 0 and r.stdout.strip():
                j = json.loads(r.stdout)
                card = next(iter(j.values())) if isinstance(j, dict) and j else {}
                keep = {k: v for k, v in card.items() if any(w in k.lower() for w in ("sclk", "mclk", "power", "temperature (sensor junction)", "fclk"))}
                out.update(keep, tool="rocm-smi")
                return out
        out["error"] = "neither amd-smi nor rocm-smi answered"
    except Exception as exc:  # noqa: BLE001
        out["error"] = "%s: %s" % (type(exc).__name__, exc)
    return out


DUMP_LIMIT_BYTES = 64_000_000


def dump_outputs(path, loss, neg, trainer):
    """--dump-outputs: what the last timed step handed back and left behind, as float32 .npy files - loss.npy,
    neg_scores.npy (Trainer.step's return values) and state.npy (every floating tensor of the model's and the loss
    module's state_dicts after the optimiser step, flattened in state_dict order).  The state is a fixed seeded
    sample of its elements when the whole would exceed DUMP_LIMIT_BYTES."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    out = {"loss": loss.detach().reshape(1), "neg_scores": neg.detach().reshape(-1)}
    sds = (trainer.model.state_dict(), trainer.loss.state_dict())
    state = torch.cat([t.detach().reshape(-1).float() for sd in sds for t in sd.values() if t.is_floating_point()])
    room = (DUMP_LIMIT_BYTES - 4 * sum(v.numel() for v in out.values())) // 4 - 1024  # (.npy headers)
    if state.numel() > room:
        idx = torch.randperm(state.numel(), generator=torch.Generator().manual_seed(688))[:room].sort().values
        state = state[idx.to(state.device)]
    out["state"] = state
    for name, t in out.items():
        np.save(os.path.join(path, name + ".npy"), t.float().cpu().numpy())


def synth_batch(step, rank, device):
    g = torch.Generator(device=device).manual_seed(688 + rank * 1000 + step)
    pcm = 0.1 * torch.randn(BATCH, LENGTH, generator=g, device=device, dtype=torch.float32)
    labels = (torch.rand(BATCH, generator=g, device=device) < 0.9).long()
    labels[0] = 0
    labels[1] = 1
    return pcm, labels


def roofline_leg(trainer, batches):
    """Three eager warm steps, then three instrumented steps: every conv / LFCC launch is bracketed by HIP events on
    the launch stream inside the library (csrc/prof.hip)."""
    from asvspoof2021_air_amd import _hip
    lib = _hip.lib()
    lib.air_prof_kernel_name.restype = ctypes.c_char_p
    # kernels are timed one at a time: the side-stream overlap of the weight-gradient kernels
    # (resnet.py) is switched off for these two steps, otherwise the event brackets of
    # co-running kernels would include each other's time
    overlap = getattr(trainer.model, "overlap_wgrad", False)
    trainer.model.overlap_wgrad = False
    graphed, trainer.use_graph = trainer.use_graph, False  # eager launches: a replayed hipGraph records no events
    # (round 5: the timed steps are graph replays now, so the eager path is cold when this leg starts - its first
    # bracketed launches read 5 % above the rocprofv3 table of the same command; three eager steps first)
    NI = 3  # instrumented steps
    for i in range(3):
        trainer.step(*batches[i % len(batches)])
    torch.cuda.synchronize()
    lib.air_prof_enable(1)
    for i in range(NI):
        trainer.step(*batches[i % len(batches)])
    torch.cuda.synchronize()
    trainer.model.overlap_wgrad = overlap
    trainer.use_graph = graphed
    rows = []
    for kid in range(lib.air_prof_kernel_count()):
        n, ms, work, issued, nbytes = ctypes.c_int(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _hip.check(lib.air_prof_collect2(kid, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(work),
                                         ctypes.byref(issued), ctypes.byref(nbytes)), "air_prof_collect2")
        if n.value:
            name = lib.air_prof_kernel_name(kid).decode()
            rows.append({"kernel": name, "launches": n.value, "total_ms": ms.value, "work": work.value,
                         "issued": issued.value if issued.value != work.value else WINO_ISSUE.get(name, 1.0) * work.value,
                         "bytes": nbytes.value})
    lib.air_prof_enable(0)
    # wino4_conv_kernel launches whose epilogue also takes BatchNorm statistics (forward) or the BatchNorm-backward
    # sums (data gradient) are timed under "wino4_conv_kernel+bn": ONE family for the roofline - the same kernel, the
    # same MFMA work, plus a reduction that used to be a separate HBM pass - with the split reported beside it
    w4 = [r for r in rows if r["kernel"].startswith("wino4_conv_kernel")]
    split = None
    if len(w4) == 2:
        split = {r["kernel"]: {"launches_per_step": r["launches"] // NI, "avg_launch_ms": round(r["total_ms"] / r["launches"], 4),
                               "frac": round(r["issued"] / (r["total_ms"] * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4)} for r in w4}
        merged = {"kernel": "wino4_conv_kernel"}
        for k in ("launches", "total_ms", "work", "issued", "bytes"):
            merged[k] = w4[0][k] + w4[1][k]
        rows = [r for r in rows if not r["kernel"].startswith("wino4_conv_kernel")] + [merged]
    # the split-bf16 kernels report 6 bf16 MFMA FLOPs per algorithmic FLOP as "issued": their issued rate is against the
    # bf16 peak (2500 TF), the f32 kernels' against 157.3
    for r in rows:
        if r["kernel"].endswith("_bf3_kernel"):
            r["mfma"] = "bf16 (six products per fp32 product)"
    convs = [r for r in rows if r["kernel"].startswith(("conv", "wino", "c1b"))]
    dom = max(convs, key=lambda r: r["total_ms"])
    algorithmic = dom["work"] / (dom["total_ms"] * 1e-3) / 1e12
    all_flops = sum(r["work"] for r in convs)
    all_ms = sum(r["total_ms"] for r in convs)
    # the bf16 pointwise kernels (ECAPA, --dtype bf16) are priced against the bf16 MFMA peak
    peak = PEAK_BF16_MFMA_TFLOPS if dom["kernel"].startswith("c1b") else PEAK_F32_MFMA_TFLOPS
    # FLOPs a kernel puts through the matrix pipe per algorithmic FLOP (2 * MACs of the direct convolution,
    # SURVEY.md 8d): the Winograd kernels multiply 16 (F(2x2,3x3)) / 36 (F(4x4,3x3)) transformed values per
    # 2x2 / 4x4 output tile where the direct algorithm multiplies 36 / 144.  "achieved" and "frac" are the
    # ISSUED rate against the MFMA peak - a fraction of the roofline, never above 1 - and the
    # algorithmic-equivalent rate (what a direct kernel would have to sustain) is reported beside it.
    issue = dom["issued"] / dom["work"]
    achieved = algorithmic * issue
    out = {"bound": "mfma", "kernel": dom["kernel"], "achieved": round(achieved, 2),
           "peak": peak, "unit": "TFLOP/s", "frac": round(achieved / peak, 4),
           "traffic": None,
           "algorithmic_equivalent": round(algorithmic, 2), "issued_per_algorithmic_flop": round(issue, 4),
           "avg_launch_ms": round(dom["total_ms"] / dom["launches"], 4), "launches_per_step": dom["launches"] // NI,
           "all_conv_kernels": {"algorithmic_equivalent": round(all_flops / (all_ms * 1e-3) / 1e12, 2),
                                "ms_per_step": round(all_ms / NI, 3)}}
    # algorithmic HBM bytes per launch where the kernel states them (operands read once, results written once);
    # "traffic" (measured HBM-side bytes per launch) is filled in by pmc_traffic_leg() from PMC passes of THIS run
    if dom["bytes"] > 0:
        out["algorithmic_bytes"] = round(dom["bytes"] / dom["launches"])
    if split is not None and dom["kernel"] == "wino4_conv_kernel":
        out["instances"] = split
    if dom["kernel"] == "c1b_fwd_kernel":
        # ECAPA: the fused 512-channel pointwise kernel is HBM-bound on the fp32 tensors (127 FLOP per
        # algorithmic byte < 312 FLOP/B machine balance): price it on bytes as well.  4*(Cin+Cout) bytes
        # per 2*Cin*Cout FLOP = FLOPs / 128 at Cin = Cout = 512 (12 of its 16 launches per step).
        gbs = dom["work"] / 128.0 / (dom["total_ms"] * 1e-3) / 1e9
        out["hbm_view"] = {"bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                           "frac": round(gbs / PEAK_HBM_GBS, 4)}
    lf = [r for r in rows if r["kernel"] == "lfcc_kernel"]
    if lf:
        # A 35 us kernel inside a single event bracket reads ~20 us long (event -> kernel -> event dependency gaps:
        # round 3's line said 57.9 us where rocprofv3 says 34.9).  So the front-end kernel is timed over N = 50
        # back-to-back launches inside ONE bracket on the launch stream (= torch's current stream), the same
        # fused LFCC + pad + transpose call the train step makes; the single-bracket figure is kept beside it.
        pcm = batches[0][0]
        for _ in range(5):
            trainer.features(pcm)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        nrep = 50
        e0.record()
        for _ in range(nrep):
            trainer.features(pcm)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / nrep
        # 4 L + 4 T 60 = 352,240 B per 4 s utterance (PCM in, the T = 401 feature frames out) is THE
        # algorithmic figure; the launch also writes the repeat-padded frames 401..feat_len-1 (what the library counts)
        per_launch_bytes = lf[0]["work"] / lf[0]["launches"]
        nutt = pcm.shape[0]
        survey_bytes = nutt * (4 * pcm.shape[1] + 4 * (1 + pcm.shape[1] // 160) * 60)
        gbs = survey_bytes / (ms * 1e-3) / 1e9
        gbs_padded = per_launch_bytes / (ms * 1e-3) / 1e9
        out["lfcc_kernel"] = {"bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                              "frac": round(gbs / PEAK_HBM_GBS, 4), "avg_launch_ms": round(ms, 4),
                              "timing": "%d back-to-back launches in one event bracket" % nrep,
                              "algorithmic_bytes": round(survey_bytes),
                              "bytes_per_utt": round(survey_bytes / nutt),
                              "with_padded_output": {"bytes": round(per_launch_bytes), "achieved": round(gbs_padded, 1),
                                                     "frac": round(gbs_padded / PEAK_HBM_GBS, 4)},
                              "single_bracket_launch_ms": round(lf[0]["total_ms"] / lf[0]["launches"], 4)}
    out["per_kernel"] = [{"kernel": r["kernel"], "launches_per_step": r["launches"] // NI,
                          "ms_per_step": round(r["total_ms"] / NI, 3),
                          "algorithmic_rate": round(r["work"] / (r["total_ms"] * 1e-3) / 1e12, 2),
                          "issued_rate": round(r["issued"] / (r["total_ms"] * 1e-3) / 1e12, 2),
                          **({"mfma": r["mfma"]} if "mfma" in r else {})}
                         for r in rows]
    return out


def pmc_traffic_leg(model_name, family, argv_extra, timeout_s=170):
    """HBM-side bytes per launch of the dominant kernel, measured in THIS run: two plain child runs of this script
    (1 warm-up + 2 timed steps) under ``rocprofv3 --kernel-trace --pmc FETCH_SIZE`` and ``--pmc WRITE_SIZE`` -
    separate passes and the unit / gfx950 corrections as MI355X_MICROARCH.md prescribes (counters are KB;
    FETCH_SIZE tallies 128-byte requests at 64 B on gfx950: doubled; WRITE_SIZE as reported).  Returns a dict for
    the roofline object, with traffic = None and the reason when rocprofv3 is missing or a pass fails."""
    import shutil
    import sqlite3
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3")
    if prof is None:
        return {"traffic": None, "traffic_source": "rocprofv3 not on PATH: not measured in this run"}
    prefix = PMC_FAMILY.get(family, family)
    per, launches, whole = {}, 0, {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        with tempfile.TemporaryDirectory(dir="/tmp") as d:
            cmd = [prof, "--kernel-trace", "--pmc", counter, "-d", d, "-o", "pmc", "--", sys.executable,
                   os.path.join(ROOT, "bench.py"), "--model", model_name, "--steps", "2", "--warmup", "1"] + argv_extra
            env = dict(os.environ, TMPDIR="/tmp", PYTHONPATH=ROOT)
            try:
                r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=timeout_s)
            except subprocess.TimeoutExpired:
                return {"traffic": None, "traffic_source": "rocprofv3 --pmc %s pass timed out after %d s" % (counter, timeout_s)}
            dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(d) for f in fs if f.endswith(".db")]
            if r.returncode != 0 or not dbs:
                return {"traffic": None, "traffic_source": "rocprofv3 --pmc %s pass failed (rc %d)" % (counter, r.returncode)}
            try:
                cur = sqlite3.connect(dbs[0]).cursor()
                rows = cur.execute("select kernel_name, counter_name, value from counters_collection").fetchall()
            except sqlite3.Error as e:
                return {"traffic": None, "traffic_source": "rocpd database of the %s pass unreadable: %s" % (counter, e)}
        tot, n, everything = 0.0, 0, 0.0
        for k, c, v in rows:
            k = k.replace("(anonymous namespace)::", "").replace("void ", "")
            if c != counter:
                continue
            everything += v
            if k.startswith(prefix):
                tot += v
                n += 1
        # whole-step bytes: everything the child's kernels moved / the train steps the child actually ran, which it
        # reports itself (1 warm-up + 2 timed, plus the 2 eager steps and the capture pass in front of a hipGraph
        # replay: round 4 divided ECAPA's 6 steps by 3)
        nsteps = 3.0
        for ln in reversed(r.stdout.strip().splitlines()):
            if ln.startswith("{"):
                try:
                    nsteps = float(json.loads(ln).get("steps_run_total") or 3.0)
                except ValueError:
                    pass
                break
        whole[counter] = everything / nsteps
        whole["steps"] = nsteps
        if n == 0:
            return {"traffic": None, "traffic_source": "no %s launch in the %s pass" % (prefix, counter)}
        per[counter] = tot / n
        launches = n
    return {"traffic": round((2.0 * per["FETCH_SIZE"] + per["WRITE_SIZE"]) * 1024.0),
            "traffic_detail": {"fetch_kb_per_launch": round(per["FETCH_SIZE"], 1), "write_kb_per_launch": round(per["WRITE_SIZE"], 1),
                               "launches_sampled": launches,
                               "whole_step_bytes_all_kernels": round((2.0 * whole["FETCH_SIZE"] + whole["WRITE_SIZE"]) * 1024.0),
                               "whole_step_divisor_steps": whole["steps"]},
            "traffic_source": "measured in this run: child passes of this command under rocprofv3 --kernel-trace --pmc "
                              "FETCH_SIZE / --pmc WRITE_SIZE (separate passes); bytes = (2*FETCH_SIZE + WRITE_SIZE) KB per "
                              "launch, launch average over every %s* instance" % prefix}


def cpu_baseline_leg():
    """CPU oracle on BASELINE.json configs[0], bounded: per-utterance LFCC loop over 64 seeded
    4 s wavs (preprocess.py:239-244) + repeat-pad to 750 + ResNet-18/ang_iso train steps at
    batch 8 (3 warm-up + 5 timed, median)."""
    import numpy as np
    from oracle import lfcc as o_lfcc, pad as o_pad, resnet as o_resnet, train as o_train
    from oracle.filler import fill_state, fill_value, synth_pcm
    # 3 warm-up + 10 timed steps, plain MEDIAN, at a STATED thread count.  PyTorch-CPU's conv backward
    # collapses when oversubscribed (256 threads on a batch-8 problem ran 100x slower than 8), so "all cores" is not a
    # baseline anyone would run: the count is fixed at min(16, host threads) - the fastest of {8, 16, 32, 64} on every
    # box seen so far.  A 2-step sweep over those counts is reported beside it as `sweep` / `best` (VERDICT r4 item 12:
    # `value` is the plain median at the stated count, never a best-of).
    ncpu = os.cpu_count() or 1
    cores = min(16, ncpu)
    pcm = synth_pcm(64, LENGTH, seed=688)
    fb, dct = o_lfcc.linear_filterbank(), o_lfcc.dct2_ortho_matrix()
    torch.set_num_threads(cores)
    t0 = time.perf_counter()
    feats = [o_lfcc.lfcc_forward(pcm[i:i + 1].numpy().copy(), fb=fb, dct=dct) for i in range(64)]
    t_lfcc = time.perf_counter() - t0
    x = torch.stack([o_pad.repeat_pad(torch.from_numpy(f), FEAT_LEN) for f in feats[:8]])
    x = o_pad.to_model_input(x).contiguous()
    labels = torch.tensor([0, 1, 1, 1, 0, 1, 1, 1])
    tr = o_train.OracleTrainer("resnet", fill_state(o_resnet.resnet18_shapes()), fill_value("center", (1, 256)))
    times = []
    t_start = time.perf_counter()
    for it in range(13):
        t0 = time.perf_counter()
        tr.step(x, labels, None)
        times.append(time.perf_counter() - t0)
        if time.perf_counter() - t_start > 25.0 and len(times) >= 5:  # bounded sample
            break
    warm = min(3, len(times) - 2)
    step = float(np.median(times[warm:]))
    sweep = {}
    for nt in (8, 16, 32, 64):
        if nt > ncpu and sweep:
            break
        torch.set_num_threads(min(nt, ncpu))
        tr.step(x, labels, None)
        t0 = time.perf_counter()
        tr.step(x, labels, None)
        sweep[min(nt, ncpu)] = round(8.0 / (time.perf_counter() - t0), 2)
        if time.perf_counter() - t_start > 45.0:
            break
    torch.set_num_threads(cores)
    per_utt = t_lfcc / 64 + step / 8
    best_threads = max(sweep, key=sweep.get)
    return {"value": round(1.0 / per_utt, 2), "unit": "utt/s", "cores": cores,
            "host_cpu_count": os.cpu_count(), "kind": "port",
            "sample": "oracle (PyTorch-CPU port pinned to the reference by tests/golden): per-utterance LFCC over "
                      "64 seeded 4 s wavs (numpy rfft LFCC - not the reference's torch.stft route -, single un-warmed pass, "
                      "%.1f ms/utt) + ResNet-18/ang_iso train step batch 8, T=750, %d warm-up + "
                      "%d timed steps, plain median %.3f s/step at %d of %d host threads (PyTorch-CPU conv backward "
                      "collapses when oversubscribed: see sweep)" % (
                          1e3 * t_lfcc / 64, warm, len(times) - warm, step, cores, ncpu),
            "step_times_s": [round(t, 3) for t in times[warm:]],
            "sweep": {"unit": "train-step utt/s, one step after one warm-up step", "threads": sweep},
            "best": {"threads": best_threads, "train_step_utt_per_s": sweep[best_threads],
                     "note": "single-step figure from the sweep; not the reported value"},
            "lfcc_utt_per_s": round(64 / t_lfcc, 1), "train_step_utt_per_s": round(8 / step, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default="resnet", choices=["resnet", "ecapa"],
                    help="resnet = the headline config (BASELINE configs[1]); ecapa = ECAPA-TDNN-512 "
                         "(BASELINE configs[2], see --dtype)")
    ap.add_argument("--dtype", default=None, choices=["fp32", "bf16", "bf16c"],
                    help="ecapa only: bf16 = BASELINE configs[2] (pointwise convs on the bf16 matrix cores, "
                         "fp32 accumulate; default for --model ecapa), fp32 = the reference's arithmetic")
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch (default 64 resnet / 128 ecapa)")
    ap.add_argument("--feat-len", type=int, default=750,
                    help="model frames per utterance: 750 = the reference default (--feat_len, padding='repeat': "
                         "401 LFCC frames tiled to 750); 401 = the native frame count of 4 s audio")
    ap.add_argument("--augment", action="store_true",
                    help="on-the-fly IR-convolution channel augmentation of every utterance in the HIP front-end "
                         "(BASELINE configs[4]; 30 synthetic 1024-tap IRs)")
    ap.add_argument("--sync-each-step", action="store_true",
                    help="read the loss back on the host after every timed step, as the reference's loop does "
                         "(main_train.py:479-481 writes loss.item() to train_loss.log per iteration)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's results (loss, neg_scores, the model and loss state after the step) "
                         "as float32 DIR/<name>.npy, at most 64 MB in all; the inputs depend on the arguments alone")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement beyond the headline: the windowed protocol, roofline + PMC traffic, "
                         "exposed communication (N > 1), the extra configurations, the Dataset-fed leg, the CPU baseline")
    ap.add_argument("--windows", type=int, default=5, help="--full: windows of the windowed protocol (median reported)")
    ap.add_argument("--plain-timing", action="store_true",
                    help="--full: skip the windowed protocol (and with it the Dataset-fed leg and the A-B-A repeat)")
    ap.add_argument("--from-dataset", action="store_true",
                    help="--full: also time the configuration fed by DataLoader(ASVspoof2019 over a SyntheticSource) -> "
                         "pinned PCM -> copy stream -> Trainer.step (reported under configs.*_from_dataset; part of every "
                         "--full run without --plain-timing)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="--full: skip the roofline leg")
    ap.add_argument("--no-pmc", action="store_true",
                    help="--full: skip the two rocprofv3 --pmc child passes that measure roofline.traffic (N = 1, rank 0 only)")
    ap.add_argument("--no-extra-configs", action="store_true",
                    help="--full: skip the ECAPA-TDNN-512 bf16 and T = 401 legs reported under 'configs'")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.from_dataset and not args.full:
        ap.error("--from-dataset is one of the --full measurements: add --full")

    from asvspoof2021_air_amd import dist as air_dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit("--gpus %d needs one process per GPU: python -m torch.distributed.run "
                         "--nproc-per-node %d bench.py --gpus %d ..." % (args.gpus, args.gpus, args.gpus))
    # AIR_DIST_BACKEND=gloo lets the multi-process path run on a box with fewer GPUs than ranks
    # (tests/test_dist_gpu.py: two ranks share cuda:0); the driver's runs use RCCL ("nccl").
    backend = os.environ.get("AIR_DIST_BACKEND", "nccl")
    ndev = max(1, torch.cuda.device_count())
    local = int(os.environ.get("LOCAL_RANK", "0")) % ndev
    torch.cuda.set_device(local)
    air_dist.init_from_env(backend if world > 1 else None, device_index=local)
    rank = air_dist.rank()
    device = torch.device("cuda", local)

    from asvspoof2021_air_amd.train import Trainer
    global BATCH, FEAT_LEN
    FEAT_LEN = args.feat_len

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            td.barrier()
        torch.cuda.synchronize()

    def run_config(model_name, dtype, batch, steps, warmup, augment, want_roofline, nwin=3, dump_dir=None):
        """One configuration: W warm-up steps and ONE timed window of exactly K steps (barrier + synchronize fences,
        MAX over ranks) - the headline; the last step's results go to `dump_dir`.  With --full also the windowed
        protocol, the exposed communication (world > 1) and the instrumented roofline steps.  Returns (model, dict,
        retime, from_dataset) - retime(nwin) runs the windowed protocol on the same trainer again later in the process
        (the A-B-A repeat)."""
        global BATCH
        torch.manual_seed(688)
        if model_name == "resnet":
            from asvspoof2021_air_amd.resnet import ResNet
            model = ResNet(3, 256, resnet_type="18", nclasses=2)
            BATCH = batch or 64
        else:
            from asvspoof2021_air_amd.ecapa_tdnn import Bottle2neck, Res2Net2
            model = Res2Net2(Bottle2neck, C=512, model_scale=8, nOut=2, n_mels=60)
            model.set_compute_dtype(dtype or "bf16")
            BATCH = batch or 128
        # (Trainer broadcasts rank 0's weights, loss centre and BatchNorm buffers when world > 1)
        trainer = Trainer(model, enc_dim=256, lr=5e-4, r_real=0.9, r_fake=0.2, alpha=20.0,
                          feat_len=FEAT_LEN, device=device, ecapa=(model_name == "ecapa"))
        # hipGraph replay of front-end + forward + backward (train.py): bit-identical to the eager launches of the same
        # chain (tests/test_ecapa_gpu.py, tests/test_resnet_gpu.py).  Captured as ONE chain it needs ~0.2 ms of host
        # time per step instead of 4 - 7.  Round 5: the ResNet too (its attention noise comes from a device-side
        # Philox offset), and with world > 1 the gradient all-reduce runs behind the replay.  Defaults: ECAPA always;
        # ResNet at N = 1 - with N > 1 it stays eager with the all-reduce in buckets from inside backward (BASELINE
        # configs[3]: "overlapped with backward").  AIR_GRAPH=0 / 1 forces eager / replay everywhere.
        want_graph = os.environ.get("AIR_GRAPH", "")
        # (the IR augmentation runs in front of the captured region - its per-utterance draw is host state - and hands
        # its output to the replay like any other batch)
        # Round 6: with world > 1 the replay is SEGMENTED (Trainer.enable_graph: several graphs cut at backward's bucket
        # boundaries, each bucket's all-reduce launched between two replays), so both models replay at every N - the
        # N = 1 and N = 8 legs of a scaling curve run the same launch mode.  AIR_GRAPH=0 -> eager with buckets from
        # inside backward; AIR_GRAPH_SEGMENTS=0 -> one chain + the whole exchange behind it.
        if want_graph != "0":
            trainer.enable_graph()
        if augment:
            from asvspoof2021_air_amd.augment import ChannelAugment
            trainer.augment = ChannelAugment(p=1.0, seed=688 + rank, device=device)
        nb = max(2, min(4, steps + warmup))
        batches = [synth_batch(i, rank, device) for i in range(nb)]  # inputs resident in HBM
        nrun = [0]

        def window(n):
            """n steps between barrier + synchronize fences; (seconds, host-issue seconds, the last step's (loss,
            neg_scores)), MAX over ranks."""
            fence()
            t0 = time.perf_counter()
            last = None
            for i in range(n):
                last = trainer.step(*batches[i % nb])
                if args.sync_each_step:
                    last[0].item()
            t_host = time.perf_counter() - t0  # all launches issued (the host side of the step; the GPU is behind)
            fence()
            dt = time.perf_counter() - t0
            nrun[0] += n
            if world > 1:
                t = torch.tensor([dt], device=device, dtype=torch.float64)
                td.all_reduce(t, op=td.ReduceOp.MAX)
                dt = float(t.item())
            return dt, t_host, last

        def launch_mode():
            if trainer.use_graph and trainer._graph is not None and trainer._graph.get("segments"):
                return ("hipGraph replay (%d segments, a bucket's all-reduce between two replays) + optimiser launches"
                        % len(trainer._graph["segments"]))
            return "hipGraph replay (one chain) + optimiser launches" if trainer.use_graph else "eager"

        def windowed(nwin):
            """--full: the stability protocol on the warm trainer; a dict of its median window and how it was taken."""
            smi0 = smi_sample(local) if rank == 0 else None
            # Round 5 (the round-4 headline was taken 0.1 s after start on a cold box and read 11 %
            # low).  Warm-up by TIME and STABILITY: 10-step windows until >= 2 s have been run and three consecutive
            # windows agree within 1 % (capped at 12 s; the decision uses the all-reduced MAX, so every rank leaves the
            # loop together).  Then `nwin` windows of max(K, 50) steps; value = the MEDIAN window.
            settle, t_settle = [], 0.0
            while True:
                dt, _, _ = window(10)
                settle.append(1e3 * dt / 10)
                t_settle += dt
                last3 = settle[-3:]
                stable = len(last3) == 3 and (max(last3) - min(last3)) <= 0.01 * min(last3)
                if (t_settle >= 2.0 and stable) or t_settle >= 12.0:
                    break
            wsteps = max(steps, 50)
            wins = [window(wsteps) for _ in range(nwin)]
            timing = {"protocol": "after the headline window: 10-step windows until >= 2 s and three consecutive windows "
                                  "within 1 %% (cap 12 s), then %d windows of max(K, 50) = %d steps between barrier + "
                                  "synchronize fences; value and ms_per_step are the MEDIAN window" % (nwin, wsteps),
                      "settle_windows_ms_per_step": [round(v, 3) for v in settle], "settle_s": round(t_settle, 2),
                      "settled": bool(stable)}
            per = sorted(1e3 * w[0] / wsteps for w in wins)
            med = per[len(per) // 2] if len(per) % 2 else 0.5 * (per[len(per) // 2 - 1] + per[len(per) // 2])
            dt = med * 1e-3 * wsteps
            t_host = sorted(w[1] for w in wins)[len(wins) // 2]
            last = wins[-1][2][0]
            timing.update({"steps_per_window": wsteps, "windows_ms_per_step": [round(1e3 * w[0] / wsteps, 3) for w in wins],
                           "min_ms_per_step": round(per[0], 3), "max_ms_per_step": round(per[-1], 3),
                           "spread": round((per[-1] - per[0]) / med, 4)})
            if smi0 is not None:
                timing["smi_before"], timing["smi_after"] = smi0, smi_sample(local)
                # The clock the compute units run at DURING the steps (amd-smi above is sampled with the GPU idle): one
                # probe wave on a side stream (air_debug_clock_probe) beside 20 further, untimed steps.  The MFMA-dense
                # kernels are power-capped well below the 2.4 GHz that the peaks in `roofline` are quoted at.
                try:
                    if world > 1:
                        raise RuntimeError("single-process runs only (the extra steps would need every rank)")
                    from asvspoof2021_air_amd.ops import ClockProbe
                    import numpy as np
                    n_probe = 20
                    probe = ClockProbe(device, n_samples=int(min(45000, n_probe * med * 1e3 / 100.0 * 1.5 + 200)), interval_us=100.0)
                    probe.start()
                    time.sleep(0.002)
                    for i in range(n_probe):  # (no fence: a device-wide synchronize would wait for the probe itself)
                        trainer.step(*batches[i % nb])
                    nrun[0] += n_probe
                    torch.cuda.current_stream(device).synchronize()
                    t, f = probe.samples()
                    sel = f[(t > 1000.0) & (t < n_probe * med * 1e3)]
                    if sel.size:
                        timing["core_clock_mhz_during_steps"] = {
                            "median": round(float(np.median(sel)), 1), "p10": round(float(np.percentile(sel, 10)), 1),
                            "p90": round(float(np.percentile(sel, 90)), 1), "min": round(float(sel.min()), 1),
                            "max": round(float(sel.max()), 1), "samples": int(sel.size), "interval_us": 100.0,
                            "how": "s_memtime / 100 MHz wall clock sampled by one wave on a side stream beside %d untimed steps" % n_probe}
                except Exception as e:  # instrumentation only
                    timing["core_clock_mhz_during_steps"] = {"error": repr(e)[:200]}
            return {"value": round(world * BATCH * wsteps / dt, 2), "unit": "utt/s", "ms_per_step": round(1e3 * dt / wsteps, 3),
                    "final_loss": round(float(last.item()), 5), "host_issue_ms_per_step": round(1e3 * t_host / wsteps, 3),
                    "steps_timed_per_window": wsteps, "windows": len(wins), "timing": timing}

        if trainer.use_graph:  # two eager steps + the capture happen before the W warm-up steps, never inside the timed ones
            for i in range(3):
                trainer.step(*batches[i % nb])
            nrun[0] += 3
        for i in range(warmup):
            trainer.step(*batches[i % nb])
        nrun[0] += warmup
        # the headline: ONE window of exactly K steps
        dt, t_host, (last_loss, last_neg) = window(steps)
        if dump_dir is not None and rank == 0:
            dump_outputs(dump_dir, last_loss, last_neg, trainer)
        step_s = dt / steps
        res = {"value": round(world * BATCH * steps / dt, 2), "unit": "utt/s", "steps": steps, "warmup": warmup,
               "ms_per_step": round(1e3 * step_s, 3), "per_gpu_batch": BATCH, "global_batch": world * BATCH,
               "final_loss": round(float(last_loss.item()), 5), "host_issue_ms_per_step": round(1e3 * t_host / steps, 3),
               "launch": launch_mode(), "steps_timed_per_window": steps, "windows": 1,
               "timing": {"protocol": "W warm-up steps (behind the two eager steps + capture of a hipGraph replay), then ONE "
                                      "window of exactly K steps between barrier + synchronize fences"}}
        if args.full and not args.plain_timing:
            res["windowed"] = windowed(nwin)
        comm = None
        if args.full and world > 1:
            # exposed communication: the same steps without the gradient exchange (no buckets from inside
            # backward, no all-reduce; replicas drift apart, which no later figure depends on), MAX over ranks
            arena = model.arena()
            ar_bytes = 4 * (arena.head_total + sum(p.numel() for p in trainer.loss.parameters()))
            saved = (trainer.world, getattr(model, "_bucketer", None))
            trainer.world, model._bucketer = 1, None
            k2 = max(2, min(steps, 5))
            trainer.step(*batches[0])
            fence()
            t1 = time.perf_counter()
            for i in range(k2):
                trainer.step(*batches[i % nb])
            fence()
            d2 = torch.tensor([(time.perf_counter() - t1) / k2], device=device, dtype=torch.float64)
            td.all_reduce(d2, op=td.ReduceOp.MAX)
            trainer.world, model._bucketer = saved
            trainer.sync_from_rank0()
            comm = {"allreduce_bytes_per_step": ar_bytes, "step_ms_without_exchange": round(1e3 * float(d2.item()), 3),
                    "exposed_ms": round(1e3 * (step_s - float(d2.item())), 3),
                    "overlap": os.environ.get("AIR_DDP_OVERLAP", "1") == "1"}
        # The instrumented roofline steps are ordinary train steps: with world > 1 they contain the gradient
        # all-reduce, so EVERY rank runs them (rank 0 alone would wait for its peers forever); only rank 0 reports.
        if want_roofline:
            res["roofline"] = roofline_leg(trainer, batches)
            nrun[0] += 6
        bucketer = getattr(model, "_bucketer", None)
        seg_b = getattr(trainer, "_seg_bucketer", None)
        res["ddp"] = {"device": "cuda:%d" % local, "world": world,
                      "buckets_in_backward": (bucketer.total_launched if bucketer is not None else 0),
                      "buckets_between_replays": (seg_b.total_launched if seg_b is not None else 0)}
        if world > 1:
            # self-documenting first multi-GPU run: what the process group actually is
            res["ddp"].update(backend=td.get_backend(), ranks_seen=td.get_world_size(),
                              nccl_version=(".".join(str(v) for v in torch.cuda.nccl.version())
                                            if td.get_backend() == "nccl" else None),
                              devices_visible=torch.cuda.device_count())
        if comm is not None:
            res["ddp"]["communication"] = comm
        res["steps_run_total"] = nrun[0]

        def from_dataset(nwin=3, wsteps=50):
            """the same trainer fed by the drop-in Dataset surface instead of HBM-resident batches -
            ``ASVspoof2019`` over a ``SyntheticSource`` (the separable corpus of synth.py, 4 s waveforms generated once:
            they stand for the corpus on disk), ``return_pcm='batch'`` + ``collate_fn`` (one pinned (B, L) host tensor per
            batch), ``DataLoader(shuffle=True, num_workers=0)`` (the reference's default, main_train.py:63),
            ``DevicePrefetcher`` (H2D of batch n + 1 on a copy stream under step n).  main_train.py:310-348's loop
            body with the features made by the trainer's fused front-end inside the replayed graph."""
            from torch.utils.data import DataLoader
            from asvspoof2021_air_amd import dataset as air_ds
            nutt = 4 * BATCH
            src = air_ds.SyntheticSource(688 + rank, nutt, length=LENGTH, device=device, cache_items=None)
            ds = air_ds.ASVspoof2019("LA", None, "train", feat_len=FEAT_LEN, padding="repeat", source=src,
                                     return_pcm="batch")
            t0 = time.perf_counter()
            for i in range(nutt):
                src.pcm(i)
            gen_s = time.perf_counter() - t0
            dl = DataLoader(ds, batch_size=BATCH, shuffle=True, drop_last=True, collate_fn=ds.collate_fn, num_workers=0)
            t0 = time.perf_counter()
            nb_host = 0
            for _ in dl:  # host side alone: __getitem__ x B + the pinned stack
                nb_host += 1
            host_ms = 1e3 * (time.perf_counter() - t0) / max(1, nb_host)

            def batches_forever():
                while True:
                    for b in air_ds.DevicePrefetcher(dl, device, depth=2):
                        yield b

            it = batches_forever()

            def win(n):
                fence()
                t0 = time.perf_counter()
                last = None
                for _ in range(n):
                    b = next(it)
                    last, _ = trainer.step(b[0], b[3])
                fence()
                dt = time.perf_counter() - t0
                if world > 1:
                    t = torch.tensor([dt], device=device, dtype=torch.float64)
                    td.all_reduce(t, op=td.ReduceOp.MAX)
                    dt = float(t.item())
                return dt, last

            win(10)
            wins = [win(wsteps) for _ in range(nwin)]
            per = sorted(1e3 * w[0] / wsteps for w in wins)
            med = per[len(per) // 2]
            out = {"value": round(world * BATCH * 1e3 / med, 2), "unit": "utt/s", "ms_per_step": round(med, 3),
                   "windows_ms_per_step": [round(1e3 * w[0] / wsteps, 3) for w in wins], "steps_timed_per_window": wsteps,
                   "final_loss": round(float(wins[-1][1].item()), 5),
                   "host_loader_ms_per_batch": round(host_ms, 3), "h2d_bytes_per_step": BATCH * LENGTH * 4 + BATCH * 8,
                   "corpus": "%d synthetic 4 s utterances (synth.py), generated once in %.1f s, shuffled every epoch" % (nutt, gen_s),
                   "pipeline": "ASVspoof2019(SyntheticSource, return_pcm='batch').collate_fn -> pinned (B, L) -> "
                               "DevicePrefetcher (copy stream, depth 2) -> Trainer.step (fused LFCC inside the replay)",
                   "vs_resident": round((world * BATCH * 1e3 / med) / res.get("windowed", res)["value"], 4)}
            return out

        return model, res, windowed, from_dataset

    model, main_res, retime_main, dataset_main = run_config(args.model, args.dtype, args.batch, args.steps, args.warmup,
                                                            args.augment, args.full and not args.no_roofline,
                                                            nwin=args.windows, dump_dir=args.dump_outputs)
    roofline = main_res.pop("roofline", None)
    main_batch = BATCH
    # BASELINE configs[2] (ECAPA-TDNN-512, bf16 compute, batch 128 per GPU) rides along in a --full run so
    # that its bench line carries a measured number for it too
    extra = {}
    if args.full and args.model == "resnet" and not args.no_extra_configs and args.batch == 0 and not args.augment:
        # (the headline's model and trainer stay alive for the A-B-A repeat at the end: 288 GB of HBM)
        # (a failure of this additional leg must not cost the headline line; with world > 1 every rank takes the
        # same path through its collectives, so an exception there is not caught - it would desynchronise the ranks)
        try:
            _, e, _, _ = run_config("ecapa", "bf16", 0, args.steps, args.warmup, False, not args.no_roofline)
            e["metric"] = "utterances/sec (LFCC+ECAPA-TDNN-512-OCSoftmax train step, 4 s@16 kHz)"
            e["dtype"] = "bf16"
            e["workload"] = ("BASELINE configs[2]: fused HIP LFCC + ECAPA-TDNN-512 + OC-Softmax train step, bf16-resident "
                             "activations (pointwise and dilated convs on v_mfma_f32_32x32x16_bf16, fp32 accumulate), T=401 "
                             "repeat-padded to %d" % FEAT_LEN)
            extra["ecapa_bf16_b128"] = e
        except Exception as exc:  # noqa: BLE001
            if world > 1:
                raise
            extra["ecapa_bf16_b128"] = {"error": "%s: %s" % (type(exc).__name__, exc)}
        # the native frame count of 4 s audio ("frame count must be stated with every number"): both models
        # without the reference's repeat-padding to feat_len 750, same steps / warm-up, no instrumented legs
        if FEAT_LEN != 401:
            keep_len = FEAT_LEN
            for key, (mname, mdt) in (("resnet_f32_b64_t401", ("resnet", None)), ("ecapa_bf16_b128_t401", ("ecapa", "bf16"))):
                try:
                    FEAT_LEN = 401
                    torch.cuda.empty_cache()
                    _, e, _, _ = run_config(mname, mdt, 0, args.steps, args.warmup, False, False)
                    e["dtype"] = "bf16" if mdt else "f32"
                    e["workload"] = "the same train step at the native T = 401 frames (no repeat-padding)"
                    extra[key] = e
                except Exception as exc:  # noqa: BLE001
                    if world > 1:
                        raise
                    extra[key] = {"error": "%s: %s" % (type(exc).__name__, exc)}
                finally:
                    FEAT_LEN = keep_len
        model = None
    BATCH = main_batch
    # roofline.traffic: measured now, by PMC child passes of this same command (N = 1 only: rocprofv3 around one
    # rank of a multi-process job would profile that rank alone)
    if rank == 0 and world == 1 and roofline is not None and not args.no_pmc:
        passthru = ["--feat-len", str(args.feat_len)] + (["--batch", str(args.batch)] if args.batch else [])
        if args.model == "ecapa" and args.dtype:
            passthru += ["--dtype", args.dtype]
        if args.augment:
            passthru += ["--augment"]
        torch.cuda.empty_cache()
        roofline.update(pmc_traffic_leg(args.model, roofline["kernel"], passthru))
        e = extra.get("ecapa_bf16_b128")
        if e is not None and "roofline" in e:
            e["roofline"].update(pmc_traffic_leg("ecapa", e["roofline"]["kernel"], ["--feat-len", str(args.feat_len)]))

    # the headline configuration fed through the Dataset surface (DataLoader -> pinned PCM -> copy stream -> Trainer.step)
    if args.full and (args.from_dataset or (extra and not args.plain_timing)) and not args.augment:
        BATCH = main_batch
        try:
            extra["%s_from_dataset" % ("resnet_f32_b64" if args.model == "resnet" else "ecapa_b128")] = dataset_main()
        except Exception as exc:  # noqa: BLE001
            if world > 1:
                raise
            extra["from_dataset"] = {"error": "%s: %s" % (type(exc).__name__, exc)}
    # A-B-A: the windowed protocol of the headline configuration once more at the END of the process (same trainer, no
    # warm-up beyond the stability windows), so that a drift between the first and the last leg shows in the record
    repeat = None
    if args.full and not args.plain_timing and extra:
        BATCH = main_batch
        r2 = retime_main(3)
        repeat = {k: r2[k] for k in ("value", "ms_per_step", "host_issue_ms_per_step", "timing")}
        repeat["vs_first"] = round(r2["value"] / main_res["windowed"]["value"], 4)
    if rank == 0:
        line = {
            "metric": "utterances/sec (LFCC+ResNet-OCSoftmax train step, 4 s@16 kHz)",
            "value": main_res["value"], "unit": "utt/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": main_res["ms_per_step"], "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "BASELINE configs[1]: fused HIP LFCC(320,160,512,20 filters) + ResNet-18 + "
                                   "OC-Softmax(ang_iso) fp32 train step (fwd+bwd+Adam+SGD), 4 s @ 16 kHz PCM in HBM, "
                                   "T=401 frames repeat-padded to feat_len=%d" % FEAT_LEN,
                       "global_batch": world * BATCH, "per_gpu_batch": BATCH, "feat_len": FEAT_LEN,
                       "parallelism": "dp%d" % world},
            "final_loss": main_res["final_loss"],
            "host_issue_ms_per_step": main_res["host_issue_ms_per_step"],
            "launch": main_res["launch"],
            # value / ms_per_step: ONE window of exactly `steps` timed steps (--full reports its windowed protocol under
            # `windowed`)
            "steps_timed_per_window": main_res["steps_timed_per_window"], "windows": main_res["windows"],
            "timing": main_res["timing"], "steps_run_total": main_res["steps_run_total"],
            "sync_each_step": bool(args.sync_each_step),
            "ddp": main_res["ddp"],
        }
        if args.model == "ecapa":
            line["metric"] = "utterances/sec (LFCC+ECAPA-TDNN-512-OCSoftmax train step, 4 s@16 kHz)"
            dt = args.dtype or "bf16"
            line["dtype"] = "bf16" if dt in ("bf16", "bf16c") else "f32"
            line["config"]["workload"] = (
                "BASELINE configs[2]: fused HIP LFCC + ECAPA-TDNN-512 + OC-Softmax train step, T=401 repeat-padded to "
                "%d, " % FEAT_LEN + ("bf16-resident activations (every (B,C,T) tensor bf16 in HBM; K=1 and dilated K=3 convs on "
                           "v_mfma_f32_32x32x16_bf16 with fp32 accumulate; statistics, parameters and gradients fp32)"
                           if dt == "bf16" else
                           "bf16 compute on fp32 tensors (rounds 1-2 arithmetic)" if dt == "bf16c" else
                           "fp32 compute (the reference's arithmetic; configs[2] itself is the bf16 variant)"))
        if args.augment:
            line["config"]["workload"] += "; + on-the-fly IR convolution (1024 taps) of every utterance ahead of LFCC"
        if "windowed" in main_res:
            line["windowed"] = main_res["windowed"]
        if roofline is not None:
            line["roofline"] = roofline
        if extra:
            line["configs"] = extra
        if repeat is not None:
            line["headline_repeat_at_end"] = repeat
        if args.full and world == 1 and not args.no_cpu_baseline and args.model == "resnet":
            try:
                line["cpu_baseline"] = cpu_baseline_leg()
            except Exception as exc:  # noqa: BLE001  (the headline line still goes out)
                line["cpu_baseline"] = {"value": None, "error": "%s: %s" % (type(exc).__name__, exc)}
        text = json.dumps(line)
        # ONE write of the whole line (print() may split a line longer than the pipe buffer into several writes, between
        # which another rank's output can land when N processes share the launcher's stdout)
        sys.stdout.flush()
        os.write(sys.stdout.fileno(), (text + "\n").encode())
        out_path = os.environ.get("AIR_BENCH_JSON_OUT")  # tests: the same line into a file as well
        if out_path:
            with open(out_path, "w") as f:
                f.write(text + "\n")
    if world > 1:
        td.barrier()
        td.destroy_process_group()


if __name__ == "__main__":
    main()
