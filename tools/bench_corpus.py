#!/usr/bin/env python3
"""What drawing a ragged batch out of the HBM-resident corpus costs (profiles/device_corpus.md).  One process, one GPU.

  gather    air_corpus_gather at B = 64 and 128 for Lcap = 64,000 and 208,000 samples, int16 and float32, over a store of
            ``--utterances`` utterances of exactly Lcap samples (so a batch moves B * Lcap elements, read once, written
            once) in a random permutation's order - fresh output tensors per batch, as CorpusSampler allocates them.
            Beside it, in the same run and alternating with it, a plain device-to-device copy of the same bytes
            (``torch.empty`` + ``copy_`` of a (B, Lcap) tensor).  Each window is ``--iters`` back-to-back calls between
            two device events after a warm-up window; ``--runs`` windows of each: median (min .. max).
  perm      air_corpus_permutation at n = 25,380 and 2^20, the same protocol.
  step      Trainer.step (ResNet-18, OC-Softmax head, hipGraph replay, B = 64, Lcap = 64,000 int16) fed by
            ``sampler.epoch()`` against the same step fed from tensors that are already resident, alternating.
  store     bytes per hour of audio of a store whose utterances are 1 .. 13 s long (host arithmetic: the alignment rule).

Usage: python tools/bench_corpus.py [--iters 32] [--runs 5] [--steps 32] [--json out.json] [--skip-step]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLAC_DECODE_MS_B64 = 8.87   # profiles/flac_decode.md: B = 64 x 4 s
RESNET_STEP_MS_B64 = 17.4   # README


def _window(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def _stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def _alternate(fns, iters, runs):
    """{name: per-call ms statistics}; one warm-up window each, then ``runs`` windows of each, alternating."""
    for fn in fns.values():
        _window(fn, iters)
    got = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            got[k].append(_window(fn, iters))
    return {k: _stats(v) for k, v in got.items()}


def build_corpus(torch, dtype, n, L, batch=128):
    from asvspoof2021_air_amd.corpus import DeviceCorpus
    corpus = DeviceCorpus(dtype).reserve(n * L, n)
    for lo in range(0, n, batch):
        B = min(batch, n - lo)
        if dtype == torch.int16:
            pcm = torch.randint(-32768, 32767, (B, L), dtype=torch.int16, device="cuda")
        else:
            pcm = torch.rand((B, L), dtype=torch.float32, device="cuda") - 0.5
        corpus.append(pcm, [L] * B, (np.arange(lo, lo + B) % 2))
    return corpus


def bench_gather(torch, args):
    from asvspoof2021_air_amd import ops
    rows = []
    for L in (64000, 208000):
        n = args.utterances if L == 64000 else args.utterances // 2
        for dtype in (torch.int16, torch.float32):
            corpus = build_corpus(torch, dtype, n, L)
            c = corpus
            perm = ops.corpus_permutation(0, n, 688, 0)
            for B in (64, 128):
                steps = n // B
                state = {"s": 0}
                src = torch.empty((B, L), dtype=dtype, device="cuda").copy_(corpus.samples[:B * L].view(B, L))

                def gather():
                    s = state["s"] = (state["s"] + 1) % steps
                    return ops.corpus_gather(c.samples, c.offsets, c.lengths, c.labels, c.tags, c.index, None, n,
                                             [(perm, s * B, B, 0)], 688, 750, 160, L)

                def copy():
                    return torch.empty((B, L), dtype=dtype, device="cuda").copy_(src)

                out = gather()
                idx = perm[state["s"] * B:(state["s"] + 1) * B]
                assert torch.equal(out[0], corpus.samples.view(n, L)[idx]) and torch.equal(out[6], idx)
                t = _alternate({"gather": gather, "copy": copy}, args.iters, args.runs)
                nbytes = 2.0 * B * L * src.element_size()  # read once, written once
                row = {"Lcap": L, "dtype": str(dtype).replace("torch.", ""), "B": B, "utterances": n,
                       "store_MB": corpus.sample_bytes / 1e6, "batch_MB": nbytes / 2e6, "gather_ms": t["gather"],
                       "copy_ms": t["copy"], "gather_TBps": nbytes / (t["gather"]["median"] * 1e-3) / 1e12,
                       "copy_TBps": nbytes / (t["copy"]["median"] * 1e-3) / 1e12,
                       "gather_over_copy_rate": t["copy"]["median"] / t["gather"]["median"]}
                rows.append(row)
                print("gather Lcap %6d %-7s B %3d: %.3f ms (%.3f .. %.3f) = %.2f TB/s | copy %.3f ms (%.3f .. %.3f) = %.2f TB/s | "
                      "rate ratio %.2f" % (L, row["dtype"], B, t["gather"]["median"], t["gather"]["min"], t["gather"]["max"],
                                           row["gather_TBps"], t["copy"]["median"], t["copy"]["min"], t["copy"]["max"],
                                           row["copy_TBps"], row["gather_over_copy_rate"]), flush=True)
            del corpus, c, perm, src
            torch.cuda.empty_cache()
    return rows


def bench_perm(torch, args):
    from asvspoof2021_air_amd import ops
    out = {}
    for n in (25380, 1 << 20):
        buf = torch.empty(n, dtype=torch.int64, device="cuda")
        gen = {"g": 0}

        def perm():
            gen["g"] += 1
            ops.corpus_permutation(0, n, 688, ops.corpus_stream(gen["g"], 0), out=buf)

        out[str(n)] = _alternate({"perm": perm}, max(8, args.iters // 2), args.runs)["perm"]
        print("permutation n = %7d: %.3f ms (%.3f .. %.3f)" % (n, out[str(n)]["median"], out[str(n)]["min"], out[str(n)]["max"]),
              flush=True)
    return out


def bench_step(torch, args):
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.resnet import ResNet
    from asvspoof2021_air_amd.train import Trainer
    B, L = 64, 64000
    corpus = build_corpus(torch, torch.int16, 2048, L)
    torch.manual_seed(0)
    tr = Trainer(ResNet(3, 256, resnet_type="18", nclasses=2), loss_module=AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0))
    tr.enable_graph()
    sampler = corpus.sampler(B, Lcap=L)
    resident = [next(sampler.epoch()) for _ in range(4)]
    it = {"gen": iter(()), "k": 0}

    def fed():
        b = next(it["gen"], None)
        if b is None:
            it["gen"] = sampler.epoch()
            b = next(it["gen"])
        tr.step(b.pcm, b.labels, start=b.start, lengths=b.lengths)

    def from_hbm():
        b = resident[it["k"] % 4]
        it["k"] += 1
        tr.step(b.pcm, b.labels, start=b.start, lengths=b.lengths)

    for _ in range(6):  # two eager steps, the capture, first replays
        from_hbm()
    torch.cuda.synchronize()
    t = _alternate({"sampler": fed, "resident": from_hbm}, args.steps, args.runs)
    print("step B 64 x 4 s: fed by sampler.epoch() %.3f ms (%.3f .. %.3f) | resident tensors %.3f ms (%.3f .. %.3f)" % (
        t["sampler"]["median"], t["sampler"]["min"], t["sampler"]["max"], t["resident"]["median"], t["resident"]["min"],
        t["resident"]["max"]), flush=True)
    return {"B": B, "Lcap": L, "graph": tr._graph is not None, "sampler_ms": t["sampler"], "resident_ms": t["resident"]}


def store_bytes_per_hour():
    rng = np.random.default_rng(0)
    lens = rng.integers(16000, 208001, 25380)
    held = (lens + 7) // 8 * 8
    hours = lens.sum() / 16000.0 / 3600.0
    return {"utterances": int(lens.size), "hours": float(hours), "int16_bytes_per_hour": float(2 * held.sum() / hours),
            "float32_bytes_per_hour": float(4 * held.sum() / hours), "gap_fraction": float((held - lens).sum() / lens.sum()),
            "int16_total_GB": float(2 * held.sum() / 1e9)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--utterances", type=int, default=2048)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    out = {"store": store_bytes_per_hour(), "flac_decode_ms_b64": FLAC_DECODE_MS_B64, "resnet_step_ms_b64": RESNET_STEP_MS_B64}
    print("store: %.0f bytes per hour of audio as int16 (%.4f %% alignment gaps), %.2f GB for %d utterances of 1 - 13 s" % (
        out["store"]["int16_bytes_per_hour"], 100 * out["store"]["gap_fraction"], out["store"]["int16_total_GB"],
        out["store"]["utterances"]))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_corpus.py measures on the GPU: none found")
    out["permutation_ms"] = bench_perm(torch, args)
    out["gather"] = bench_gather(torch, args)
    if not args.skip_step:
        out["step"] = bench_step(torch, args)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
