#!/usr/bin/env python3
"""What the embedding projections cost at the size of the reference's figure (profiles/embedding_vis.md): N = 10,003
points (a centre, 5,000 dev and 5,000 eval embeddings), D = 256, three synthetic clusters.  One process on one GPU.

  device   the phases of visualize.tsne_device, each timed alone on resident data - pairwise squared distances, the
           perplexity bisection, the joint distribution, and the descent (``--iters`` iterations, the default schedule) -
           then tsne_device and pca_device end to end.  Median of ``--runs`` runs (min .. max) behind one warm-up run each;
           a host clock around work that ends in a device synchronise.  The bytes and operations each phase needs are
           computed from the shapes beside the times.
  host     where scikit-learn imports: TSNE(perplexity=40, early_exaggeration=40) in its default form - Barnes-Hut, an
           APPROXIMATION of the objective the device minimises exactly - once, on this machine's CPUs (named in the
           output), with its kl_divergence_; ``--no-host`` skips it.

Usage: python tools/bench_tsne.py [--n 10003] [--d 256] [--iters 1000] [--runs 3] [--no-host] [--json out.json]
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from asvspoof2021_air_amd import ops, visualize  # noqa: E402


def synthetic(n, d, seed=3):
    rng = np.random.RandomState(seed)
    labels = np.arange(n) % 3
    centres = rng.randn(3, d) * 2.0
    return (centres[labels] + rng.randn(n, d)).astype(np.float32), labels


def timed(runs, fn):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return {"median_s": float(np.median(out)), "min_s": min(out), "max_s": max(out)}


def cpu_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10003)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsne.py measures on the GPU: none found")
    N, D = args.n, args.d
    x, labels = synthetic(N, D)
    X = torch.from_numpy(x).cuda()
    row = dict(n=N, d=D, iters=args.iters, gpu=torch.cuda.get_device_name(0))

    dist = torch.empty(N, N, device="cuda")
    cond = torch.empty(N, N, device="cuda")
    ws = torch.empty(ops.tsne_ws_bytes(N), dtype=torch.uint8, device="cuda")
    row["distances"] = timed(args.runs, lambda: ops.pairwise_sqdist(X, out=dist))
    row["distances"].update(flop=3.0 * N * N * D, bytes=4.0 * N * N + 4.0 * N * D)  # (fp64 sub, fma per term; one write)
    row["affinities"] = timed(args.runs, lambda: ops.tsne_affinities(dist, 40.0, out=cond))
    P = cond.clone()

    def joint():
        P.copy_(cond)
        ops.tsne_joint(P, ws)

    row["joint_with_copy"] = timed(args.runs, joint)
    row["joint_with_copy"].update(bytes=4.0 * N * N * 5)  # copy: read + write; row sums: read; symmetrise: read + write
    lr = max(N / 40.0 / 4.0, 50.0)
    y0 = visualize._pca_init(visualize.pca_device(X, 2).projection)
    y, update, gains = torch.empty_like(y0), torch.empty_like(y0), torch.empty_like(y0)
    status = ops.tsne_new_status("cuda")

    def descent():
        y.copy_(y0)
        ops.tsne_run(P, y, update, gains, status, max_iter=args.iters, learning_rate=lr, early_exaggeration=40.0, ws=ws)

    row["descent"] = timed(args.runs, descent)
    st = ops.tsne_read_status(status)
    checks = sum(1 for i in range(args.iters) if (i >= 250 and (i + 1) % 50 == 0) or i == args.iters - 1)
    row["descent"].update(n_iter=st["n_iter"], stopped=st["stopped"], kl=st["kl"],
                          bytes_P=4.0 * N * N * (args.iters + checks), pairs=float(N) * N * (2 * args.iters + checks))
    row["tsne_device_end_to_end"] = timed(args.runs, lambda: visualize.tsne_device(X, max_iter=args.iters))
    emb, kl, n_iter = visualize.tsne_device(X, max_iter=args.iters)
    row["tsne_device_end_to_end"].update(kl=kl, n_iter=n_iter)
    row["pca_device"] = timed(args.runs, lambda: visualize.pca_device(X, 2))
    e = emb.cpu().numpy().astype(np.float64)
    sub = np.random.RandomState(0).permutation(N)[:2000]  # nearest-neighbour purity on a sample (host, O(n^2))
    d2 = ((e[sub, None, :] - e[None, :, :]) ** 2).sum(2)
    d2[np.arange(len(sub)), sub] = np.inf
    row["device_nn_purity"] = float(np.mean(labels[np.argmin(d2, 1)] == labels[sub]))
    print(json.dumps(row), flush=True)

    if not args.no_host:
        try:
            from sklearn.manifold import TSNE
        except ImportError:
            TSNE = None
        if TSNE is not None:
            t0 = time.perf_counter()
            ts = TSNE(perplexity=40, early_exaggeration=40, random_state=88)
            eh = ts.fit_transform(x).astype(np.float64)
            host = dict(seconds=time.perf_counter() - t0, kl=float(ts.kl_divergence_), n_iter=int(ts.n_iter_),
                        method="barnes_hut (scikit-learn's default: approximate)", cpu=cpu_name(),
                        threads=int(os.environ.get("OMP_NUM_THREADS", 0)) or os.cpu_count())
            d2 = ((eh[sub, None, :] - eh[None, :, :]) ** 2).sum(2)
            d2[np.arange(len(sub)), sub] = np.inf
            host["nn_purity"] = float(np.mean(labels[np.argmin(d2, 1)] == labels[sub]))
            row["host_sklearn"] = host
            print(json.dumps({"host_sklearn": host}), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
