"""Times the --ADV_AUG train step (adversarial.AdversarialTrainer, profiles/adv_replay.md).

  python tools/bench_adv.py [--rounds 5] [--reps 5] [--shape 1|2|all] [--repo PATH]

Shape 1: ECAPA-TDNN-512 bf16-resident, B = 128, 4 s PCM, feat_len 400, heads (61, 28).
Shape 2: ResNet-18 fp32, B = 64, 4 s PCM, feat_len 750, same heads.  Both with recompute=True (the reference's step).
Variants: (a) eager with the module heads - only API that older trees have too; (b) eager with the fused heads;
(c) hipGraph replay of the two captured phases.  Device events around ``reps`` back-to-back steps give the step time, a
host clock around the same enqueue loop (before the synchronise) the host time per step; the variants alternate round by
round and the first two rounds only warm up.

``--repo PATH``: variant (a) is ALSO measured with the package imported from the built tree at PATH (a checkout of the
parent commit), in a fresh child process before and after this tree's rounds, one process on the GPU at a time.  That
number is the yardstick for (b) and (c); the two identical legs show the run-to-run spread.
Exits without a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HEADS = (61, 28)
SHAPES = {1: dict(model="ecapa", B=128, L=64000, feat_len=400), 2: dict(model="resnet", B=64, L=64000, feat_len=750)}


def make_trainer(shape, variant):
    import torch
    from asvspoof2021_air_amd.adversarial import AdversarialTrainer
    cfg = SHAPES[shape]
    torch.manual_seed(688)
    if cfg["model"] == "ecapa":
        from asvspoof2021_air_amd.ecapa_tdnn import Bottle2neck, Res2Net2
        model = Res2Net2(Bottle2neck, C=512, model_scale=8, nOut=2, n_mels=60)
        model.set_compute_dtype("bf16")
    else:
        from asvspoof2021_air_amd.resnet import ResNet
        model = ResNet(3, 256, resnet_type="18", nclasses=2)
    kw = dict(enc_dim=256, lr=5e-4, r_real=0.9, r_fake=0.2, alpha=20.0, feat_len=cfg["feat_len"],
              ecapa=cfg["model"] == "ecapa")
    if variant == "a":
        return AdversarialTrainer(model, HEADS, recompute=True, **kw)
    tr = AdversarialTrainer(model, HEADS, recompute=True, fused_heads=True, **kw)
    if variant == "c":
        tr.enable_graph()
    return tr


def batch(shape):
    import torch
    cfg = SHAPES[shape]
    g = torch.Generator().manual_seed(10)
    B = cfg["B"]
    pcm = (0.1 * torch.randn(B, cfg["L"], generator=g)).cuda()
    lab = (torch.arange(B) % 2).cuda()
    channels = torch.stack([torch.arange(B) % HEADS[0], torch.arange(B) % HEADS[1]], 1).cuda()
    return pcm, lab, channels


def timed(fn, reps):
    """(device ms per step, host ms per step to enqueue it)."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    host = time.perf_counter() - t0
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, host * 1e3 / reps


def measure(shape, variants, rounds, reps):
    import torch
    pcm, lab, ch = batch(shape)
    trainers = {v: make_trainer(shape, v) for v in variants}
    for v, tr in trainers.items():
        for _ in range(4):  # (c): two eager steps, the capture, one replay
            loss = tr.step(pcm, lab, channels=ch, epoch_num=1)[0]
        assert bool(torch.isfinite(loss)), v
        assert v != "c" or (tr._graph is not None and tr._graph.get("tail") is not None)
    out = {v: dict(ms=[], host_ms=[]) for v in variants}
    for r in range(rounds + 2):
        for v, tr in trainers.items():
            ms, host = timed(lambda: tr.step(pcm, lab, channels=ch, epoch_num=1), reps)
            if r >= 2:
                out[v]["ms"].append(ms)
                out[v]["host_ms"].append(host)
    return out


def line(name, res):
    ms, host = res["ms"], res["host_ms"]
    return "%-44s median %8.3f ms  min %8.3f  max %8.3f   host %7.3f ms / step" % (
        name, statistics.median(ms), min(ms), max(ms), statistics.median(host))


def parent_leg(args, shape):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--repo", args.repo, "--shape", str(shape),
           "--rounds", str(args.rounds), "--reps", str(args.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit("the leg on %s failed:\n%s" % (args.repo, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main(args):
    names = {"a": "(a) eager, module heads", "b": "(b) eager, fused heads", "c": "(c) hipGraph replay, fused heads"}
    for shape in ([1, 2] if args.shape == "all" else [int(args.shape)]):
        cfg = SHAPES[shape]
        print("shape %d: %s, B = %d, %d samples, feat_len %d, heads %s, recompute=True; %d rounds of %d steps" % (
            shape, cfg["model"], cfg["B"], cfg["L"], cfg["feat_len"], HEADS, args.rounds, args.reps), flush=True)
        before = parent_leg(args, shape) if args.repo else None
        if before:
            print(line("(a) on %s, before" % args.repo, before["a"]), flush=True)
        res = measure(shape, ["a", "b", "c"], args.rounds, args.reps)
        for v in ("a", "b", "c"):
            print(line(names[v], res[v]), flush=True)
        if args.repo:
            import torch
            torch.cuda.empty_cache()
            after = parent_leg(args, shape)
            print(line("(a) on %s, after" % args.repo, after["a"]), flush=True)
            m0, m1 = statistics.median(before["a"]["ms"]), statistics.median(after["a"]["ms"])
            print("spread of the two identical legs: %.3f ms (%.2f %%)" % (abs(m0 - m1), 100.0 * abs(m0 - m1) / min(m0, m1)),
                  flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", default="all", choices=["1", "2", "all"])
    ap.add_argument("--repo", default=None, help="a built tree of the parent commit: variant (a) is measured there too")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    # the package comes from --repo in the child, from this tree otherwise
    sys.path.insert(0, os.path.abspath(args.repo) if args.child else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_adv.py needs a GPU: there is nothing to measure without one")
    if args.child:
        print(json.dumps(measure(int(args.shape), ["a"], args.rounds, args.reps)))
    else:
        main(args)
