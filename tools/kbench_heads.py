"""Times the loss heads of csrc/loss_heads.hip (P2SGrad, Isolate, IsolateSquare forward / backward, AMSoftmax forward)
and, for reference, the OC-Softmax and CE kernels, at B = 64 and 128; then (--steps) the hipGraph-replayed train step
of ResNet-18 and LCNN at B = 64, 4 s, under each Trainer head.  Numbers: profiles/loss_heads.md."""
import argparse
import json
import time

import torch

from asvspoof2021_air_amd import ops


def t(fn, reps=200):
    """Mean per call in us, python call + launch included, back to back on one stream."""
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def kernels():
    rows = []
    for B in (64, 128):
        x = 0.1 * torch.randn(B, 256, device="cuda")
        c = torch.randn(1, 256, device="cuda")
        w = torch.rand(256, 2, device="cuda") * 2 - 1
        cs = torch.randn(2, 256, device="cuda")
        lab = (torch.arange(B, device="cuda") % 2).long()
        logits = torch.randn(B, 2, device="cuda")
        probs = ops.softmax_rows(logits)
        from asvspoof2021_air_amd import _hip
        d = torch.empty_like(probs)

        def ce_bwd():
            _hip.check(_hip.lib().air_softmax_ce_bwd(_hip.dptr(probs), _hip.dptr(lab, torch.int64), _hip.ci(B), _hip.ci(2),
                                                     _hip.dptr(None, allow_none=True), _hip.dptr(d), _hip.stream()), "ce")
        r = {"B": B,
             "ocsoftmax": (t(lambda: ops.ocsoftmax_fwd(x, c, lab, 0.9, 0.2, 20.0)),
                           t(lambda: ops.ocsoftmax_bwd(x, c, lab, 0.9, 0.2, 20.0))),
             "ce": (t(lambda: ops.softmax_rows(logits)), t(ce_bwd)),
             "p2sgrad": (t(lambda: ops.p2sgrad_fwd(x, w, lab, 0.0)), t(lambda: ops.p2sgrad_bwd(x, w, lab, 0.0))),
             "isolate": (t(lambda: ops.isolate_fwd(x, c, lab, 0.9, 0.2, False)),
                         t(lambda: ops.isolate_bwd(x, c, lab, 0.9, 0.2, False))),
             "iso_sq": (t(lambda: ops.isolate_fwd(x, c, lab, 0.9, 0.2, True)),
                        t(lambda: ops.isolate_bwd(x, c, lab, 0.9, 0.2, True))),
             "amsoftmax": (t(lambda: ops.amsoftmax_fwd(x, cs, lab, 20.0, 0.9)), None)}
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def steps(n=30, warm=5):
    from asvspoof2021_air_amd.lcnn import LCNN
    from asvspoof2021_air_amd.resnet import ResNet
    from asvspoof2021_air_amd.train import Trainer
    from oracle.filler import synth_pcm
    B = 64
    pcm = synth_pcm(B, 64000, seed=1).cuda()
    labels = (torch.arange(B) % 2).long().cuda()
    out = []
    for model in ("resnet", "lcnn"):
        for head in ("ang_iso", None, "isolate", "iso_sq", "p2sgrad"):
            torch.manual_seed(0)
            m = ResNet(3, 256, resnet_type="18", nclasses=2) if model == "resnet" else LCNN(60, 256, nclasses=2)
            tr = Trainer(m.cuda(), add_loss=head, feat_len=750).enable_graph(True)
            for _ in range(warm):
                tr.step(pcm, labels)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                tr.step(pcm, labels)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / n * 1e3
            assert tr._graph is not None
            r = {"model": model, "head": str(head), "B": B, "step_ms": round(ms, 3), "utt_per_s": round(B / ms * 1e3, 1)}
            out.append(r)
            print(json.dumps(r), flush=True)
            del tr, m
            torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", action="store_true", help="also time the graphed train steps")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"kernels_us_fwd_bwd": kernels()}
    if a.steps:
        res["steps"] = steps()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
