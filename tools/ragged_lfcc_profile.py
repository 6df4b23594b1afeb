"""Ragged LFCC launch vs a fixed-length launch: the launches to trace with rocprofv3 --kernel-trace --stats.
B = 64, int16; ragged: Lcap = 13 s, lengths uniform in 1..13 s (seed 0); fixed: L = 64000; feat_len 750, repeat."""
import sys

import numpy as np
import torch

from asvspoof2021_air_amd.feature_extraction import LFCC

N = 50
FOUT = 28
B, cap, feat_len = 64, 13 * 16000, 750
rng = np.random.RandomState(0)
lengths = rng.randint(16000, cap + 1, size=B)
T = 1 + lengths // 160
start = np.array([rng.randint(t - feat_len) if t > feat_len else 0 for t in T], dtype=np.int32)
live = 0
for t, s in zip(T, start):
    for t0 in range(0, 1 + cap // 160, FOUT):
        if t0 >= t:
            continue
        if t > feat_len and (t0 + FOUT <= s or t0 >= s + feat_len):
            continue
        live += 1
tiles_cap = -(-(1 + cap // 160) // FOUT)
print("ragged: seconds %.2f mean, T mean %.1f, tiles launched %d, live %d (%.1f %%), frames written per live tile %d"
      % (lengths.mean() / 16000, T.mean(), B * tiles_cap, live, 100.0 * live / (B * tiles_cap), FOUT))
print("ragged: live output frames %d ; sum min(T, feat_len) %d ; sum T %d" % (live * FOUT, int(np.minimum(T, feat_len).sum()), int(T.sum())))
print("fixed : tiles %d, output frames %d" % (B * 15, B * 401))
g = torch.Generator().manual_seed(1)
x16 = torch.randint(-20000, 20000, (B, cap), generator=g, dtype=torch.int32).to(torch.int16).cuda()
xf = x16[:, :64000].contiguous()
m = LFCC(320, 160, 512, 16000, 20).cuda()
m.mutate_input = False
ld = torch.from_numpy(lengths.astype(np.int32)).cuda()
sd = torch.from_numpy(start).cuda()
for _ in range(3):
    a = m.forward_ragged(x16, ld, feat_len, sd, "repeat")
    b = m.forward_padded(xf, feat_len, None, "repeat")
torch.cuda.synchronize()
ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
ev[0].record()
for _ in range(N):
    a = m.forward_ragged(x16, ld, feat_len, sd, "repeat")
ev[1].record()
for _ in range(N):
    b = m.forward_padded(xf, feat_len, None, "repeat")
ev[2].record()
torch.cuda.synchronize()
print("events (back-to-back launches incl. output allocation): ragged %.1f us / launch, fixed %.1f us / launch"
      % (1e3 * ev[0].elapsed_time(ev[1]) / N, 1e3 * ev[1].elapsed_time(ev[2]) / N))
print("finite", bool(torch.isfinite(a).all()), bool(torch.isfinite(b).all()))
