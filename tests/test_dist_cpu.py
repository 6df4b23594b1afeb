"""CPU, world_size 2, gloo: the data-parallel gradient exchange (asvspoof2021_air_amd/dist.py)
over flat arenas, and the arena layout itself."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as td
import torch.multiprocessing as mp
import torch.nn as nn

from asvspoof2021_air_amd import dist as air_dist
from asvspoof2021_air_amd.hip_model import HipModel


def test_bucket_slices_cover_reverse_order():
    n = 12_450_546
    sl = air_dist.bucket_slices(n, 16 << 20)
    assert sl[0][1] == n and sl[-1][0] == 0
    assert all(a[0] == b[1] for a, b in zip(sl, sl[1:]))  # contiguous, last layers first
    assert max(e - s for s, e in sl) <= (16 << 20) // 4
    assert air_dist.bucket_slices(10, 16) == [(6, 10), (2, 6), (0, 2)]


class Toy(HipModel):
    TAIL = ("tail.weight", "tail.bias")

    def __init__(self):
        super().__init__()
        self.a = nn.Linear(7, 5)
        self.tail = nn.Linear(5, 2)


def test_arena_views_and_tail():
    m = Toy()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    ar = m.arena()
    assert ar.bound()
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k])  # values preserved
    # every view 16-byte aligned, tail last
    offs = {n: o for n, _, o, _ in ar.entries}
    assert all(o % 4 == 0 for o in offs.values())
    assert offs["tail.weight"] >= ar.head_total and offs["a.bias"] < ar.head_total
    m.a.weight.data.add_(1.0)  # writing a parameter writes the arena
    o = offs["a.weight"]
    assert torch.equal(ar.flat[o:o + 35].view(5, 7), m.a.weight.data)
    sd = m.state_dict()
    m2 = Toy()
    m2.arena()
    m2.load_state_dict(sd)  # in-place copy keeps the views bound
    assert m2.arena().bound() and torch.equal(m2.a.weight, m.a.weight)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    air_dist.init_from_env("gloo")
    assert air_dist.world_size() == world and air_dist.rank() == rank
    torch.manual_seed(0)
    m = Toy()
    ar = m.arena()
    # rank-dependent gradients; tail has none (like fc_mu under ang_iso)
    ar.grad.zero_()
    ar.grad[:ar.head_total] = float(rank + 1) * torch.arange(ar.head_total, dtype=torch.float32)
    ar.grad[ar.head_total:] = 123.0 + rank
    ar.tail_has_grad = False
    centre = nn.Parameter(torch.zeros(1, 8))
    centre.grad = torch.full((1, 8), float(rank + 1))
    holder = nn.Module()
    holder.center = centre
    air_dist.BUCKET_BYTES = 64  # force several buckets
    air_dist.allreduce_grads(m, holder)
    total = sum(range(1, world + 1))
    ok = torch.equal(ar.grad[:ar.head_total], total * torch.arange(ar.head_total, dtype=torch.float32))
    ok &= bool((ar.grad[ar.head_total:] == 123.0 + rank).all())  # tail untouched
    ok &= bool((centre.grad == total).all())
    # early stop under `if rank == 0: save_checkpoint(...)`: only rank 0's counter advanced, every rank must stop
    from asvspoof2021_air_amd.train import Trainer
    tr = Trainer.__new__(Trainer)
    tr.world, tr.device, tr.early_stop_cnt = world, torch.device("cpu"), (3 if rank == 0 else 0)
    ok &= tr.should_stop(patience=4) is False and tr.early_stop_cnt == 3
    tr.early_stop_cnt += 1 if rank == 0 else 0
    ok &= tr.should_stop(patience=4) is True
    # improve -> reset -> should_stop.  Rank 0 saw an improvement and reset; the other ranks still carry
    # the count they adopted (4).  The reference counts CONSECUTIVE epochs (main_train.py:705-711): everyone is at 0.
    if rank == 0:
        tr.early_stop_cnt = 0
    ok &= tr.should_stop(patience=4) is False and tr.early_stop_cnt == 0
    tr.early_stop_cnt += 1 if rank == 0 else 0
    ok &= tr.should_stop(patience=4) is False and tr.early_stop_cnt == 1
    out[rank] = bool(ok)
    td.barrier()
    td.destroy_process_group()


def test_allreduce_grads_gloo_world2():
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    assert dict(out) == {0: True, 1: True}


class Toy8(HipModel):
    """Several tensors of awkward sizes so that small buckets cut through the middle of them."""
    TAIL = ("tail.weight", "tail.bias")

    def __init__(self):
        super().__init__()
        self.a = nn.Linear(13, 11)
        self.b = nn.Linear(11, 9)
        self.c = nn.Linear(9, 7)
        self.tail = nn.Linear(7, 3)


def _worker8(rank, world, port, out, tail_has_grad):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    air_dist.init_from_env("gloo")
    torch.manual_seed(0)
    m = Toy8()
    ar = m.arena()
    n, h = ar.total, ar.head_total
    base = torch.arange(n, dtype=torch.float32)
    ar.grad.copy_((rank + 1) * base + rank)          # exact in fp32: the sums below are integers < 2^24
    ar.tail_has_grad = tail_has_grad
    centre = nn.Parameter(torch.zeros(1, 8))
    centre.grad = torch.full((1, 8), float(rank + 1))
    holder = nn.Module()
    holder.center = centre
    # 100-byte buckets = 25 floats: every tensor boundary (143, 11, 99, 9, 63, 7 floats, 16-byte padded) falls
    # inside some bucket, and the first bucket sent is shorter than the rest of the head
    air_dist.BUCKET_BYTES = 100
    slices = air_dist.bucket_slices(h, 100)
    offs = sorted(o for _, _, o, _ in ar.entries if 0 < o < h)
    assert any(s < o < e for o in offs for s, e in slices), "no bucket cuts through a tensor"
    # a GradBucketer that already sent the last 30 floats of the head from "inside backward"
    bk = air_dist.GradBucketer(bucket_bytes=100)
    m._bucketer = bk
    bk.reset(ar.grad, h)
    # CPU stand-in for flush(): same bookkeeping, no HIP stream
    lo = h - 30
    bk.lo = lo
    bk.works.append(td.all_reduce(ar.grad[lo:h], op=td.ReduceOp.SUM, async_op=True))
    bk.launched += 1
    bk.hi = lo
    air_dist.allreduce_grads(m, holder)
    ws = sum(r + 1 for r in range(world))
    wr = sum(range(world))
    want = ws * base + wr
    ok = torch.equal(ar.grad[:h], want[:h])
    if tail_has_grad:
        ok &= torch.equal(ar.grad[h:], want[h:])
    else:
        ok &= torch.equal(ar.grad[h:], ((rank + 1) * base + rank)[h:])  # untouched
    ok &= bool((centre.grad == ws).all())
    ok &= bk.grad is None  # reset for the next step
    mean = air_dist.all_mean(float(rank))
    ok &= abs(mean - (world - 1) / 2.0) < 1e-12
    out[rank] = bool(ok)
    td.barrier()
    td.destroy_process_group()


@pytest.mark.parametrize("tail_has_grad", [False, True])
def test_allreduce_grads_gloo_world8_mid_tensor_buckets(tail_has_grad):
    """World 8 (BASELINE configs[3]/[4] run 8 ranks): buckets that split tensors, a region already sent from
    inside backward, and the tail both with and without gradients (fc_mu.* gets one under the CE head)."""
    world = 8
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker8, args=(world, _free_port(), out, tail_has_grad), nprocs=world, join=True)
    assert dict(out) == {r: True for r in range(world)}
