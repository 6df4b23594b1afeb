"""GPU: data-parallel training under the CE and P2SGrad heads with TWO ranks (one process each, both on cuda:0, gloo
transport), on the pattern of tests/test_lcnn_dist_gpu.py: the step equals one optimiser step on the averaged
single-rank gradients - the arena tail (fc_mu, the CE head's) and the P2SGrad weight included - and under CE the
segmented hipGraph replay (a capture cut at backward's bucket boundaries, each bucket all-reduced between replays, the
tail behind the last) equals the eager bucketed step bit for bit."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle.filler import fill_module_, synth_feat, synth_pcm

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _make(head):
    from asvspoof2021_air_amd.lcnn import LCNN
    from asvspoof2021_air_amd.train import Trainer
    m = fill_module_(LCNN(60, 256))
    tr = Trainer(m, feat_len=750, add_loss=head)
    if tr.loss is not None:
        fill_module_(tr.loss)
    return tr


def _shard(rank):
    x = synth_feat((4, 1, 60, 750), seed=250 + rank)
    labels = torch.tensor([0, 1, 1, 0]) if rank == 0 else torch.tensor([1, 1, 0, 1])
    g = torch.Generator().manual_seed(260 + rank)
    keep = (torch.rand(4, 4416, generator=g) >= 0.7).float() / 0.3
    return x, labels, keep


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from asvspoof2021_air_amd import dist as air_dist
    torch.cuda.set_device(0)
    air_dist.init_from_env("gloo")


def _worker(rank, world, port, head, out):
    _init(rank, world, port)
    tr = _make(head)
    x, labels, keep = _shard(rank)
    tr.model.set_dropout_mask(keep)
    loss, _ = tr.step_features(x.cuda(), labels.cuda())
    torch.cuda.synchronize()
    hp = [p.detach().cpu().numpy() for p in tr._loss_params()]
    out[rank] = (loss.item(), tr.model.arena().flat.detach().cpu().numpy(), hp)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("head", [None, "p2sgrad"])
def test_two_rank_step_equals_averaged_gradients(head):
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), head, out), nprocs=world, join=True)
    (l0, w0, h0), (l1, w1, h1) = out[0], out[1]
    assert np.array_equal(w0, w1) and all(np.array_equal(a, b) for a, b in zip(h0, h1))
    grads, hgrads, losses, tails = [], [], [], []
    for r in range(world):
        tr = _make(head)
        x, labels, keep = _shard(r)
        tr.model.set_dropout_mask(keep)
        tr.model.train()
        loss, _ = tr.step_features(x.cuda(), labels.cuda())  # world 1: the gradients stay in the arena / p.grad
        grads.append(tr.model.arena().grad.clone())
        tails.append(tr.model.arena().tail_has_grad)
        hgrads.append([p.grad.clone() for p in tr._loss_params()])
        losses.append(loss.item())
    assert tails == [head is None] * 2
    np.testing.assert_allclose([l0, l1], losses, rtol=1e-6)
    tr = _make(head)
    arena = tr.model.arena()
    for n_, p, _, _ in arena.entries:
        p.grad = None if (head is not None and n_.startswith("fc_mu")) else arena.grad_view(n_)
    arena.grad.copy_(grads[0] + grads[1])
    arena.tail_has_grad = head is None
    for p, g0, g1 in zip(tr._loss_params(), *hgrads) if hgrads[0] else ():
        p.grad = g0 + g1
    tr._optimise(0.5)
    np.testing.assert_array_equal(arena.flat.cpu().numpy(), w0)
    for p, want in zip(tr._loss_params(), h0):
        np.testing.assert_array_equal(p.detach().cpu().numpy(), want)


def _seg_worker(rank, world, port, out):
    _init(rank, world, port)
    te, tg = _make(None), _make(None)
    te.model._mask_seed = tg.model._mask_seed = 4321 + rank
    tg.segment_bytes = 256 << 10  # cut the LCNN's 4 MB arena into several segments
    tg.enable_graph(True)
    assert tg.graph_segments
    res = []
    for i in range(5):
        pcm = synth_pcm(4, 16000, seed=500 + 10 * rank + i).cuda()
        labels = torch.tensor([0, 1, 1, 0] if (rank + i) % 2 else [1, 0, 1, 1]).cuda()
        le, _ = te.step(pcm, labels)
        lg, _ = tg.step(pcm, labels)
        torch.cuda.synchronize()
        res.append((torch.equal(le, lg), torch.equal(te.model.arena().flat, tg.model.arena().flat)))
    g = tg._graph
    out[rank] = (res, g is not None and len(g["graphs"]) > 1, tg._seg_bucketer is not None and
                 tg._seg_bucketer.total_launched > 0, tg.model.arena().tail_has_grad)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_rank_segmented_replay_equals_eager_under_ce():
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_seg_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    for r in range(world):
        res, segmented, sent, tail = out[r]
        assert segmented and sent and tail, (r, segmented, sent, tail)
        assert all(a and b for a, b in res), (r, res)
