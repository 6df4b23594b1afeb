"""GPU: SE-Res2Net-50's data-parallel train step with TWO ranks (one process each, both on cuda:0, gloo transport), on the
pattern of tests/test_dist_gpu.py: Trainer.step_features -> Res2Net backward with the gradient all-reduce launched from
inside it (dist.GradBucketer, cut where schedule.BackwardSchedule.grads_final_from reports a part of the arena final)
-> optimiser with grad_scale 1/world.  dist.py is used unchanged."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle.filler import fill_module_, synth_feat

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _make():
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.res2net import Res2Net, SEBottle2neck
    from asvspoof2021_air_amd.train import Trainer
    m = fill_module_(Res2Net(SEBottle2neck, [3, 4, 6, 3], baseWidth=26, scale=4, pretrained=False, num_classes=2))
    lossm = fill_module_(AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0))
    return Trainer(m, loss_module=lossm, feat_len=300)


def _shard(rank):
    x = synth_feat((4, 1, 60, 300), seed=150 + rank)
    labels = torch.tensor([0, 1, 1, 0]) if rank == 0 else torch.tensor([1, 1, 0, 1])
    return x, labels


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from asvspoof2021_air_amd import dist as air_dist
    torch.cuda.set_device(0)
    air_dist.init_from_env("gloo")
    tr = _make()
    assert tr.world == world and tr.model._bucketer is not None  # Trainer turned the in-backward all-reduce on
    x, labels = _shard(rank)
    loss, _ = tr.step_features(x.cuda(), labels.cuda())
    torch.cuda.synchronize()
    out[rank] = (loss.item(), tr.model.arena().flat.detach().cpu().numpy(), tr.loss.center.detach().cpu().numpy(),
                 tr.model._bucketer.total_launched)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_rank_res2net_step_equals_averaged_gradients():
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    (l0, w0, c0, nb0), (l1, w1, c1, nb1) = out[0], out[1]
    assert np.array_equal(w0, w1) and np.array_equal(c0, c1)  # ranks stay in lock-step, bit for bit
    assert nb0 == nb1 and nb0 >= 3, (nb0, nb1)  # buckets of layer4 .. layer1 left inside backward
    # single process: per-shard gradients, averaged by hand, one optimiser step
    grads, cgrads, losses = [], [], []
    for r in range(world):
        tr = _make()
        x, labels = _shard(r)
        tr.model.train()
        feats, _ = tr.model(x.cuda())
        loss, _ = tr.loss(feats, labels.cuda())
        loss.backward()
        grads.append(tr.model.arena().grad.clone())
        cgrads.append(tr.loss.center.grad.clone())
        losses.append(loss.item())
    np.testing.assert_allclose([l0, l1], losses, rtol=1e-6)
    tr = _make()
    arena = tr.model.arena()
    for n_, p, _, _ in arena.entries:  # gradients = views of the arena, as backward leaves them
        p.grad = None if n_ in ("cls_layer.weight", "cls_layer.bias") else arena.grad_view(n_)
    arena.grad.copy_(grads[0] + grads[1])
    arena.tail_has_grad = False
    tr.loss.center.grad = cgrads[0] + cgrads[1]
    tr.feat_optimizer.step(grad_scale=0.5)
    tr.loss_optimizer.step(grad_scale=0.5)
    n = arena.head_total
    np.testing.assert_array_equal(arena.flat[:n].cpu().numpy(), w0[:n])
    np.testing.assert_array_equal(tr.loss.center.detach().cpu().numpy(), c0)
