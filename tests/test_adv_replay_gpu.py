"""GPU: the --ADV_AUG step on the fused classifier heads (AdversarialTrainer(fused_heads=True)) against the oracle,
and its hipGraph replay (two captured phases) against the same steps launched eagerly, bit for bit."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle.filler import fill_module_, synth_pcm

pytestmark = pytest.mark.gpu

HEADS = (6, 3)


# ---------------------------------------------------------------------------------------------- fused step vs oracle
@pytest.mark.parametrize("path", ["strict", "default"])
def test_fused_step_gradients_against_the_oracle(path):
    """The objective and the bounds of tests/test_adversarial.py::_adversarial_step, on the fused heads."""
    from _budget import conv_path
    with conv_path(path):
        _fused_step(path)


def _fused_step(path):
    from _budget import tol
    from asvspoof2021_air_amd.adversarial import AdversarialTrainer
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.resnet import ResNet
    from oracle import adversarial as o_adv
    from oracle import resnet as o_resnet
    from oracle.filler import fill_state, fill_value, synth_feat
    from oracle.loss import ocsoftmax_forward
    B, T, NC, LAM = 8, 96, 5, 1.0
    x = synth_feat((B, 1, 60, T), seed=31)
    labels = torch.tensor([0, 1, 1, 0, 1, 1, 0, 1])
    channels = torch.tensor([0, 3, 1, 4, 2, 2, 0, 3])

    def make(fused):
        m = ResNet(3, 256, resnet_type="18", nclasses=2)
        fill_module_(m)
        m.set_attention_noise(None)
        lossm = AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)
        fill_module_(lossm)
        tr = AdversarialTrainer(m, NC, lambda_=LAM, recompute=True, fused_heads=fused, loss_module=lossm, feat_len=T)
        fill_module_(tr.classifiers[0])
        tr.classifiers[0].classifier[1].p = 0.0  # no dropout: comparable with the oracle
        return tr

    tr = make(True)
    w_before = tr.classifiers[0].classifier[0].weight.detach().clone()
    tr.step_features(x.cuda(), labels.cuda(), channels.cuda(), epoch_num=1)
    g_conv1 = tr.model.conv1.weight.grad.detach().cpu().numpy()
    g_fc = tr.model.fc.weight.grad.detach().cpu().numpy()
    assert int(tr.model.bn1.num_batches_tracked) == 2
    assert not torch.equal(w_before, tr.classifiers[0].classifier[0].weight.detach())
    sd = fill_state(o_resnet.resnet18_shapes())
    names = [k for k, v in sd.items() if v.dtype.is_floating_point and not o_resnet.is_buffer(k)]
    for k in names:
        sd[k] = sd[k].clone().requires_grad_(True)
    feat, _ = o_resnet.resnet18_forward(sd, x, True, None, {})
    l_oc, _ = ocsoftmax_forward(feat, fill_value("center", (1, 256)), labels, 0.9, 0.2, 20.0)
    cp = fill_state(o_adv.classifier_shapes(256, NC))
    l_adv = o_adv.cross_entropy(o_adv.classifier_forward(cp, feat, LAM, None), channels)
    g_oc = torch.autograd.grad(l_oc, [sd["conv1.weight"], sd["fc.weight"]], retain_graph=True)
    (l_oc + l_adv).backward()
    for got, k, plain in ((g_conv1, "conv1.weight", g_oc[0]), (g_fc, "fc.weight", g_oc[1])):
        ref = sd[k].grad.numpy()
        err = np.abs(got - ref).max() / np.abs(ref).max()
        gap = np.abs(plain.numpy() - ref).max() / np.abs(ref).max()  # what dropping the adversarial term would cost
        print("fused adv %s [%s]: rel max err %.3g, bound %.3g, gap %.3g" % (k, path, err, tol("adv_rel_max", path), gap))
        assert err <= tol("adv_rel_max", path) and gap > 20 * err, (path, k, err, gap)
    np.testing.assert_allclose(float(tr.last["adv_loss"]), l_adv.item(), rtol=1e-4)
    # the accuracy counts: those of the module path on the same weights
    ref = make(False)
    ref.step_features(x.cuda(), labels.cuda(), channels.cuda(), epoch_num=1)
    for key in ("correct_m", "correct_c"):
        got = tr.last[key]
        assert got.dtype == torch.int32 and got.dim() == 0 and got.is_cuda
        assert int(got) == int(ref.last[key]), key
    assert tr.epoch_accuracy() == ref.epoch_accuracy() == (100.0 * int(tr.last["correct_m"]) / B,
                                                          100.0 * int(tr.last["correct_c"]) / B)


# ---------------------------------------------------------------------------------------------- replay equals eager
def _model(kind, seed=4242):
    if kind == "ecapa":
        from asvspoof2021_air_amd.ecapa_tdnn import Bottle2neck, Res2Net2
        m = Res2Net2(Bottle2neck, C=512, model_scale=8, nOut=2, n_mels=60)
        fill_module_(m)
        return m.cuda().set_compute_dtype("bf16")
    from asvspoof2021_air_amd.resnet import ResNet
    m = ResNet(3, 256, resnet_type="18", nclasses=2)
    fill_module_(m)
    m = m.cuda()
    m._noise_seed = seed  # device-side attention noise: replays draw afresh
    return m


def _trainer(kind, graph, recompute=True, heads=HEADS, cls=None, seed=4242, **kw):
    from asvspoof2021_air_amd.adversarial import AdversarialTrainer
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.train import Trainer
    lossm = AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)
    fill_module_(lossm)
    common = dict(loss_module=lossm, feat_len=128 if kind == "ecapa" else 96, ecapa=(kind == "ecapa"), **kw)
    if cls is Trainer:
        return Trainer(_model(kind, seed), **common)
    tr = AdversarialTrainer(_model(kind, seed), heads, recompute=recompute, fused_heads=True, **common)
    for k, c in enumerate(tr.classifiers):
        fill_module_(c)
        c._seed = 1000 + k
    if graph:
        tr.enable_graph()
    return tr


def _batch(i, B=8, L=16000):
    pcm = synth_pcm(B, L, seed=300 + i).cuda()
    labels = ((torch.arange(B) + i) % 3 != 0).long().cuda()
    channels = torch.stack([(torch.arange(B) * 5 + i) % HEADS[0], (torch.arange(B) + 2 * i) % HEADS[1]], 1).cuda()
    return pcm, labels, channels


def _bn(model):
    return model.bn1


def _state(tr):
    """Everything a step leaves behind, as tensors / numbers to compare bit for bit."""
    torch.cuda.synchronize()
    out = [tr.model.arena().flat.clone(), tr.loss.center.detach().clone(), _bn(tr.model).running_var.clone(),
           torch.tensor(int(_bn(tr.model).num_batches_tracked))]
    for c, opt in zip(tr.classifiers, tr.classifier_optimizers):
        out += [c.flatten().clone(), opt.flat_state[0].clone(), opt.flat_state[1].clone(),
                c.counter(c.flatten().device).clone()]
    out.append(torch.tensor(tr.epoch_accuracy()))
    return out


def _last(tr):
    last = tr.last
    return [None if last["adv_loss"] is None else float(last["adv_loss"])] + [float(l) for l in last["classifier_loss"]] + [
        int(last["correct_m"]), int(last["correct_c"])]


def _same(a, b):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), "entry %d differs" % i


@pytest.mark.parametrize("recompute", [True, False])
@pytest.mark.parametrize("kind", ["ecapa", "resnet"])
def test_replay_equals_eager(kind, recompute):
    batches = [_batch(i) for i in range(8)]
    ends = []
    for graph in (False, True):
        tr = _trainer(kind, graph, recompute)
        losses, lasts, captures = [], [], []
        for i, (pcm, lab, ch) in enumerate(batches):
            if i == 6:
                tr.set_epoch(4, lr_decay=0.5, interval=4)
            losses.append(tr.step(pcm, lab, channels=ch, epoch_num=0 if i < 4 else 1)[0].item())
            lasts.append(_last(tr))
            if tr._graph is not None and not any(tr._graph is g for g in captures):
                captures.append(tr._graph)
        assert (tr._graph is not None) == graph
        if graph:  # each phase of both keys (without and with the adversarial term) was captured
            assert len(captures) == 2 and all(g["tail"] is not None for g in captures)
            assert [("adv" in g["key"]) for g in captures] == [True, True] and captures[0]["key"] != captures[1]["key"]
        assert int(_bn(tr.model).num_batches_tracked) == (16 if recompute else 8)
        assert lasts[3][0] is None and lasts[4][0] is not None
        ends.append((losses, lasts, _state(tr)))
    (l0, a0, s0), (l1, a1, s1) = ends
    assert all(np.isfinite(l0)) and l0 == l1 and a0 == a1
    _same(s0, s1)
    for c in range(len(HEADS)):  # dropout was live: two draws per step once the adversarial term is on
        assert int(s0[4 + 4 * c + 3]) == (4 + 2 * 4) * ((8 * 128 + 3) // 4)


def test_replays_interleaved_with_eager_steps():
    """The sequence of test_graphed_steps_interleaved_with_eager with adversarial steps; the steps without channels
    are a plain Trainer's."""
    from asvspoof2021_air_amd.train import Trainer
    batches = [_batch(400 + i) for i in range(12)]
    big = _batch(77, B=24)
    ends = []
    for graph in (False, True):
        tr = _trainer("ecapa", graph)
        plain = []
        losses = []
        for i, (pcm, lab, ch) in enumerate(batches):
            if i == 3:    # a plain eager adversarial step on the same trainer
                out = tr.step_features(tr.features(pcm), lab, ch, 1)
            elif i == 5:  # external zero_grad on all optimisers + a scoring pass in between
                for opt in [tr.feat_optimizer, tr.loss_optimizer] + tr.classifier_optimizers:
                    opt.zero_grad()
                tr.score(pcm)
                out = tr.step(pcm, lab, channels=ch)
            elif i == 6:  # a larger eager batch outgrows the scratch buffers the graph points into
                out = tr.step_features(tr.features(big[0]), big[1], big[2], 1)
            elif i == 8:  # a step without channels: Trainer's path
                ref = _trainer("ecapa", False, cls=Trainer)
                ref.model.arena().flat.copy_(tr.model.arena().flat)
                for a, b in zip(ref.model.buffers(), tr.model.buffers()):
                    a.copy_(b)
                ref.loss.center.data.copy_(tr.loss.center.data)
                want = ref.step(pcm, lab)
                out = tr.step(pcm, lab, channels=None)
                # (Adam's moments differ - the reference trainer is new - so the comparison is the step's own output
                # and gradients)
                assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
                assert torch.equal(tr.model.arena().grad, ref.model.arena().grad)
                plain.append(out[0].item())
            else:
                out = tr.step(pcm, lab, channels=ch)
            losses.append(out[0].item())
        if graph:
            assert tr._graph is not None and tr.model.training
        ends.append((losses, _last(tr), _state(tr)))
    (l0, a0, s0), (l1, a1, s1) = ends
    assert all(np.isfinite(l0)) and l0 == l1 and a0 == a1
    _same(s0, s1)


def test_ragged_batches_with_the_augment_chain():
    from asvspoof2021_air_amd.augment import AugmentChain, ChannelAugment, CodecAugment
    B, cap, lengths = 4, 16000, [16000, 9000, 4000, 1]
    ends = []
    for graph in (False, True):
        chain = AugmentChain(CodecAugment(p=0.7, seed=11), ChannelAugment(p=0.7, seed=12))
        n_codec, n_chan = 3, int(chain.stages[1].irs.shape[0]) + 1
        tr = _trainer("resnet", graph, heads=(n_codec, n_chan), augment=chain)
        losses = []
        for i in range(5):
            pcm = (synth_pcm(B, cap, seed=600 + i) * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
            for b, n in enumerate(lengths):
                pcm[b, n:] = 0
            lab = ((torch.arange(B) + i) % 3 != 0).long().cuda()
            channels = chain.prepare(B)
            assert int(channels[:, 0].max()) < n_codec and int(channels[:, 1].max()) < n_chan
            ln = torch.tensor(lengths[i % 4:] + lengths[:i % 4], dtype=torch.int32).cuda()
            losses.append(tr.step(pcm.cuda(), lab, channels=channels, lengths=ln)[0].item())
        assert (tr._graph is not None) == graph
        ends.append((losses, _last(tr), _state(tr)))
    (l0, a0, s0), (l1, a1, s1) = ends
    assert all(np.isfinite(l0)) and l0 == l1 and a0 == a1
    _same(s0, s1)


# ---------------------------------------------------------------------------------------------- two ranks, one GPU
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out, graph):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from asvspoof2021_air_amd import dist as air_dist
    torch.cuda.set_device(0)
    air_dist.init_from_env("gloo")
    tr = _trainer("resnet", False, seed=77 + rank)
    if graph:
        tr.segment_bytes = 8 << 20
        tr.enable_graph()
    losses = []
    for i in range(4):
        pcm, lab, ch = _batch(900 + 10 * i + rank, B=4)
        losses.append(tr.step(pcm, lab, channels=ch)[0].item())
    torch.cuda.synchronize()
    assert tr.world == world and (tr._graph is not None) == graph
    if graph:
        assert len(tr._graph["segments"]) >= 3 and tr._graph["tail"] is not None
    out[rank] = (losses, _last(tr), [t.cpu().numpy() for t in _state(tr)])
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_replay_equals_two_ranks_eager():
    world = 2
    mgr = mp.Manager()
    ends = []
    for graph in (False, True):
        out = mgr.dict()
        mp.spawn(_worker, args=(world, _free_port(), out, graph), nprocs=world, join=True)
        ends.append((out[0], out[1]))
        # the classifiers are replicas: parameters (and moments) agree across the ranks
        s0, s1 = out[0][2], out[1][2]
        for c in range(len(HEADS)):
            for j in range(3):
                np.testing.assert_array_equal(s0[4 + 4 * c + j], s1[4 + 4 * c + j])
        np.testing.assert_array_equal(s0[0], s1[0])
    for rank in range(world):
        (le, ae, se), (lg, ag, sg) = ends[0][rank], ends[1][rank]
        assert le == lg and ae == ag
        for u, v in zip(se, sg):
            np.testing.assert_array_equal(u, v)
