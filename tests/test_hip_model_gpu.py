"""GPU: the two ways into a hip_model.HipModel - ``model(x)`` + ``backward()`` through the one autograd Function, and
``forward_saved`` + ``backward_saved`` (train.Trainer's capture) - launch the same kernels in the same order, so every
entry of the gradient arena is the same to the bit.  Each model at the smallest shape its own gradient test uses."""
import pytest
import torch

from oracle.filler import fill_module_, synth_feat

pytestmark = pytest.mark.gpu


def _resnet():
    from asvspoof2021_air_amd.resnet import ResNet
    m = fill_module_(ResNet(3, 256, resnet_type="18", nclasses=2))
    m.set_attention_noise(1e-5 * synth_feat((2, 12, 256), seed=5))  # both passes see the same draw
    return m


def _ecapa():
    from asvspoof2021_air_amd.ecapa_tdnn import Bottle2neck, Res2Net2
    return fill_module_(Res2Net2(Bottle2neck, C=512, model_scale=8, nOut=2, n_mels=60))


def _lcnn():
    from asvspoof2021_air_amd.lcnn import LCNN
    m = fill_module_(LCNN(60, 256))
    keep = (torch.rand(2, 4416, generator=torch.Generator().manual_seed(52)) >= 0.7).float() / 0.3
    m.set_dropout_mask(keep)
    return m


def _res2net():
    from asvspoof2021_air_amd.res2net import Res2Net, SEBottle2neck
    return fill_module_(Res2Net(SEBottle2neck, [3, 4, 6, 3], baseWidth=26, scale=4, pretrained=False,
                                num_classes=2))


BUILD = {"resnet": (_resnet, (2, 1, 60, 96)), "ecapa": (_ecapa, (2, 60, 96)), "lcnn": (_lcnn, (2, 1, 60, 750)),
         "res2net": (_res2net, (2, 1, 60, 401))}


def _grads(build, saved_path, x, gf, go):
    """Gradients of every arena entry from a fresh model in train mode (clones, None where there is none), feat."""
    m = build().cuda().train()
    if saved_path:
        feat, saved = m.forward_saved(x)
        grads = m.backward_saved(saved, gf, dout=go)
    else:
        feat, out = m(x)
        torch.autograd.backward([feat] + ([out] if go is not None else []), [gf] + ([go] if go is not None else []))
        grads = [p.grad for _, p, _, _ in m.arena().entries]
    torch.cuda.synchronize()
    arena = m.arena()
    names = [n for n, _, _, _ in arena.entries]
    tail = [n for n, _, o, _ in arena.entries if o >= arena.head_total]
    return names, [None if g is None else g.detach().clone() for g in grads], feat.detach().clone(), tail


@pytest.mark.parametrize("name", sorted(BUILD))
def test_autograd_and_saved_paths_bit_equal(name):
    build, shape = BUILD[name]
    x = synth_feat(shape, seed=71).cuda()
    gf, go_full = synth_feat((2, 256), seed=72).cuda(), synth_feat((2, 2), seed=73).cuda()
    for go in (go_full, None):  # with the CE branch through the tail layer, and without it (ang_iso)
        names, ga, fa, tail = _grads(build, False, x, gf, go)
        names_s, gs, fs, _ = _grads(build, True, x, gf, go)
        assert names == names_s and torch.equal(fa, fs)
        for n, a, s in zip(names, ga, gs):
            assert (a is None) == (s is None), n
            assert (a is None) == (go is None and n in tail), n  # every entry but a dead tail has a gradient
            if a is not None:
                assert torch.equal(a, s), "%s: %.3g" % (n, (a - s).abs().max().item())
