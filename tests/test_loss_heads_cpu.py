"""CPU: the loss heads of loss.py (P2SGradLoss, IsolateLoss, IsolateSquareLoss, AMSoftmax): the fp64 restatement
(tests/loss_heads_oracle.py) against the golden from the real reference, seeded construction and state_dict keys
equal to the reference's, and no CPU fallback."""
import numpy as np
import pytest
import torch

import loss_heads_oracle as o

SEED_INIT = 1303


@pytest.fixture(scope="module")
def gold(golden):
    return golden("heads.npz")


def _d(t):
    return t.detach().double()


@pytest.mark.parametrize("case", ["mixed", "bona"])
def test_oracle_matches_reference_golden(gold, case):
    B = int(gold["cfg"][0])
    x, labels = o.inputs(B)
    if case == "bona":
        labels = torch.zeros(B, dtype=torch.int64)
    P = o.params()
    for smooth in (0.0, 0.1):
        (lo, neg), (dx, dw) = o.grads(lambda a, w: o.p2sgrad(a, w, labels, smooth), _d(x), _d(P["p2s"]))
        tag = "p2s%g_%s" % (smooth, case)
        np.testing.assert_allclose(lo.item(), gold[tag + "_loss"], rtol=1e-5)
        np.testing.assert_allclose(neg.detach().numpy(), gold[tag + "_neg"], atol=1e-6)
        np.testing.assert_allclose(dx.numpy(), gold[tag + "_dx"], atol=1e-7 * 100, rtol=1e-4)
        np.testing.assert_allclose(dw.numpy(), gold[tag + "_dw"], atol=1e-6, rtol=1e-4)
    for sq in (False, True):
        tag = "%s_%s" % ("isosq" if sq else "iso", case)
        lo, (dx, dc) = o.grads(lambda a, c: o.isolate(a, c, labels, square=sq), _d(x), _d(P["iso"]))
        if case == "bona":  # torch's mean of an empty tensor: NaN; the bona fide class's gradient stays finite
            assert np.isnan(gold[tag + "_loss"]) and torch.isnan(lo)
            assert np.isfinite(gold[tag + "_dx"]).all() and torch.isfinite(dx).all()
        else:
            np.testing.assert_allclose(lo.item(), gold[tag + "_loss"], rtol=1e-5)
        np.testing.assert_allclose(dx.numpy(), gold[tag + "_dx"], atol=1e-6, rtol=1e-4)
        np.testing.assert_allclose(dc.numpy(), gold[tag + "_dc"], atol=1e-6, rtol=1e-4)
    lg, mg = o.amsoftmax(_d(x), _d(P["ams"]), labels)
    np.testing.assert_allclose(lg.numpy(), gold["ams_%s_logits" % case], atol=1e-6)
    np.testing.assert_allclose(mg.numpy(), gold["ams_%s_margin" % case], atol=2e-5)


def test_seeded_construction_and_state_dict_keys_equal_the_reference(gold):
    from asvspoof2021_air_amd.loss import AMSoftmax, IsolateLoss, IsolateSquareLoss, P2SGradLoss
    ctors = {"p2s": lambda: P2SGradLoss(256, 2, smooth=0.0), "iso": lambda: IsolateLoss(2, 256),
             "iso_sq": lambda: IsolateSquareLoss(2, 256), "ams": lambda: AMSoftmax(2, 256)}
    for name, ctor in ctors.items():
        torch.manual_seed(SEED_INIT)
        m = ctor()
        sd = m.state_dict()
        assert list(sd.keys()) == list(gold[name + "_keys"]), name
        v = next(iter(sd.values())).double()
        np.testing.assert_allclose([float(v.sum()), float(v.abs().sum()), float((v * v).sum())], gold[name + "_init"],
                                   rtol=1e-6, err_msg=name)
    # constructor defaults and attribute names of the reference
    p = P2SGradLoss(256, 2)
    assert (p.in_dim, p.out_dim, p.smooth, tuple(p.weight.shape)) == (256, 2, 0.1, (256, 2))
    i = IsolateLoss()
    assert (i.num_classes, i.feat_dim, i.r_real, i.r_fake, tuple(i.center.shape)) == (10, 2, 0.042, 1.638, (1, 2))
    a = AMSoftmax(2, 256)
    assert (a.num_classes, a.enc_dim, a.s, a.m, tuple(a.centers.shape)) == (2, 256, 20, 0.9, (2, 256))


def test_whole_module_pickles_round_trip(tmp_path):
    from asvspoof2021_air_amd.loss import IsolateLoss, P2SGradLoss
    for m in (P2SGradLoss(256, 2, smooth=0.0), IsolateLoss(2, 256, r_real=0.9, r_fake=0.2)):
        path = str(tmp_path / "m.pt")
        torch.save(m, path)
        back = torch.load(path, weights_only=False)
        assert type(back) is type(m)
        for (k, v), (k2, v2) in zip(m.state_dict().items(), back.state_dict().items()):
            assert k == k2 and torch.equal(v, v2)


def test_cpu_tensors_raise_air_error():
    from asvspoof2021_air_amd._hip import AirError
    from asvspoof2021_air_amd.loss import AMSoftmax, CrossEntropyLoss, IsolateLoss, IsolateSquareLoss, P2SGradLoss
    x, labels = o.inputs(4)
    for m in (P2SGradLoss(256, 2), IsolateLoss(2, 256), IsolateSquareLoss(2, 256)):
        with pytest.raises(AirError):
            m(x, labels)
    with pytest.raises(AirError), torch.no_grad():
        AMSoftmax(2, 256)(x, labels)
    with pytest.raises(AirError):
        CrossEntropyLoss()(torch.zeros(4, 2), labels)


def test_trainer_rejects_unknown_heads():
    from asvspoof2021_air_amd.train import ADD_LOSSES, Trainer
    assert ADD_LOSSES == (None, "isolate", "iso_sq", "ang_iso", "p2sgrad")
    with pytest.raises(ValueError):
        Trainer(torch.nn.Linear(2, 2), add_loss="amsoftmax")
