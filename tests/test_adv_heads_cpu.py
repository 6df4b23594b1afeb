"""CPU: the fused classifier heads' C-ABI entry (air_adv_heads) is declared and exported and refuses what it does not
support ahead of any HIP call; the AdversarialTrainer surface; the flat classifier storage survives a pickle."""
import ctypes
import inspect
import io
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from asvspoof2021_air_amd import _hip, build
    build.build(verbose=False)
    return _hip.lib()


def test_declared_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "air_hip.h")).read()
    assert re.search(r"\bint\s+air_adv_heads\s*\(\s*const\s+AirAdvHeads\s*\*\s*d\s*,\s*air_stream_t\s+stream\s*\)", text)
    assert hasattr(lib, "air_adv_heads") and hasattr(lib, "air_adv_heads_ws_bytes")


def descriptor(B=8, D=16, classes=(3,), want_dx=1, ws_bytes=1 << 20):
    """A well-formed descriptor whose pointers are never followed: every call below is refused on the host."""
    from asvspoof2021_air_amd import _hip
    d = _hip.AirAdvHeads()
    d.B, d.D, d.nheads, d.want_dx, d.lambda_ = B, D, len(classes), want_dx, 0.05
    d.feats, d.dx, d.ws, d.ws_bytes = 0x1000, 0x2000, 0x3000, ws_bytes
    for k, C in enumerate(classes[:_hip.ADV_MAX_HEADS]):
        h = d.head[k]
        h.w1, h.b1, h.w2, h.b2, h.targets = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
        h.grads, h.loss, h.correct = 0x60000, 0x70000, 0x80000
        h.counter = 0x90000 + 8 * k
        h.C, h.p = C, 0.3
    return d


def refused(lib, d):
    return lib.air_adv_heads(ctypes.byref(d), ctypes.c_void_p(0)) == EINVAL


def test_refusals_need_no_device(lib):
    assert lib.air_adv_heads(None, ctypes.c_void_p(0)) == EINVAL
    for kw in (dict(B=0), dict(B=4097), dict(D=0), dict(D=7), dict(D=1026), dict(classes=()), dict(classes=(0,)),
               dict(classes=(257,)), dict(classes=(3, 300)), dict(ws_bytes=16)):
        assert refused(lib, descriptor(**kw)), kw
    d = descriptor(classes=(3, 3, 3, 3))
    d.nheads = 5
    assert refused(lib, d)
    for field in ("feats", "dx", "ws"):
        d = descriptor()
        setattr(d, field, None)
        assert refused(lib, d), field
    for field in ("w1", "b1", "w2", "b2", "targets", "grads", "loss", "correct"):
        d = descriptor(classes=(3, 4))
        setattr(d.head[1], field, None)
        assert refused(lib, d), field
    for p in (-0.1, 1.0, 1.5, float("nan")):
        d = descriptor()
        d.head[0].p = p
        assert refused(lib, d), p
    d = descriptor()
    d.head[0].counter = 0x90004  # not 8-byte aligned
    assert refused(lib, d)
    d = descriptor(classes=(3, 4))
    d.head[1].counter = d.head[0].counter  # two workgroups would advance one counter
    assert refused(lib, d)
    counts = (ctypes.c_int * 2)(3, 4)
    assert lib.air_adv_heads_ws_bytes(8, 16, 2, counts, 1) == 4 * (2 * (2 * 8 * 8 + 8 * 16) + 8 * 3 + 8 * 4)
    assert lib.air_adv_heads_ws_bytes(8, 16, 2, counts, 0) == 4 * (2 * 2 * 8 * 8 + 8 * 3 + 8 * 4)
    assert lib.air_adv_heads_ws_bytes(8, 15, 2, counts, 0) == 0 and lib.air_adv_heads_ws_bytes(8, 16, 5, counts, 0) == 0


def test_trainer_surface():
    from asvspoof2021_air_amd.adversarial import AdversarialTrainer
    params = inspect.signature(AdversarialTrainer.__init__).parameters
    names = list(params)
    assert names[:6] == ["self", "model", "n_channels", "lambda_", "lr_d", "recompute"] and names[6] == "fused_heads"
    assert params["fused_heads"].default is None
    assert list(inspect.signature(AdversarialTrainer.step).parameters) == [
        "self", "pcm", "labels", "channels", "start", "epoch_num", "lengths"]
    assert callable(AdversarialTrainer.epoch_accuracy)


def test_flat_classifier_keeps_state_dict_and_pickle():
    from asvspoof2021_air_amd.adversarial import ChannelClassifier
    from oracle import adversarial as o_adv
    from oracle.filler import fill_module_
    clf = fill_module_(ChannelClassifier(16, 5, 0.05))
    before = {k: v.clone() for k, v in clf.state_dict().items()}
    flat = clf.flatten()
    assert flat.numel() == 8 * 16 + 8 + 5 * 8 + 5 and clf.flatten() is flat
    assert {k: tuple(v.shape) for k, v in clf.state_dict().items()} == o_adv.classifier_shapes(16, 5)
    base = flat.data_ptr()
    for (k, v), off in zip(clf.state_dict().items(), (0, 128, 136, 176)):
        assert torch.equal(v, before[k]) and v.data_ptr() == base + 4 * off, k
    buf = io.BytesIO()
    torch.save(clf, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    assert list(back.state_dict()) == list(before)
    for k, v in back.state_dict().items():
        assert v.shape == before[k].shape and torch.equal(v, before[k]), k
    assert back._seed == clf._seed and back._offset == clf._offset
    with torch.no_grad():  # the views stay views of one block after the round trip
        back.flatten().zero_()
    assert all(float(v.abs().sum()) == 0 for v in back.state_dict().values())
