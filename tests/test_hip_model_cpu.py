"""CPU: what hip_model.HipModel gives the four HIP models without a GPU - runtime state stays out of whole-module
pickles, pickles of any age load (class-level defaults), the per-device Philox counter carries its count through a
pickle, and the base adds nothing to ``state_dict`` or to a seeded construction."""
import pickle

import pytest
import torch

from asvspoof2021_air_amd.hip_model import HipModel

RUNTIME = ("_arena", "_side_stream", "_bucketer", "_segment_cut")


def _resnet():
    from asvspoof2021_air_amd.resnet import ResNet
    return ResNet(3, 16, resnet_type="18", nclasses=2)


def _ecapa():
    from asvspoof2021_air_amd.ecapa_tdnn import Bottle2neck, Res2Net2
    return Res2Net2(Bottle2neck, C=64, model_scale=8, nOut=2, n_mels=60)


def _lcnn():
    from asvspoof2021_air_amd.lcnn import LCNN
    return LCNN(16, 16)


def _res2net():
    from asvspoof2021_air_amd.res2net import Res2Net, SEBottle2neck
    return Res2Net(SEBottle2neck, [1, 1, 1, 1], baseWidth=26, scale=4, num_classes=2)


BUILD = {"resnet": _resnet, "ecapa": _ecapa, "lcnn": _lcnn, "res2net": _res2net}
BUCKET = {"resnet": None, "ecapa": 8 << 20, "lcnn": 256 << 10, "res2net": 256 << 10}


def _load(cls, state):
    m = cls.__new__(cls)
    m.__setstate__(state)
    return m


@pytest.mark.parametrize("name", sorted(BUILD))
def test_pickle_drops_runtime_state(name):
    m = BUILD[name]()
    assert isinstance(m, HipModel)
    fresh = pickle.loads(pickle.dumps(m))
    # ... and a model that has been used: arenas bound, overlap on, a capture hook and a stream installed
    m.arena()
    m.enable_ddp_overlap()
    m._segment_cut = lambda lo: None  # (not picklable: it has to be dropped, not carried)
    m._side_stream = object()
    used = pickle.loads(pickle.dumps(m))
    for m2 in (fresh, used):
        for f in RUNTIME:
            assert f not in m2.__dict__ and getattr(m2, f) is None, f
        assert list(m2.state_dict()) == list(m.state_dict())
    for k, v in m.state_dict().items():
        assert torch.equal(used.state_dict()[k], v), k
    assert m._arena is not None and m._bucketer is not None  # pickling leaves the live model alone


@pytest.mark.parametrize("name", sorted(BUILD))
def test_stripped_dict_loads_and_enables_overlap(name):
    """A pickle from before a runtime field existed: the class-level defaults stand in."""
    m = BUILD[name]()
    st = {k: v for k, v in m.__getstate__().items() if k not in RUNTIME + ("overlap_wgrad",)}
    m2 = _load(type(m), st)
    for f in RUNTIME:
        assert getattr(m2, f) is None, f
    assert m2.overlap_wgrad is True
    assert m2.enable_ddp_overlap() is m2 and m2._bucketer is not None
    assert m2._bucketer.bucket_bytes == BUCKET[name]
    assert m2.enable_ddp_overlap(1 << 20)._bucketer.bucket_bytes == 1 << 20
    assert m2.arena().tail_names == type(m).TAIL and m2.arena().bound()


@pytest.mark.parametrize("name,field", [("resnet", "_noise"), ("lcnn", "_mask")])
def test_counter_survives_pickles_old_and_new(name, field):
    m = BUILD[name]()
    st = m.__getstate__()
    st[field + "_offset"] = 1234
    for k in (field + "_ctr", field + "_ctrs"):  # an old pickle carries the host offset only
        st.pop(k, None)
    m2 = _load(type(m), st)
    assert getattr(m2, field + "_offset") == 1234
    assert getattr(m2, field + "_ctr") is None and getattr(m2, field + "_ctrs") is None
    cpu = torch.device("cpu")
    ctr = m2.device_counter(field, cpu)  # the rule itself needs no GPU
    assert ctr.dtype == torch.int64 and ctr.item() == 1234 and getattr(m2, field + "_ctr") is ctr
    ctr += 8  # what a draw does on the device
    assert m2.device_counter(field, cpu) is ctr  # one counter per device, never replaced
    m3 = pickle.loads(pickle.dumps(m2))
    assert getattr(m3, field + "_offset") == 1242 and getattr(m3, field + "_ctr") is None
    assert m3.device_counter(field, cpu).item() == 1242
    assert ctr.item() == 1242 and getattr(m2, field + "_ctr") is ctr  # pickling leaves the live counter alone


def test_base_adds_nothing_to_a_model():
    before = torch.get_rng_state()
    base = HipModel()
    assert torch.equal(torch.get_rng_state(), before)
    assert len(base.state_dict()) == 0 and not list(base.named_parameters()) and not list(base.named_buffers())
    assert not list(base.children())
    for build in BUILD.values():
        assert issubclass(type(build()), HipModel)
