"""CPU: the host helpers of ragged.py - the ``lengths`` check every ragged entry point shares, the pinned ring and the
row-status check - and that their callers reach them.  Nothing here touches a GPU."""
import numpy as np
import pytest
import torch

from asvspoof2021_air_amd import ragged
from asvspoof2021_air_amd.ragged import PinnedRing, check_status, device_lengths, round_capacity

B, LCAP = 3, 1000
GOOD = [1, 500, 1000]


@pytest.mark.parametrize("lengths", [GOOD, torch.tensor(GOOD, dtype=torch.int64), np.array(GOOD, dtype=np.int32)],
                         ids=["list", "int64 tensor", "int32 array"])
def test_device_lengths_accepts_host_integers(lengths):
    got = device_lengths(lengths, B, LCAP, "cpu")
    assert got.dtype == torch.int32 and got.is_contiguous() and got.tolist() == GOOD
    assert device_lengths(lengths, B, LCAP, "cpu", non_blocking=True).tolist() == GOOD


def _raise(host, Lcap):
    raise ValueError("extra: %s in %d" % (host.tolist(), Lcap))


BAD = {"wrong count": [1, 2], "float": [1.0, 2.0, 3.0], "bool": [True, True, False], "zero": [0, 5, 5],
       "beyond the capacity": [5, 5, LCAP + 1]}


@pytest.mark.parametrize("name", sorted(BAD))
def test_device_lengths_refuses(name):
    with pytest.raises(ValueError, match="lengths must"):
        device_lengths(BAD[name], B, LCAP, "cpu")


def test_device_lengths_extra_check_runs_behind_the_range_check():
    with pytest.raises(ValueError, match=r"extra: \[1, 500, 1000\] in 1000"):
        device_lengths(GOOD, B, LCAP, "cpu", extra_check=_raise)
    with pytest.raises(ValueError, match="lie in"):  # the range check comes first
        device_lengths(BAD["zero"], B, LCAP, "cpu", extra_check=_raise)
    seen = []
    device_lengths(GOOD, B, LCAP, "cpu", extra_check=lambda host, Lcap: seen.append((host.tolist(), Lcap)))
    assert seen == [(GOOD, LCAP)]


def test_device_lengths_of_an_empty_batch():
    got = device_lengths(torch.zeros(0, dtype=torch.int64), 0, LCAP, "cpu")  # (no min() of nothing)
    assert got.shape == (0,) and got.dtype == torch.int32
    with pytest.raises(ValueError, match="lengths must be 0 integers"):
        device_lengths([7], 0, LCAP, "cpu")


def _augmenters():
    from asvspoof2021_air_amd.augment import ChannelAugment, CodecAugment, RawBoostAugment
    return [ChannelAugment(irs=torch.ones(2, 4), p=0.5, device="cpu"), CodecAugment(p=0.5, device="cpu"),
            RawBoostAugment(p=0.5, device="cpu")]


@pytest.mark.parametrize("k", range(3), ids=["channel", "codec", "rawboost"])
@pytest.mark.parametrize("name", sorted(BAD))
def test_a_refused_batch_does_not_advance_the_augmenters_generator(k, name):
    aug = _augmenters()[k]
    before = aug.rng.bit_generator.state
    with pytest.raises(ValueError, match="lengths must"):
        aug(torch.zeros(B, LCAP), lengths=BAD[name])
    assert aug.rng.bit_generator.state == before
    idx, lengths = aug._begin(torch.zeros(B, LCAP), None, GOOD)  # an accepted one draws
    assert aug.rng.bit_generator.state != before and idx.shape == (B,) and lengths.tolist() == GOOD


def test_the_four_callers_refuse_alike():
    """LFCC.forward_ragged, _Spectral.forward_ragged, Trainer._ragged_lengths and the augmenters refuse CPU tensors ahead
    of the lengths, so the helper is called here the way each of them calls it."""
    from asvspoof2021_air_amd.feature_extraction import Melspec
    from asvspoof2021_air_amd.train import Trainer
    pcm = torch.zeros(B, LCAP)
    mel = Melspec("reflect")
    callers = {
        "LFCC": lambda l: device_lengths(l, B, LCAP, pcm.device),
        "Melspec": lambda l: device_lengths(l, B, LCAP, pcm.device, extra_check=mel._check_lengths),
        "Trainer": lambda l: Trainer._ragged_lengths(None, l, pcm),
        "augmenter": lambda l: _augmenters()[0](pcm, lengths=l),
    }
    for who, call in callers.items():
        for name in ("bool", "zero", "beyond the capacity"):
            with pytest.raises(ValueError, match="lengths must"):
                call(BAD[name])
    assert callers["Trainer"](GOOD).tolist() == GOOD and callers["Melspec"]([257, 500, 1000]).tolist() == [257, 500, 1000]
    with pytest.raises(ValueError, match="at least 257"):  # the Melspec rule rides on the shared check
        callers["Melspec"](GOOD)


def test_round_capacity_and_the_one_constant():
    from asvspoof2021_air_amd import corpus, dataset, flac, resample
    assert ragged.RAGGED_ROUND == 16000
    for home in (flac, resample, corpus, dataset._SpoofDataset):
        assert home.RAGGED_ROUND is ragged.RAGGED_ROUND
    assert [round_capacity(n) for n in (0, 1, 16000, 16001, 40000)] == [16000, 16000, 16000, 32000, 48000]
    assert resample.DeviceRing is ragged.DeviceRing and issubclass(flac.FlacDecoder, ragged.DeviceRing)


def test_pinned_ring_without_cuda(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    ring = PinnedRing(2)
    a = ring.take("k", (3, 5), torch.int16)
    assert a.shape == (3, 5) and a.dtype == torch.int16 and not hasattr(a, "_air_ring")
    assert ring.take("k", (3, 5), torch.int16) is not a


class _Event:
    def __init__(self):
        self.waited = 0

    def synchronize(self):
        self.waited += 1


def test_pinned_ring_reuses_a_slot_behind_its_event(monkeypatch):
    real, pinned = torch.empty, []

    def empty(*args, pin_memory=False, **kw):
        pinned.append(pin_memory)
        return real(*args, **kw)

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch, "empty", empty)
    depth = 3
    ring = PinnedRing(depth)
    bufs = [ring.take(("b", 4), (4, 8), torch.float32) for _ in range(depth)]
    assert pinned == [True] * depth and len(set(id(b) for b in bufs)) == depth
    for j, b in enumerate(bufs):
        assert b.shape == (4, 8) and b.dtype == torch.float32 and b._air_ring[1] == j and b._air_ring[0] is bufs[0]._air_ring[0]
    ev = _Event()
    events, j = bufs[1]._air_ring
    events[j] = ev  # what DevicePrefetcher does behind its copy
    assert ring.take(("b", 4), (4, 8), torch.float32) is bufs[0] and ev.waited == 0
    assert ring.take(("b", 4), (4, 8), torch.float32) is bufs[1] and ev.waited == 1 and events[1] is None
    assert ring.take(("b", 4), (4, 8), torch.float32) is bufs[2] and ev.waited == 1
    assert pinned == [True] * depth  # nothing allocated since
    assert ring.take(("other", 4), (4, 8), torch.float32) is not bufs[0]  # another key, another ring


def test_check_status_lists_the_rows_that_are_not_ok():
    from asvspoof2021_air_amd import flac, resample, wav
    check_status(torch.zeros(4, dtype=torch.int32), 0, flac.FlacError)
    status = torch.tensor([0, 3, 0, 5], dtype=torch.int32)
    with pytest.raises(flac.FlacError, match=r"FLAC decode failed for 2 row\(s\): row 1 UNSUPPORTED, row 3 CANDIDATE_OVERFLOW") as e:
        check_status(status, flac.OK, flac.FlacError)
    assert e.value.rows == [(1, 3), (3, 5)]
    for call, error in ((flac.check, flac.FlacError), (flac.FlacDecoder.check, flac.FlacError), (wav.check, wav.WavError),
                        (wav.WavDecoder.check, wav.WavError), (resample.check, resample.ResampleError)):
        call(torch.zeros(2, dtype=torch.int32))
        with pytest.raises(error) as e:
            call(status)
        assert e.value.rows == [(1, 3), (3, 5)] and type(e.value) is error
