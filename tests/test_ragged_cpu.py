"""CPU: the ``return_pcm='ragged'`` collate (dataset.py) and the argument checks of ``air_lfcc_fwd_ragged`` - nothing here
touches a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEAT_LEN = 40
# samples: T = 1, 2, 28 (one full tile), 29, 40 (= feat_len), 41, 101, and two more long ones (three crop draws)
LENGTHS = [159, 160, 28 * 160 - 1, 28 * 160, 39 * 160, 40 * 160, 100 * 160 + 37, 77 * 160 + 3, 3000, 55 * 160]


def _items(lengths, dtype=np.float32, first=0):
    rng = np.random.RandomState(11)
    out = []
    for i, n in enumerate(lengths):
        w = rng.standard_normal(n).astype(np.float32) * 0.1
        if dtype == np.int16:
            w = np.clip(np.round(w * 32768.0), -32768, 32767).astype(np.int16)
        out.append(("%05d_LA_T_%07d_%s_%s" % (first + i, 1000000 + first + i, "A%02d" % (1 + i % 6) if i % 2 else "-",
                                              "spoof" if i % 2 else "bonafide"), w))
    return out


def _dataset(items, mode="ragged"):
    from asvspoof2021_air_amd.dataset import ASVspoof2019, PCMSource
    return ASVspoof2019("LA", None, "train", feat_len=FEAT_LEN, source=PCMSource(items, device="cpu"), return_pcm=mode)


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_ragged_collate_tuple(dtype):
    items = _items(LENGTHS, dtype)
    ds = _dataset(items)
    assert ds.ragged_samples is None
    ds.ragged_samples = 17000
    np.random.seed(123)
    pcm, lengths, start, names, tags, labels = ds.collate_fn([ds[i] for i in range(len(ds))])
    assert pcm.shape == (len(items), 17000) and pcm.dtype == (torch.float32 if dtype == np.float32 else torch.int16)
    assert lengths.dtype == torch.int32 and lengths.tolist() == LENGTHS
    for j, (_, w) in enumerate(items):
        np.testing.assert_array_equal(pcm[j, :len(w)].numpy(), w)
        assert torch.count_nonzero(pcm[j, len(w):]) == 0
    # the crop draws of dataset.py:69, in item order, one per utterance longer than feat_len
    np.random.seed(123)
    want = [np.random.randint(1 + n // 160 - FEAT_LEN) if 1 + n // 160 > FEAT_LEN else 0 for n in LENGTHS]
    assert start.dtype == torch.int32 and start.tolist() == want
    assert sum(1 for v in want if v) >= 2 and want[4] == 0  # (T = feat_len draws nothing)
    assert list(names) == ["_".join(n.split("_")[1:4]) for n, _ in items]
    assert labels.tolist() == [i % 2 for i in range(len(items))] and tags.tolist() == [(1 + i % 6) if i % 2 else 0 for i in range(len(items))]


def test_ragged_collate_rewrites_the_tails_of_a_reused_buffer():
    """The rows come out of a ring of reused buffers: a shorter utterance must not inherit the last one's samples."""
    ds = _dataset(_items([5000, 300]))
    ds.ragged_samples = 6000
    ds.PINNED_RING = 1
    a = ds.collate_fn([ds[0], ds[0]])[0].clone()
    b = ds.collate_fn([ds[1], ds[1]])[0]
    assert torch.count_nonzero(a[:, 300:5000]) > 0 and torch.count_nonzero(b[:, 300:]) == 0


def test_ragged_capacity():
    items = _items([159, 16000, 16001, 40000])
    ds = _dataset(items)
    # None: the batch's longest utterance rounded up to a multiple of 16000
    assert ds.collate_fn([ds[0]])[0].shape == (1, 16000)
    assert ds.collate_fn([ds[0], ds[1]])[0].shape == (2, 16000)
    assert ds.collate_fn([ds[1], ds[2]])[0].shape == (2, 32000)
    assert ds.collate_fn([ds[3], ds[0]])[0].shape == (2, 48000)
    ds.ragged_samples = 16001
    assert ds.collate_fn([ds[0], ds[2]])[0].shape == (2, 16001)
    with pytest.raises(ValueError, match=r"LA_T_1000003.*16001"):  # names the file and the capacity
        ds.collate_fn([ds[0], ds[3]])


def test_ragged_mixed_dtypes_raise():
    ds = _dataset(_items([500], np.float32) + _items([600], np.int16, first=1))
    with pytest.raises(ValueError, match="dtype"):
        ds.collate_fn([ds[0], ds[1]])
    ds64 = _dataset([("00000_LA_T_1000000_-_bonafide", np.zeros(500, np.float64))])
    with pytest.raises(ValueError, match="dtype"):
        ds64.collate_fn([ds64[0]])


def test_batch_mode_still_raises_on_mixed_lengths():
    ds = _dataset(_items([500, 600]), mode="batch")
    assert ds.return_pcm == "batch"
    with pytest.raises(ValueError, match="one length per batch"):
        ds.collate_fn([ds[0], ds[1]])
    pcm = ds.collate_fn([ds[0], ds[0]])[0]
    assert pcm.shape == (2, 500)
    assert _dataset(_items([500]), mode=True).return_pcm is True and _dataset(_items([500]), mode=False).return_pcm is False


@pytest.fixture(scope="module")
def lib():
    from asvspoof2021_air_amd import _hip
    return _hip.lib()  # (raises when the extension has not been built: there is no fallback)


def test_ragged_entry_point_is_declared_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "air_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+air_lfcc_fwd_ragged\s*\(", text)
    assert hasattr(lib, "air_lfcc_fwd_ragged")


def test_ragged_entry_point_rejects_bad_arguments(lib):
    """AIR_EINVAL ahead of any device work: the (fake) device pointers are never dereferenced."""
    fake = [ctypes.c_void_p(0x1000 * (k + 1)) for k in range(6)]
    pcm, pcm16, lengths, out, plan, start = fake
    null = ctypes.c_void_p(0)

    def call(pcm=pcm, pcm16=null, lengths=lengths, feat_len=40, pad_mode=0, silence=null):
        return lib.air_lfcc_fwd_ragged(pcm, pcm16, ctypes.c_int(2), ctypes.c_int(16000), lengths, out, ctypes.c_int(feat_len),
                                       start, plan, ctypes.c_int(3), ctypes.c_int(pad_mode), silence, null)

    assert call(lengths=null) == -1
    assert call(pcm=null, pcm16=null) == -1
    assert call(pcm=pcm, pcm16=pcm16) == -1
    assert call(feat_len=0) == -1
    assert call(feat_len=-3) == -1
    assert call(pad_mode=3) == -1 and call(pad_mode=-1) == -1
    assert call(pad_mode=2, silence=null) == -1  # 'silence' without the frame to prepend
