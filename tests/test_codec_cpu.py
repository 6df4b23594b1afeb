"""CPU: the G.711 codec augmentation's oracle (tests/codec_oracle.py), its low-pass design, the C entry point's argument
checks ahead of any device work, and the host-side logic of ``CodecAugment`` / ``AugmentChain`` - nothing here touches a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import codec_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE = -1, -4


@pytest.fixture(scope="module")
def lib():
    from asvspoof2021_air_amd import _hip
    return _hip.lib()  # (raises when the extension has not been built: there is no fallback)


@pytest.mark.parametrize("law", [0, 1], ids=co.LAWS)
def test_oracle_coding_is_idempotent_with_255_and_256_levels(law):
    enc, dec = co.tables(law)
    assert enc.shape == (65536,) and dec.shape == (256,)
    decoded = dec[enc]
    assert np.array_equal(co.encode(decoded, law), enc)  # code(decode(code(s))) == code(s)
    assert len(np.unique(decoded)) == (255 if law == 0 else 256)
    s = np.arange(-32768, 32768)
    # the decoded level lies within one step of the sample (mu-law clips its top 14-bit magnitudes: 8159 * 4 = 32636)
    inside = np.abs(s) <= 32635
    assert np.all(np.abs(decoded.astype(np.int64) - s)[inside] <= co.step_at(enc, law)[inside])


def test_oracle_filters_equal_the_literal_definition():
    rng = np.random.default_rng(5)
    for L, fir in ((41, [0.25, 0.5, 0.25]), (40, rng.standard_normal(7) * 0.2), (1, [0.1, 0.7, 0.1]), (9, [1.0])):
        x = rng.uniform(-0.9, 0.9, L)
        for law in (0, 1):
            codes, y = co.codec_definition(x, fir, law)
            row = co.codec_row(x, fir, law, resample=True, normalize=False)
            assert np.array_equal(codes, row["codes"]) and len(codes) == (L + 1) // 2
            np.testing.assert_allclose(row["y"], y, atol=1e-15)
    row = co.codec_row(x, fir, -1)
    assert np.array_equal(row["y"], x)


def test_codec_lowpass_equals_firwin():
    from scipy.signal import firwin
    from asvspoof2021_air_amd import augment
    want = firwin(63, 0.46, window=("kaiser", 8.0))
    h64 = augment._lowpass64(63, 3680.0, 16000, 8.0)
    assert np.abs(h64 - want).max() <= 1e-12
    h = augment.codec_lowpass()
    assert h.dtype == torch.float32 and h.shape == (63,)
    assert np.array_equal(h.numpy(), want.astype(np.float32)) or np.abs(h.numpy().astype(np.float64) - want).max() <= 2.0 ** -25
    assert abs(float(h.double().sum()) - 1.0) <= 1e-6 and abs(np.abs(want).sum() - 1.855) < 1e-3
    want = firwin(31, 0.5, window=("kaiser", 5.0))
    assert np.abs(augment._lowpass64(31, 2000.0, 8000, 5.0) - want).max() <= 1e-12
    with pytest.raises(ValueError):
        augment.codec_lowpass(ntaps=64)


def test_entry_point_is_declared_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "air_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+air_g711_ragged\s*\(\s*const\s+float\s*\*\s*x\s*,\s*const\s+int16_t\s*\*\s*x16\s*,", text)
    assert re.search(r"\bsize_t\s+air_g711_ws_bytes\s*\(\s*int\s+B\s*\)", text)
    assert hasattr(lib, "air_g711_ragged") and hasattr(lib, "air_g711_ws_bytes")


def test_entry_point_rejects_bad_arguments(lib):
    """AIR_EINVAL / AIR_EWORKSPACE ahead of any device work: the (fake) device pointers are never dereferenced, and this
    machine need not have a GPU."""
    fake = [ctypes.c_void_p(0x1000 * (k + 1)) for k in range(8)]
    x, x16, lengths, fir, law, y, codes, ws = fake
    null = ctypes.c_void_p(0)
    lib.air_g711_ws_bytes.restype = ctypes.c_size_t
    need = lib.air_g711_ws_bytes(ctypes.c_int(2))
    assert need > 0 and lib.air_g711_ws_bytes(ctypes.c_int(0)) == 0

    def call(x=x, x16=null, B=2, Lcap=16000, lengths=lengths, fir=fir, ntaps=63, resample=1, normalize=0, y=y, ws=ws,
             ws_bytes=need):
        return lib.air_g711_ragged(x, x16, ctypes.c_int(B), ctypes.c_int(Lcap), lengths, fir, ctypes.c_int(ntaps), law,
                                   ctypes.c_int(resample), ctypes.c_int(normalize), y, codes, ws, ctypes.c_size_t(ws_bytes), null)

    assert call(x=null, x16=null) == EINVAL
    assert call(x=x, x16=x16) == EINVAL
    assert call(y=x) == EINVAL  # in place
    assert call(y=null) == EINVAL
    assert call(B=0) == EINVAL and call(B=-2) == EINVAL and call(Lcap=0) == EINVAL and call(Lcap=-5) == EINVAL
    for ntaps in (0, -1, 2, 62, 128, 129, 1001):
        assert call(ntaps=ntaps) == EINVAL and call(ntaps=ntaps, resample=0) == EINVAL
    assert call(fir=null) == EINVAL
    assert call(normalize=1, ws_bytes=need - 1) == EWORKSPACE
    assert call(normalize=1, ws=null) == EWORKSPACE
    assert call(x=null, x16=x16, normalize=1, ws_bytes=0) == EWORKSPACE
    assert call(lengths=null, resample=0, normalize=1, ws_bytes=0) == EWORKSPACE  # NULL lengths: the dense batch
    assert call(ntaps=2, normalize=1, ws_bytes=0) == EINVAL  # the arguments are judged first


def test_codec_augment_draw_is_reproducible_and_honours_p():
    from asvspoof2021_air_amd.augment import CodecAugment
    a, b = CodecAugment(seed=3, device="cpu"), CodecAugment(seed=3, device="cpu")
    da = [a.draw(64) for _ in range(3)]
    assert all(np.array_equal(x, b.draw(64)) for x in da)
    assert da[0].dtype == np.int32 and set(np.concatenate(da).tolist()) == {0, 1}
    assert not np.array_equal(da[0], CodecAugment(seed=4, device="cpu").draw(64))
    assert set(CodecAugment(p=0.0, device="cpu").draw(50).tolist()) == {-1}
    half = CodecAugment(p=0.5, seed=1, device="cpu").draw(4000)
    assert 0.45 < float((half < 0).mean()) < 0.55 and set(half.tolist()) == {-1, 0, 1}
    assert set(CodecAugment(laws=("alaw",), device="cpu").draw(20).tolist()) == {0}
    assert CodecAugment.supports_lengths is True
    with pytest.raises(ValueError):
        CodecAugment(laws=("g726",), device="cpu")


class _Stub:
    """A stage that records what it is called with; draws the fixed sequence it was given."""

    def __init__(self, draws, add):
        self.draws, self.add, self.calls = list(draws), add, []

    def draw(self, batch):
        return np.asarray(self.draws.pop(0)[:batch], dtype=np.int32)

    def __call__(self, pcm, idx=None, lengths=None):
        if idx is None:
            idx = self.draw(pcm.shape[0])
        self.calls.append((np.asarray(idx).tolist(), lengths))
        return pcm * 2 + self.add  # (order-sensitive)


def test_augment_chain_prepare_labels_and_order():
    from asvspoof2021_air_amd.augment import AugmentChain
    codec, device = _Stub([[1, -1, 0, 1], [0, 0, 0, 0]], 1.0), _Stub([[-1, 4, 29, 0], [2, 2, 2, 2]], 0.0)
    chain = AugmentChain(codec, device)
    assert AugmentChain.supports_lengths is True
    labels = chain.prepare(4)
    assert labels.dtype == torch.int64 and labels.tolist() == [[2, 0], [0, 5], [1, 30], [2, 1]]
    x = torch.ones(4, 8)
    y = chain(x)
    assert codec.calls == [([1, -1, 0, 1], None)] and device.calls == [([-1, 4, 29, 0], None)]
    assert torch.equal(y, (x * 2 + 1.0) * 2)  # codec first, then device
    # the prepared draw is consumed: the next call draws for itself
    chain(x)
    assert codec.calls[1][0] == [0, 0, 0, 0] and device.calls[1][0] == [2, 2, 2, 2]
    # one stage: (B,) labels
    only = AugmentChain(codec=_Stub([[0, -1, 1]], 0.0))
    assert only.prepare(3).tolist() == [1, 0, 2]
    only = AugmentChain(device=_Stub([[7, -1, 0]], 0.0))
    lab = only.prepare(3)
    assert lab.shape == (3,) and lab.tolist() == [8, 0, 1]
    with pytest.raises(ValueError):
        only(torch.ones(2, 8))  # prepared for another batch size
    with pytest.raises(ValueError):
        AugmentChain()
    # refused lengths draw nothing and leave the prepared draw in place
    chain = AugmentChain(_Stub([[1, 1]], 0.0), _Stub([[3, 3]], 0.0))
    chain.prepare(2)
    with pytest.raises(ValueError):
        chain(torch.ones(2, 8), lengths=[0, 8])
    assert chain._prepared is not None and chain.stages[0].calls == []


def test_g711_codec_refuses_cpu_tensors():
    from asvspoof2021_air_amd import _hip
    from asvspoof2021_air_amd.augment import CodecAugment, g711_codec
    with pytest.raises(_hip.AirError):
        g711_codec(torch.zeros(2, 100))
    with pytest.raises(_hip.AirError):
        g711_codec(torch.zeros(2, 100, dtype=torch.int16), torch.zeros(2, dtype=torch.int32))
    aug = CodecAugment(device="cpu")
    state = aug.rng.bit_generator.state
    with pytest.raises(ValueError):
        aug(torch.zeros(2, 100), lengths=[0, 5])
    assert aug.rng.bit_generator.state == state  # a refused batch draws nothing
