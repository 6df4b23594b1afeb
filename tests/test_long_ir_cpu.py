"""CPU: banks of impulse responses of different lengths (``augment.IRBank``, ``synthetic_room_bank``), the C entry points
behind them (``air_ir_bank_convolve``: declared, exported, argument checks ahead of any device work) and the float64
helper that tests/test_long_ir_gpu.py holds the kernels to - nothing here touches a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import channel as o_channel
from long_ir_oracle import bank_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE = -1, -4


def test_irbank_pads_and_keeps_the_tap_counts():
    from asvspoof2021_air_amd.augment import IRBank
    rng = np.random.default_rng(1)
    rows = [rng.standard_normal(5).astype(np.float32), torch.arange(1.0, 4.0), rng.standard_normal(2049), [2.0]]
    bank = IRBank(rows)
    assert len(bank) == 4 and bank.irs.shape == (4, 2049) and bank.irs.dtype == torch.float32
    assert bank.taps.dtype == torch.int32 and bank.taps.tolist() == [5, 3, 2049, 1]
    for i, r in enumerate(rows):
        r = torch.as_tensor(np.asarray(r)).float()
        assert torch.equal(bank.irs[i, : r.numel()], r) and int(torch.count_nonzero(bank.irs[i, r.numel():])) == 0
    same = bank.to("cpu")
    assert isinstance(same, IRBank) and torch.equal(same.irs, bank.irs) and torch.equal(same.taps, bank.taps)
    assert len(IRBank([np.ones(65536)])) == 1


def test_irbank_refuses_empty_and_oversized_responses():
    from asvspoof2021_air_amd.augment import IRBank
    for bad in ([], [np.ones(3), np.ones(0)], [np.ones(65537)], [np.ones((2, 3))]):
        with pytest.raises(ValueError):
            IRBank(bad)


def test_synthetic_room_bank():
    from asvspoof2021_air_amd.augment import IRBank, synthetic_ir_bank, synthetic_room_bank
    a, b = synthetic_room_bank(), synthetic_room_bank()
    assert isinstance(a, IRBank) and len(a) == 30
    assert torch.equal(a.irs, b.irs) and torch.equal(a.taps, b.taps)
    assert a.taps[:27].tolist() == [1024] * 27
    assert torch.equal(a.irs[:27, :1024], synthetic_ir_bank()[:27])  # the device responses of the dense bank
    space = a.taps[27:].tolist()
    assert all(1025 < t <= 16000 for t in space) and all(t >= 0.2 * 16000 for t in space) and a.irs.shape[1] == max(space)
    for i in range(30):
        t = int(a.taps[i])
        np.testing.assert_allclose(float((a.irs[i, :t].double() ** 2).sum()), 1.0, rtol=1e-6)
        assert int(torch.count_nonzero(a.irs[i, t:])) == 0 and (i < 27 or float(a.irs[i, t - 1]) != 0.0)
    c = synthetic_room_bank(seed=5)
    assert not torch.equal(a.taps, c.taps)
    d = synthetic_room_bank(n_device=2, n_space=1, rt60=(0.5, 0.5))
    assert d.taps.tolist() == [1024, 1024, 8000]


def test_bank_oracle_equals_definition():
    """The helper against the definition of the convolution at a small size: responses of 37, 5 and 300 taps in a table
    300 wide whose columns behind each tap count hold NaN, rows shorter than their response, one sample, a pass-through
    row, int16 input, tails of zero."""
    rng = np.random.default_rng(3)
    lengths, idx, taps = [260, 20, 1, 123, 200], np.array([1, 0, 2, -1, 2]), [37, 5, 300]
    irs = np.full((3, 300), np.nan)
    for i, t in enumerate(taps):
        irs[i, :t] = rng.standard_normal(t)
    x = rng.standard_normal((5, 260))
    x16 = (rng.standard_normal((5, 260)) * 3000).astype(np.int16)
    for b, n in enumerate(lengths):
        x[b, n:] = 1e6  # what lies behind a row's length must not reach the result
        x16[b, n:] = 32767
    for src, ref in ((x, x), (x16, x16.astype(np.float64) / 32768.0)):
        got = bank_oracle(src, lengths, irs, taps, idx, normalize=False)
        norm = bank_oracle(src, lengths, irs, taps, idx, normalize=True)
        assert np.isfinite(got).all() and np.isfinite(norm).all()
        for b, n in enumerate(lengths):
            assert not got[b, n:].any() and not norm[b, n:].any()
            if idx[b] < 0:
                assert np.array_equal(got[b, :n], ref[b, :n]) and np.array_equal(norm[b, :n], ref[b, :n])
                continue
            want = o_channel.ir_convolve_direct(ref[b, :n], irs[idx[b], : taps[idx[b]]])
            np.testing.assert_allclose(got[b, :n], want, atol=1e-11)
            np.testing.assert_allclose(np.abs(norm[b, :n]).max(), np.abs(ref[b, :n]).max(), rtol=1e-12)
            np.testing.assert_allclose(norm[b, :n] * np.abs(want).max(), want * np.abs(ref[b, :n]).max(), atol=1e-9)


@pytest.fixture(scope="module")
def lib():
    from asvspoof2021_air_amd import _hip
    return _hip.lib()  # (raises when the extension has not been built: there is no fallback)


def test_bank_entry_points_are_declared_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "air_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bsize_t\s+air_ir_bank_ws_bytes\s*\(\s*int\s+B\s*,\s*int\s+Lcap\s*,\s*int\s+n_ir\s*,\s*int\s+Hmax\s*\)", text)
    assert re.search(r"\bint\s+air_ir_bank_convolve\s*\(\s*const\s+float\s*\*\s*x\s*,\s*const\s+int16_t\s*\*\s*x16\s*,", text)
    assert re.search(r"const\s+int\s*\*\s*ir_taps_dev\s*,\s*const\s+int\s*\*\s*ir_idx\s*,", text)
    assert hasattr(lib, "air_ir_bank_convolve") and hasattr(lib, "air_ir_bank_ws_bytes")


def test_bank_workspace_size(lib):
    lib.air_ir_bank_ws_bytes.restype = ctypes.c_size_t
    lib.air_ir_convolve_ws_bytes_ex.restype = ctypes.c_size_t

    def ws(B, Lcap, n_ir, Hmax):
        return lib.air_ir_bank_ws_bytes(ctypes.c_int(B), ctypes.c_int(Lcap), ctypes.c_int(n_ir), ctypes.c_int(Hmax))

    assert ws(0, 100, 1, 1) == 0 and ws(1, 0, 1, 1) == 0 and ws(1, 100, 0, 1) == 0 and ws(1, 100, 1, 0) == 0
    assert ws(1, 100, 1, 65537) == 0 and ws(1, 100, 1, 65536) > 0
    # short banks: the peaks and the tables of the existing FFT route, nothing per sample
    assert ws(8, 64000, 30, 1024) == lib.air_ir_convolve_ws_bytes_ex(ctypes.c_int(8), ctypes.c_int(30), ctypes.c_int(1024))
    assert ws(8, 640000, 30, 1025) == ws(8, 64000, 30, 1025)
    # long banks: + a partition spectrum of 32 KB per 2048 taps and response, + the segment spectra (one packing with
    # a single partition, two otherwise; 32 KB per 4096 samples of capacity and row)
    assert ws(8, 64000, 30, 16000) - ws(8, 64000, 30, 1025) == (30 * 7 + 8 * 2 * 16) * 32768
    assert ws(8, 64000, 30, 2048) - ws(8, 64000, 30, 1025) == 8 * 1 * 16 * 32768
    assert ws(8, 64000, 30, 2049) - ws(8, 64000, 30, 2048) == (30 + 8 * 16) * 32768


def test_bank_entry_point_rejects_bad_arguments(lib):
    """AIR_EINVAL / AIR_EWORKSPACE ahead of any device work: the (fake) device pointers are never dereferenced."""
    fake = [ctypes.c_void_p(0x1000 * (k + 1)) for k in range(8)]
    x, x16, lengths, irs, taps, idx, y, ws = fake
    null = ctypes.c_void_p(0)
    lib.air_ir_bank_ws_bytes.restype = ctypes.c_size_t
    need = lib.air_ir_bank_ws_bytes(ctypes.c_int(2), ctypes.c_int(16000), ctypes.c_int(3), ctypes.c_int(5000))
    assert need > 0

    def call(x=x, x16=null, B=2, Lcap=16000, lengths=lengths, irs=irs, n_ir=3, Hmax=5000, taps=taps, normalize=0, y=y, ws=ws,
             ws_bytes=need):
        return lib.air_ir_bank_convolve(x, x16, ctypes.c_int(B), ctypes.c_int(Lcap), lengths, irs, ctypes.c_int(n_ir),
                                        ctypes.c_int(Hmax), taps, idx, ctypes.c_int(normalize), y, ws,
                                        ctypes.c_size_t(ws_bytes), null)

    assert call(Hmax=65537) == EINVAL and call(Hmax=1 << 20) == EINVAL
    assert call(taps=null) == EINVAL
    assert call(x=null, x16=null) == EINVAL
    assert call(x=x, x16=x16) == EINVAL
    assert call(y=x) == EINVAL  # in place
    assert call(B=0) == EINVAL and call(B=-2) == EINVAL
    assert call(Lcap=0) == EINVAL and call(n_ir=0) == EINVAL and call(Hmax=0) == EINVAL and call(Hmax=-5) == EINVAL
    assert call(y=null) == EINVAL and call(irs=null) == EINVAL
    # the tables live in the workspace: it is needed with and without normalize, for either sample type
    for nz in (0, 1):
        assert call(normalize=nz, ws_bytes=need - 1) == EWORKSPACE
        assert call(normalize=nz, ws=null) == EWORKSPACE
        assert call(x=null, x16=x16, normalize=nz, ws_bytes=0) == EWORKSPACE
    assert call(taps=null, ws_bytes=0) == EINVAL  # the arguments are judged first


def test_python_surface_takes_a_bank():
    from asvspoof2021_air_amd import _hip
    from asvspoof2021_air_amd.augment import AugmentChain, ChannelAugment, IRBank, ir_convolve
    bank = IRBank([np.ones(3), np.ones(2000)])
    with pytest.raises(_hip.AirError):  # no CPU fallback, as for a tensor
        ir_convolve(torch.zeros(2, 100), bank)
    aug = ChannelAugment(irs=bank, p=0.5, seed=1, device="cpu")
    assert isinstance(aug.irs, IRBank) and ChannelAugment.supports_lengths is True
    idx = aug.draw(64)
    assert np.array_equal(idx, ChannelAugment(irs=bank, p=0.5, seed=1, device="cpu").draw(64))
    assert set(np.unique(idx)) == {-1, 0, 1}
    chain = AugmentChain(device=ChannelAugment(irs=bank, p=0.5, seed=1, device="cpu"))
    labels = chain.prepare(64)
    assert torch.equal(labels, torch.from_numpy(np.where(idx < 0, 0, idx.astype(np.int64) + 1)))
