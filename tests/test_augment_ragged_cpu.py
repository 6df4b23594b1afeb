"""CPU: the ragged IR augmentation's C entry point (``air_ir_convolve_ragged``: declared, exported, its argument checks
ahead of any device work), its Python surface, and the per-row statement of the oracle that tests/test_augment_ragged_gpu.py
holds the kernel to - nothing here touches a GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from oracle import channel as o_channel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE = -1, -4


def ragged_oracle(x, lengths, irs, idx, normalize=True):
    """The spec of a ragged batch: row b is oracle/channel.py on x[b, :L_b] alone, followed by zeros.  float64 (B, Lcap)."""
    out = np.zeros(np.shape(x), dtype=np.float64)
    for b, n in enumerate(lengths):
        out[b, :n] = o_channel.ir_convolve(np.asarray(x)[b:b + 1, :n], irs, idx[b:b + 1], normalize)[0]
    return out


@pytest.fixture(scope="module")
def lib():
    from asvspoof2021_air_amd import _hip
    return _hip.lib()  # (raises when the extension has not been built: there is no fallback)


def test_ragged_entry_point_is_declared_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "air_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+air_ir_convolve_ragged\s*\(\s*const\s+float\s*\*\s*x\s*,\s*const\s+int16_t\s*\*\s*x16\s*,", text)
    assert hasattr(lib, "air_ir_convolve_ragged")


def test_ragged_entry_point_rejects_bad_arguments(lib):
    """AIR_EINVAL / AIR_EWORKSPACE ahead of any device work: the (fake) device pointers are never dereferenced."""
    fake = [ctypes.c_void_p(0x1000 * (k + 1)) for k in range(7)]
    x, x16, lengths, irs, idx, y, ws = fake
    null = ctypes.c_void_p(0)
    lib.air_ir_convolve_ws_bytes.restype = ctypes.c_size_t
    need = lib.air_ir_convolve_ws_bytes(ctypes.c_int(2))
    assert need > 0

    def call(x=x, x16=null, B=2, Lcap=16000, lengths=lengths, irs=irs, n_ir=3, H=37, normalize=0, y=y, ws=ws, ws_bytes=need):
        return lib.air_ir_convolve_ragged(x, x16, ctypes.c_int(B), ctypes.c_int(Lcap), lengths, irs, ctypes.c_int(n_ir),
                                          ctypes.c_int(H), idx, ctypes.c_int(normalize), y, ws, ctypes.c_size_t(ws_bytes), null)

    assert call(lengths=null) == EINVAL
    assert call(x=null, x16=null) == EINVAL
    assert call(x=x, x16=x16) == EINVAL
    assert call(y=x) == EINVAL  # in place
    assert call(B=0) == EINVAL and call(B=-2) == EINVAL
    assert call(Lcap=0) == EINVAL and call(n_ir=0) == EINVAL and call(H=0) == EINVAL
    assert call(y=null) == EINVAL and call(irs=null) == EINVAL
    # the peaks live in the workspace: normalize needs air_ir_convolve_ws_bytes(B) of it, for either sample type
    assert call(normalize=1, ws_bytes=need - 1) == EWORKSPACE
    assert call(normalize=1, ws=null) == EWORKSPACE
    assert call(x=null, x16=x16, normalize=1, ws_bytes=0) == EWORKSPACE
    assert call(lengths=null, normalize=1, ws_bytes=0) == EINVAL  # the arguments are judged first


def test_python_surface_takes_lengths():
    from asvspoof2021_air_amd.adversarial import AdversarialTrainer
    from asvspoof2021_air_amd.augment import ChannelAugment, ir_convolve
    sig = inspect.signature(ir_convolve).parameters
    assert list(sig) == ["pcm", "irs", "idx", "normalize", "out", "lengths"] and sig["lengths"].default is None
    sig = inspect.signature(ChannelAugment.__call__).parameters
    assert list(sig) == ["self", "pcm", "idx", "lengths"] and sig["lengths"].default is None
    assert ChannelAugment.supports_lengths is True
    sig = inspect.signature(AdversarialTrainer.step).parameters
    assert list(sig) == ["self", "pcm", "labels", "channels", "start", "epoch_num", "lengths"] and sig["lengths"].default is None


def test_ragged_oracle_equals_definition():
    """The per-row restatement of oracle/channel.py against the definition of the convolution: 300 samples of capacity,
    37 taps, three lengths (the full row, fewer samples than taps, one sample), a pass-through row, tails of zero."""
    rng = np.random.default_rng(3)
    lengths = [300, 20, 1, 123]
    x = rng.standard_normal((4, 300))
    irs = rng.standard_normal((2, 37))
    idx = np.array([1, 0, 1, -1])
    for b, n in enumerate(lengths):
        x[b, n:] = 1e6  # what lies behind a row's length must not reach the result
    got = ragged_oracle(x, lengths, irs, idx, normalize=False)
    norm = ragged_oracle(x, lengths, irs, idx, normalize=True)
    for b, n in enumerate(lengths):
        assert np.array_equal(got[b, n:], np.zeros(300 - n)) and np.array_equal(norm[b, n:], np.zeros(300 - n))
        if idx[b] < 0:
            assert np.array_equal(got[b, :n], x[b, :n]) and np.array_equal(norm[b, :n], x[b, :n])
            continue
        want = o_channel.ir_convolve_direct(x[b, :n], irs[idx[b]])
        np.testing.assert_allclose(got[b, :n], want, atol=1e-12)
        np.testing.assert_allclose(np.abs(norm[b, :n]).max(), np.abs(x[b, :n]).max(), rtol=1e-12)
        np.testing.assert_allclose(norm[b, :n] * np.abs(want).max(), want * np.abs(x[b, :n]).max(), atol=1e-9)
