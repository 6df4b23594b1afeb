"""CPU: the STFT / Melspec front-ends' oracle against the fixture of the real reference, the host plan builder against
the fp64 formulas, and the public surface (tests/test_spectral_gpu.py runs the kernels)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import spectral_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_BOUND = 1e-6  # fp64 oracle against the fp32 baselines; the reference's own fp32 error measures 6.3e-7 at worst


def test_public_surface():
    from asvspoof2021_air_amd.feature_extraction import STFT, Melspec  # (fails without the feature)
    assert list(inspect.signature(STFT.__init__).parameters)[1:] == ["fl", "fs", "fn", "sr", "with_emphasis"]
    assert inspect.signature(STFT.__init__).parameters["with_emphasis"].default is True
    assert list(inspect.signature(Melspec.__init__).parameters)[1:] == ["pad_mode"]
    m = STFT(320, 160, 512, 16000)
    assert (m.out_dim, m.fs, m.mutate_input) == (257, 160, True) and list(m.state_dict()) == []
    assert (Melspec().out_dim, Melspec().fs, Melspec().pad_mode) == (128, 128, "reflect")
    for name in ("forward", "forward_padded", "forward_ragged", "plan"):
        assert callable(getattr(STFT, name)) and callable(getattr(Melspec, name))
    assert callable(Melspec.forward_batch)
    with pytest.raises(NotImplementedError):
        STFT(400, 160, 512, 16000)
    with pytest.raises(NotImplementedError):
        STFT(320, 128, 512, 16000)
    with pytest.raises(ValueError):
        Melspec("edge")


def test_cpu_tensors_and_silence_padding_are_refused():
    from asvspoof2021_air_amd import _hip
    from asvspoof2021_air_amd.feature_extraction import STFT, Melspec
    x = torch.zeros(2, 1600)
    for m in (STFT(320, 160, 512, 16000), Melspec(), Melspec("constant")):
        for call in (lambda: m(x), lambda: m.forward_padded(x, 48), lambda: m.forward_ragged(x, [1600, 800], 48)):
            with pytest.raises(_hip.AirError):
                call()
        for call in (lambda: m.forward_padded(x, 48, None, "silence"), lambda: m.forward_ragged(x, [1600, 800], 48, None, "silence")):
            with pytest.raises(NotImplementedError, match="LFCC"):
                call()
        with pytest.raises(ValueError, match="Padding should be zero or repeat!"):
            m.forward_padded(x, 48, None, "reflect")
    with pytest.raises(_hip.AirError):
        Melspec().forward_batch(x)


def test_dataset_refuses_features_without_a_front_end():
    from asvspoof2021_air_amd import dataset as air_ds
    items = [("00000_LA_T_1000000_-_bonafide", torch.zeros(1600))]
    with pytest.raises(ValueError, match="CQCC"):
        air_ds.ASVspoof2019("LA", None, feature="CQCC", source=air_ds.PCMSource(items, device="cpu"))
    for f in ("LFCC", "STFT", "Melspec"):
        ds = air_ds.ASVspoof2019("LA", None, feature=f, source=air_ds.PCMSource(items, device="cpu"))
        assert type(ds.frontend).__name__ == f
    with pytest.raises(NotImplementedError, match="LFCC"):  # the silence frame is an LFCC frame (dataset.py:13-16)
        air_ds.ASVspoof2019("LA", None, feature="STFT", padding="silence", source=air_ds.PCMSource(items, device="cpu"))


def test_oracle_matches_the_reference_fixture(golden):
    from oracle import lfcc as o_lfcc
    g = golden("spectral.npz")
    assert np.array_equal(so.mel_filterbank(), g["mel_fb"])
    for tag, x in so.golden_cases(g):
        assert g["stft" + tag].shape == (x.shape[0], 1 + x.shape[1] // 160, 257)
        # the reference's in-place pre-emphasis (feature_extraction.py:157), bit for bit
        assert np.array_equal(o_lfcc.pre_emphasis_(x.numpy().copy())[:, :64], g["xmut" + tag])
        for pm in ("constant", "reflect"):
            key = "mel_%s%s" % (pm, tag)
            if key not in g.files:
                assert pm == "reflect" and x.shape[1] < 257
            else:
                assert g[key].shape == (x.shape[0], 1 + x.shape[1] // 128, 128)
    worst = so.baseline_errors(g)
    print("fp64 oracle vs fp32 fixture, worst per-frame relative error: %s" % worst)
    assert all(0 < v <= ORACLE_BOUND for v in worst.values()), worst
    # silence: every bin and band exactly zero
    assert not g["stft_sil"].any() and not g["mel_constant_sil"].any() and not g["mel_reflect_sil"].any()


def test_mel_filterbank_shape_of_the_formulas():
    fb = so.mel_filterbank()
    first, cnt = so.banded(fb)
    assert fb.shape == (128, 257) and (fb >= 0).all()
    assert cnt.min() >= 1 and cnt.max() == 12 and not fb[:, 256].any()
    assert (np.diff(first) >= 0).all() and first[0] == 1
    # Slaney normalisation: each triangle has unit area in Hz (sampled every 31.25 Hz: within the sampling error)
    np.testing.assert_allclose(so.mel_to_hz(so.hz_to_mel(8000.0)), 8000.0, rtol=1e-12)
    np.testing.assert_allclose(so.hz_to_mel(1000.0), 15.0)


@pytest.fixture(scope="module")
def lib():
    from asvspoof2021_air_amd import _hip, build
    build.build(verbose=False)
    return _hip.lib()


def _plan(lib, kind):
    from asvspoof2021_air_amd import _hip
    n = lib.air_spec_plan_bytes()
    assert n == 4 * (8 + 512 + 512 + 32 + 128 + 128 + 12 * 128)  # the layout include/air_hip.h documents
    plan = torch.zeros(n, dtype=torch.uint8)
    assert lib.air_spec_plan_build(ctypes.c_int(kind), _hip.hptr(plan, torch.uint8)) == 0
    i32, f32 = plan.view(torch.int32).numpy(), plan.view(torch.float32).numpy()
    return {"hdr": i32[:8], "window": f32[8:520], "lo": i32[1064:1192], "cnt": i32[1192:1320],
            "fbw": f32[1320:1320 + 12 * 128].reshape(12, 128)}


def test_symbols_declared_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "air_hip.h")).read()
    for name in ("air_spec_plan_bytes", "air_spec_plan_build", "air_spec_out_dim", "air_spec_fwd", "air_spec_fwd_ragged"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
    for macro in ("AIR_SPEC_STFT 1", "AIR_SPEC_MEL 2", "AIR_SPEC_EMPHASIS 1", "AIR_SPEC_REFLECT 2"):
        assert "#define " + macro in text
    assert lib.air_spec_plan_bytes.restype is ctypes.c_size_t
    assert (lib.air_spec_out_dim(1), lib.air_spec_out_dim(2), lib.air_spec_out_dim(3)) == (257, 128, -1)


def test_plan_builder_windows_and_mel_table(lib):
    from asvspoof2021_air_amd import _hip
    st, mel = _plan(lib, 1), _plan(lib, 2)
    assert list(st["hdr"][:5]) == [1, 257, 160, 320, 257] and list(mel["hdr"][:6]) == [2, 128, 128, 512, 257, 12]
    np.testing.assert_allclose(st["window"][:320], so.hamming_periodic(320), rtol=0, atol=1e-7)
    assert not st["window"][320:].any() and not st["fbw"].any()
    np.testing.assert_allclose(mel["window"], so.hann_periodic(512), rtol=0, atol=1e-7)
    # (torch.hamming_window / hann_window evaluate the same closed forms in fp32 and sit up to 1.5e-7 off them)
    np.testing.assert_allclose(st["window"][:320], torch.hamming_window(320).numpy(), rtol=0, atol=3e-7)
    np.testing.assert_allclose(mel["window"], torch.hann_window(512).numpy(), rtol=0, atol=3e-7)
    fb = so.mel_filterbank()
    first, cnt = so.banded(fb)
    assert np.array_equal(mel["lo"], first) and np.array_equal(mel["cnt"], cnt)
    for j in range(128):
        np.testing.assert_allclose(mel["fbw"][:cnt[j], j], fb[j, first[j]:first[j] + cnt[j]], rtol=1e-7, atol=0)
        assert not mel["fbw"][cnt[j]:, j].any()
    # bad arguments are reported, not crashed on
    plan = torch.zeros(lib.air_spec_plan_bytes(), dtype=torch.uint8)
    assert lib.air_spec_plan_build(ctypes.c_int(3), _hip.hptr(plan, torch.uint8)) == -2
    assert lib.air_spec_plan_build(ctypes.c_int(1), None) == -1


def test_entry_points_check_their_arguments_before_any_launch(lib):
    """Host-side refusals need no GPU: null pointers, sizes, the kinds and pad modes this build has."""
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    assert lib.air_spec_fwd(1, null, null, 1, 160, one, one, 0, null) == -1      # neither fp32 nor int16 PCM
    assert lib.air_spec_fwd(1, one, one, 1, 160, one, one, 0, null) == -1        # both
    assert lib.air_spec_fwd(1, one, null, 1, 0, one, one, 0, null) == -1
    assert lib.air_spec_fwd(7, one, null, 1, 160, one, one, 0, null) == -2
    assert lib.air_spec_fwd_ragged(1, one, null, 1, 160, null, one, 0, null, one, 0, 0, null) == -1   # feat_len 0
    assert lib.air_spec_fwd_ragged(1, one, null, 1, 160, null, one, 8, null, one, 0, 2, null) == -2   # AIR_PAD_SILENCE
    assert lib.air_spec_fwd_ragged(2, one, null, 1, 160, null, one, 8, null, one, 0, 2, null) == -2
    assert lib.air_spec_fwd_ragged(1, one, null, 1, 160, null, one, 8, null, one, 0, 3, null) == -1
    assert lib.air_spec_fwd_ragged(9, one, null, 1, 160, null, one, 8, null, one, 0, 0, null) == -2
