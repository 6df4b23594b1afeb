"""The CQCC definition on the CPU: what the oracle (tests/cqcc_oracle.py) computes has the properties the header block
states, and the plan the library builds holds the oracle's tables."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cqcc_oracle as co


def test_sizes_at_the_defaults():
    assert co.n_bins() == 864 and co.n_lin() == 8118
    f = co.bin_freqs()
    assert f[0] == 8000.0 / 512 and abs(f[-1] - 8000.0 * 2.0 ** (-1 / 96)) < 1e-9
    assert [co.octave_of(k) for k in (0, 95, 96, 863)] == [8, 8, 7, 0]
    assert [co.level_of(o) for o in range(9)] == [0, 0, 1, 2, 3, 4, 5, 6, 7]
    top, rest = co.atom_lengths(4.0), co.atom_lengths(8.0)
    assert (top.min(), top.max(), rest.min(), rest.max()) == (277, 551, 555, 1103) and np.all(top % 2 == 1)
    # no bin's half-length sits near an integer boundary where two fp64 libraries could floor apart
    for ratio in (4.0, 8.0):
        v = co.q_factor() * ratio * 2.0 ** (-np.arange(96) / 96) / 2.0
        assert np.abs(v - np.round(v)).min() > 1e-6


def test_low_pass_stopband_and_passband():
    """Measured: the stopband peaks at -152.9 dB; stated in the header block as below -150 dB.  The passband, to R/8
    plus one bin's bandwidth R / (8 Q), is flat to 3.5e-8."""
    h = co.fir()
    assert len(h) == 47 and abs(h.sum() - 1.0) < 1e-15 and np.array_equal(h, h[::-1])
    stop = co.fir_response(np.linspace(0.375, 0.5, 4001)).max()
    assert 20 * math.log10(stop) < -150.0
    assert stop < 2.0 ** -24  # below fp32 roundoff of a full-scale input
    edge = 0.125 * (1.0 + 1.0 / co.q_factor())
    assert np.abs(co.fir_response(np.linspace(0.0, edge, 2001)) - 1.0).max() < 1e-7


@pytest.mark.parametrize("octave", [0, 1, 2, 8])
def test_a_tone_at_a_bin_centre_gives_half_its_amplitude(octave):
    """|X| = A / 2 up to the image term: the negative-frequency half of the cosine, A / 2 times the normalised window's
    own transform 2 f / R away, plus (decimated levels) the low-pass's passband error per level."""
    A, L = 0.7, 1 << 18
    k = (8 - octave) * 96 + 37
    f = co.bin_freqs()[k]
    x = A * np.cos(2 * np.pi * f * np.arange(L) / 16000.0 + 0.3)
    t = np.array([L // 320])  # the middle frame: every atom and every level's filter lie inside the tone
    X = co.transform(x, frames=t)[0]
    s = co.level_of(octave)
    R = 16000.0 / 2 ** s
    N = co.atom_lengths(4.0 if octave == 0 else 8.0)[37]
    w = np.hanning(N) / np.hanning(N).sum()
    image = abs(np.sum(w * np.exp(-2j * np.pi * (2 * f / R) * np.arange(N))))
    assert image < 1e-4
    assert abs(abs(X[k]) - A / 2) <= (A / 2) * (image + s * 1e-7 + 1e-12)
    # and the bin is where the energy is: two bins away the window has let go
    assert abs(X[k]) > 30 * abs(X[k + 3 if k + 3 < 864 else k - 3])


def test_fused_projection_is_interpolation_then_dct():
    rng = np.random.RandomState(5)
    S = rng.randn(864, 3)
    W = co.interp_matrix()
    assert W.shape == (8118, 864) and np.allclose(W.sum(axis=1), 1.0) and W.min() >= 0.0
    v = W @ S
    # row m of W reads S at 96 log2(1 + m / 16): check it against numpy's own interpolation
    pos = 96 * np.log2(1.0 + np.arange(8118) / 16.0)
    for c in range(3):
        assert np.allclose(v[:, c], np.interp(pos, np.arange(864), S[:, c]), atol=1e-12)
    try:
        from scipy.fft import dct
        c_ref = dct(v, type=2, norm="ortho", axis=0)[:20]
    except ImportError:
        m = np.arange(8118)
        c_ref = np.stack([math.sqrt((1.0 if q == 0 else 2.0) / 8118) * (np.cos(np.pi * (m + 0.5) * q / 8118) @ v)
                          for q in range(20)])
    assert np.abs(co.projection() @ S - c_ref).max() < 1e-11


def test_deltas_are_the_lfcc_front_ends():
    from asvspoof2021_air_amd.feature_extraction import delta
    c = np.random.RandomState(6).randn(7, 20)
    ref = delta(torch.from_numpy(c)[None])[0].numpy()
    assert np.array_equal(co.delta(c), ref)
    one = np.random.RandomState(7).randn(1, 20)
    assert np.array_equal(co.delta(one), np.zeros((1, 20)))
    x = co.make_signal(1, 800, 3, n_octaves=2)[0].astype(np.float64)
    full = co.cqcc(x, n_octaves=2)
    assert full.shape == (6, 60)
    assert np.array_equal(full[:, 20:40], co.delta(full[:, :20])) and np.array_equal(full[:, 40:], co.delta(full[:, 20:40]))


def test_the_plan_holds_the_oracles_tables():
    """The library's plan builder (fp64 on the host, rounded once) against the oracle, entry by entry."""
    from asvspoof2021_air_amd import _hip
    lib = _hip.lib()
    host = torch.zeros(lib.air_cqcc_plan_bytes(), dtype=torch.uint8)
    assert lib.air_cqcc_plan_build(96, 9, 160, 20, 16, ctypes.c_double(2.0 ** -52), ctypes.c_void_p(host.data_ptr())) == 0
    ints = host[:48].view(torch.int32).numpy()
    assert list(ints[1:10]) == [9, 160, 20, 864, 47, 275, 551, 16, 8118]
    fl = host.numpy().view(np.float32)
    assert fl[12] == np.float32(2.0 ** -52)
    u = 2.0 ** -24
    h = co.fir()
    assert np.all(np.abs(fl[16:63] - h) <= u * np.abs(h) + 1e-30) and not fl[63:80].any()
    P = co.projection()
    got = fl[80:80 + 20 * 864].reshape(20, 864)
    assert np.all(np.abs(got - P) <= u * np.abs(P) + 1e-18)
    off = 80 + 32 * 864
    bins = np.arange(96)
    cre = (bins >> 4) * 32 + (bins & 15)
    for rows, ratio in ((576, 4.0), (1120, 8.0)):
        tab = fl[off:off + rows * 192].reshape(rows, 192)
        off += rows * 192
        ref, H = co.atom_table(ratio)
        assert np.all(np.abs(tab[:2 * H + 1, cre] - ref.real) <= u * np.abs(ref.real) + 1e-18)
        assert np.all(np.abs(tab[:2 * H + 1, cre + 16] - ref.imag) <= u * np.abs(ref.imag) + 1e-18)
        assert not tab[2 * H + 1:].any()
    assert off * 4 == lib.air_cqcc_plan_bytes()
    assert lib.air_cqcc_plan_build(48, 9, 160, 20, 16, ctypes.c_double(2.0 ** -52), ctypes.c_void_p(host.data_ptr())) == -2
    assert lib.air_cqcc_n_bins(96, 9) == 864
    # the workspace is a function of (B, Lcap) and the geometry: levels 1 .. 7, the log spectrum, the statics
    levels = sum(-(-64000 // 2 ** s) for s in range(1, 8))
    assert lib.air_cqcc_ws_bytes(64, 64000, 9, 160, 20) == 4 * (64 * levels + 64 * 401 * 864 + 64 * 401 * 20)


def test_the_noise_floor_the_gpu_bounds_assume():
    """The GPU tests propagate their power bound through the logarithm, which needs it below the power itself: on
    the inputs they use the bound stays under half of every |X|^2 + eps (cqcc_oracle.reference asserts the same for
    each of its cases; this is the cheapest one)."""
    ref = co.reference(2)
    assert (ref["tolP"] / ref["P"]).max() < 0.5 and ref["P"].min() > 1e4 * co.EPS


def test_front_end_surface_without_a_gpu():
    import asvspoof2021_air_amd as pkg
    from asvspoof2021_air_amd.feature_extraction import CQCC
    fe = pkg.CQCC()
    assert isinstance(fe, CQCC) and fe.out_dim == 60 and fe.fs == 160 and fe.n_bins == 864
    assert CQCC(n_octaves=3, n_coef=12).out_dim == 36
    with pytest.raises(NotImplementedError):
        CQCC(bins_per_octave=48)
    with pytest.raises(ValueError):
        fe.forward_padded(torch.zeros(1, 800), 8, padding="silence")
    with pytest.raises(ValueError):
        fe.forward_padded(torch.zeros(1, 800), 8, padding="mirror")
