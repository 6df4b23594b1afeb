"""Oracle (test infrastructure): the reference's STFT and Melspec front-ends stated in numpy, fp64 by default.

* ``stft_power`` ..... STFT.forward, feature_extraction.py:154-165: pre-emphasis (:157), torch.stft(x, 512, 160, 320,
  hamming_window(320), onesided, pad_mode="constant") (:159-161), norm(., 2, -1).pow(2) permuted to (B, T, 257) (:163).
* ``mel_power`` ...... Melspec.forward, feature_extraction.py:174-176 = librosa.feature.melspectrogram(y, sr=16000,
  n_fft=512, hop_length=128): periodic Hann window of 512, centred frames (256 samples of ``pad_mode`` each side),
  |X|^2, then ``mel_filterbank`` - librosa.filters.mel(sr=16000, n_fft=512, n_mels=128, htk=False, norm="slaney").
  librosa is not available where these tests run: the formulas below define Melspec here, its parity with librosa
  itself is unpinned.

``dtype`` is the arithmetic width; float64 is the yardstick both the fp32 baselines of tests/golden/spectral.npz and the
HIP kernels are measured against (``frame_rel_err``)."""
import math

import numpy as np

N_FFT, N_MELS, SR = 512, 128, 16000
STFT_GEO = (320, 160, 512)   # fl, fs, fn: the only geometry the reference uses (preprocess.py:40)
MEL_HOP = 128


def hamming_periodic(fl=320, dtype=np.float64):
    """torch.hamming_window(fl) (periodic): feature_extraction.py:160."""
    n = np.arange(fl, dtype=np.float64)
    return (0.54 - 0.46 * np.cos(2.0 * np.pi * n / fl)).astype(dtype)


def hann_periodic(n_fft=N_FFT, dtype=np.float64):
    """scipy.signal.get_window("hann", n_fft, fftbins=True), librosa's default window."""
    n = np.arange(n_fft, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft)).astype(dtype)


# Slaney mel scale (librosa.hz_to_mel / mel_to_hz with htk=False): linear at 200/3 Hz per mel below 1 kHz, then
# logarithmic with logstep = ln(6.4) / 27.  Scalar math.log / math.exp: the libm the host plan builder calls.
_F_SP = 200.0 / 3.0
_LOGSTEP = math.log(6.4) / 27.0


def hz_to_mel(f):
    return 15.0 + math.log(f / 1000.0) / _LOGSTEP if f >= 1000.0 else f / _F_SP


def mel_to_hz(m):
    return 1000.0 * math.exp(_LOGSTEP * (m - 15.0)) if m >= 15.0 else _F_SP * m


def mel_filterbank():
    """(128, 257) fp64: w[i][k] = max(0, min(lower, upper)) * 2 / (mel_f[i+2] - mel_f[i]) with
    fftfreqs = linspace(0, 8000, 257) and mel_f = mel_to_hz(linspace(0, hz_to_mel(8000), 130))."""
    top = hz_to_mel(SR / 2.0)
    step = top / (N_MELS + 1)
    # numpy.linspace: arange(num) * step + start with the last point set to stop
    mel_f = np.array([mel_to_hz(top if i == N_MELS + 1 else i * step) for i in range(N_MELS + 2)])
    fftfreqs = np.arange(N_FFT // 2 + 1) * (SR / 2.0 / (N_FFT // 2))
    w = np.zeros((N_MELS, N_FFT // 2 + 1))
    for i in range(N_MELS):
        lower = (fftfreqs - mel_f[i]) / (mel_f[i + 1] - mel_f[i])
        upper = (mel_f[i + 2] - fftfreqs) / (mel_f[i + 2] - mel_f[i + 1])
        w[i] = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (mel_f[i + 2] - mel_f[i]))
    return w


def banded(w):
    """(first bin, count) of every filter's support."""
    first = np.array([int(np.nonzero(r)[0][0]) for r in w])
    last = np.array([int(np.nonzero(r)[0][-1]) for r in w])
    return first, last - first + 1


def _power(frames, dtype):
    spec = np.fft.rfft(frames.astype(np.float64) if dtype == np.float64 else frames, axis=-1)
    re, im = spec.real.astype(dtype), spec.imag.astype(dtype)
    return (re * re + im * im).astype(dtype)


def stft_power(x, with_emphasis=True, dtype=np.float64):
    """(B, L) -> (B, 1 + L // 160, 257).  ``x`` is not modified (the reference pre-emphasises it in place, :157: that
    side effect is oracle.lfcc.pre_emphasis_)."""
    fl, fs, fn = STFT_GEO
    work = np.array(x, dtype=dtype)
    if with_emphasis:
        work[:, 1:] = work[:, 1:] - dtype(0.97) * work[:, :-1].copy()
    B, L = work.shape
    T = 1 + L // fs
    padded = np.zeros((B, L + fn), dtype=dtype)  # center=True, pad_mode="constant"
    padded[:, fn // 2: fn // 2 + L] = work
    win = np.zeros(fn, dtype=dtype)
    off = (fn - fl) // 2  # torch.stft centres the short window in the frame
    win[off:off + fl] = hamming_periodic(fl, dtype)
    idx = (np.arange(T) * fs)[:, None] + np.arange(fn)[None, :]
    return _power(padded[:, idx] * win, dtype)


def mel_frames_power(x, pad_mode="reflect", dtype=np.float64):
    """(B, L) -> (B, 1 + L // 128, 257): the power spectrogram under the mel filterbank."""
    work = np.array(x, dtype=dtype)
    B, L = work.shape
    if pad_mode == "reflect":
        if L < N_FFT // 2 + 1:
            raise ValueError("reflect padding of %d needs at least %d samples" % (N_FFT // 2, N_FFT // 2 + 1))
        padded = np.pad(work, ((0, 0), (N_FFT // 2, N_FFT // 2)), mode="reflect")
    elif pad_mode == "constant":
        padded = np.pad(work, ((0, 0), (N_FFT // 2, N_FFT // 2)), mode="constant")
    else:
        raise ValueError(pad_mode)
    T = 1 + L // MEL_HOP
    idx = (np.arange(T) * MEL_HOP)[:, None] + np.arange(N_FFT)[None, :]
    return _power(padded[:, idx] * hann_periodic(N_FFT, dtype), dtype)


def mel_power(x, pad_mode="reflect", dtype=np.float64, fb=None):
    """(B, L) -> (B, 1 + L // 128, 128), frame-major (the reference returns (128, T) of x[0])."""
    fb = mel_filterbank() if fb is None else fb
    return (mel_frames_power(x, pad_mode, dtype) @ fb.astype(dtype).T).astype(dtype)


def frame_rel_err(y, y64):
    """The error measure of a power-domain output: max |y - y64| / (that frame's largest fp64 value) over the frames
    (last axis = bins or bands); a frame whose fp64 values are all zero must be zero exactly (-> inf otherwise)."""
    y = np.asarray(y, dtype=np.float64)
    y64 = np.asarray(y64, dtype=np.float64)
    assert y.shape == y64.shape, (y.shape, y64.shape)
    if y.size == 0:
        return 0.0
    top = np.abs(y64).max(axis=-1)
    err = np.abs(y - y64).max(axis=-1)
    live = top > 0
    worst = float((err[live] / top[live]).max()) if live.any() else 0.0
    if (err[~live] != 0).any():
        return float("inf")
    return worst


# ---------------------------------------------------------------------------- the fixture (tests/golden/spectral.npz)
def golden_cases(g):
    """(tag, input tensor) of every case of spectral.npz: the seeded inputs regenerated from
    oracle.filler.synth_pcm and checked against their checksums, then the stored silence / impulse / sine inputs."""
    import torch
    from oracle.filler import synth_pcm
    out = []
    for ci in range(int(g["nshapes"])):
        B, L = (int(v) for v in g["shape%d" % ci])
        x = synth_pcm(B, L, seed=int(g["seed0"]) + ci)
        np.testing.assert_allclose([x.double().sum().item(), x.double().abs().sum().item()], g["xsum%d" % ci], rtol=1e-12)
        out.append(("%d" % ci, x))
    return out + [("_" + nm, torch.from_numpy(g["x_" + nm].copy())) for nm in ("sil", "imp", "sine")]


def baseline_errors(g):
    """e_ref per front-end: the worst ``frame_rel_err`` of the fixture's fp32 baselines (the reference's STFT on the CPU,
    the fp32 restatement of the mel spectrogram under either pad mode) against the fp64 oracle."""
    worst = {"stft": 0.0, "mel_constant": 0.0, "mel_reflect": 0.0}
    fb = mel_filterbank()
    for tag, x in golden_cases(g):
        xn = x.numpy()
        worst["stft"] = max(worst["stft"], frame_rel_err(g["stft" + tag], stft_power(xn)))
        for pm in ("constant", "reflect"):
            key = "mel_%s%s" % (pm, tag)
            if key in g.files:
                worst["mel_" + pm] = max(worst["mel_" + pm], frame_rel_err(g[key], mel_power(xn, pm, fb=fb)))
    return worst
