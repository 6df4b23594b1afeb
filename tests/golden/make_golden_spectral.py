#!/usr/bin/env python3
"""Generate tests/golden/spectral.npz: the fp32 baselines of the STFT and Melspec front-ends.

Runs only in the build container (needs /root/reference), under the shims of make_golden.py (a stub ``librosa``,
``torch.stft`` with ``return_complex=True``).

* STFT: the REAL reference class, ``feature_extraction.STFT(320, 160, 512, 16000)`` (feature_extraction.py:141-165), on
  the CPU: its output and the first 64 samples of the input it pre-emphasised in place.
* MEL: librosa is not installed here, so the reference's Melspec (a librosa call, :175) cannot run.  Stored instead: an
  fp32 CPU restatement of ``librosa.feature.melspectrogram(sr=16000, n_fft=512, hop_length=128)`` - ``torch.stft`` with
  the 512-point periodic Hann window, |X|^2, an fp32 product with the filterbank of tests/spectral_oracle.py - under
  both pad modes, and that filterbank in fp64.  Parity with librosa itself is unpinned.

Inputs are regenerated from ``oracle.filler.synth_pcm(B, L, seed=SEED0 + case)`` and guarded by a checksum; the silence,
impulse and sine inputs are those of lfcc.npz.  ``reflect`` needs 257 samples: shorter cases have no ``mel_reflect``.
While generating, the fp64 oracle is measured against every baseline with the error measure of the tests.

Usage:  python tests/golden/make_golden_spectral.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import numpy as np
import torch

from make_golden import install_shims, save

SHAPES = [(1, 1), (1, 159), (2, 161), (2, 4481), (3, 9599)]
SEED0 = 700


def structured():
    L = 8000
    sil = torch.zeros(1, L)
    imp = torch.zeros(1, L)
    imp[0, 1234] = 1.0
    sine = (0.5 * torch.sin(2 * np.pi * 1000.0 * torch.arange(L) / 16000.0)).reshape(1, L).float()
    return (("sil", sil), ("imp", imp), ("sine", sine))


def mel32(x, pad_mode, fb32, raw_stft):
    spec = raw_stft(x, 512, 128, 512, window=torch.hann_window(512), center=True, pad_mode=pad_mode, onesided=True,
                    return_complex=True)
    power = spec.real ** 2 + spec.imag ** 2        # (B, 257, T) fp32
    return torch.matmul(power.permute(0, 2, 1).contiguous(), fb32.t()).contiguous()  # (B, T, 128)


def main():
    raw_stft = torch.stft
    install_shims()
    import feature_extraction as ref_fe  # noqa: E402
    import spectral_oracle as so
    from oracle.filler import synth_pcm

    torch.set_num_threads(8)
    ref = ref_fe.STFT(320, 160, 512, 16000)
    fb64 = so.mel_filterbank()
    fb32 = torch.from_numpy(fb64).float()
    first, cnt = so.banded(fb64)
    print("mel filterbank: widest %d bins, empty %d, Nyquist weight max %.3g" % (cnt.max(), int((cnt < 1).sum()),
                                                                                 fb64[:, 256].max()))
    out = {"mel_fb": fb64, "nshapes": len(SHAPES), "seed0": SEED0}
    cases = [("%d" % ci, synth_pcm(B, L, seed=SEED0 + ci)) for ci, (B, L) in enumerate(SHAPES)]
    worst = {"stft": 0.0, "constant": 0.0, "reflect": 0.0}
    for tag, xin in cases + [("_" + nm, sig) for nm, sig in structured()]:
        x = xin.clone()
        y = ref(x)  # mutates x
        e = so.frame_rel_err(y.numpy(), so.stft_power(xin.numpy()))
        worst["stft"] = max(worst["stft"], e)
        line = "  case %-5s %-10s stft fp32-vs-fp64 %.3g" % (tag, tuple(xin.shape), e)
        if tag[0] != "_":
            out["shape" + tag] = np.array(xin.shape)
            out["xsum" + tag] = np.array([xin.double().sum().item(), xin.double().abs().sum().item()])
        else:
            out["x" + tag] = xin
        out["stft" + tag] = y
        out["xmut" + tag] = x[:, :64].clone()
        for pm in ("constant", "reflect"):
            if pm == "reflect" and xin.shape[1] < 257:
                continue
            m = mel32(xin, pm, fb32, raw_stft)
            e = so.frame_rel_err(m.numpy(), so.mel_power(xin.numpy(), pm, fb=fb64))
            worst[pm] = max(worst[pm], e)
            line += "  mel/%s %.3g" % (pm, e)
            out["mel_%s%s" % (pm, tag)] = m
        print(line)
    print("worst fp32-vs-fp64: %s" % worst)
    save("spectral.npz", **out)


if __name__ == "__main__":
    main()
