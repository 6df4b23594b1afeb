"""Drop-ins for the reference's front-ends: ``LFCC`` (feature_extraction.py:61-138) on the kernel of csrc/lfcc.hip,
``STFT`` (:141-165) and ``Melspec`` (:168-176) on the kernels of csrc/spectral.hip.  What the three share on the host -
plan cache, input checks, output allocation, the padded / ragged call - is ``_FrontEnd``.

``LFCC``: same constructor, same ``forward(x:(B,L)) -> (B, 1+L//fs, 3*filter_num)``,
same ``state_dict`` keys (``lfcc_fb``, ``l_dct.weight``), same in-place
pre-emphasis of the caller's tensor (:106).  The device work is ONE fused HIP
kernel reached through ``air_lfcc_fwd``.
"""
import math

import torch
import torch.nn as nn

from . import _hip
from .ragged import device_lengths, pcm_pointers


def trimf(x, params):
    """Triangular membership (feature_extraction.py:16-39): strict inequalities on
    both slopes, exactly 1 at x == b."""
    if len(params) != 3:
        raise ValueError("trimf requires params to be a list of 3 elements")
    a, b, c = params
    if a > b or b > c:
        raise ValueError("trimf(x, [a, b, c]) requires a<=b<=c")
    y = torch.zeros_like(x, dtype=torch.float32)
    if a < b:
        up = (a < x) & (x < b)
        y[up] = (x[up] - a) / (b - a)
    if b < c:
        down = (b < x) & (x < c)
        y[down] = (c - x[down]) / (c - b)
    y[x == b] = 1
    return y


def dct_ortho(x):
    """Orthonormal DCT-II over the last dim via an FFT of the even/odd-reordered
    signal (the algorithm of utils_dsp.py:147-176, on torch.fft)."""
    n = x.shape[-1]
    flat = x.contiguous().view(-1, n)
    v = torch.cat([flat[:, ::2], flat[:, 1::2].flip([1])], dim=1)
    vc = torch.view_as_real(torch.fft.fft(v))
    k = -torch.arange(n, dtype=x.dtype)[None, :] * math.pi / (2 * n)
    out = vc[:, :, 0] * torch.cos(k) - vc[:, :, 1] * torch.sin(k)
    out[:, 0] /= math.sqrt(n) * 2
    out[:, 1:] /= math.sqrt(n / 2) * 2
    return 2 * out.view(*x.shape)


class LinearDCT(nn.Linear):
    """DCT as a frozen linear layer (utils_dsp.py:220-244); only type 'dct' is on the path."""

    def __init__(self, in_features, type, norm=None, bias=False):
        if type != "dct" or norm != "ortho":
            raise NotImplementedError("only LinearDCT(n, 'dct', norm='ortho') is on the hot path")
        self.type, self.N, self.norm = type, in_features, norm
        super().__init__(in_features, in_features, bias=bias)

    def reset_parameters(self):
        self.weight.data = dct_ortho(torch.eye(self.N)).data.t().contiguous()
        self.weight.requires_grad = False


def delta(x):
    """feature_extraction.py:41-58 on the host (kept for API parity; the kernel fuses it)."""
    xp = torch.cat((x[:, :1], x, x[:, -1:]), 1)
    return xp[:, 2:] - xp[:, :-2]


PAD_MODES = {"repeat": 0, "zero": 1, "silence": 2}


def pad_mode_id(padding):
    """--padding choice -> AIR_PAD_* (include/air_hip.h); the reference's error for anything else (dataset.py:79)."""
    if padding not in PAD_MODES:
        raise ValueError("Padding should be zero or repeat!")
    return PAD_MODES[padding]


def _pcm_source(x):
    """What the kernels read ``x`` as: int16 PCM or float32, contiguous; any other dtype is converted with ``.float()``."""
    if x.dtype in (torch.int16, torch.float32):
        return x.contiguous()
    return x.float().contiguous()


def preemph_inplace_(x):
    """x[:, 1:] -= 0.97 * x[:, :-1] on the original samples, in place (feature_extraction.py:106, :157)."""
    lib = _hip.lib()
    B, L = x.shape
    nbytes = lib.air_preemph_ws_bytes(_hip.ci(B), _hip.ci(L))
    ws = torch.empty(max(1, nbytes // 4), device=x.device, dtype=torch.float32)
    _hip.check(lib.air_preemph_inplace(_hip.dptr(x), _hip.ci(B), _hip.ci(L), _hip.cf(0.97),
                                       _hip.dptr(ws), _hip.csz(nbytes), _hip.stream()),
               "air_preemph_inplace")


class _FrontEnd(nn.Module):
    """What the three PCM front-ends share on the host: the cached plan blob, the input checks, the ``start`` upload, the
    output allocation around the dense and the padded / ragged call, and the reference's in-place pre-emphasis of the
    caller's tensor.  A subclass supplies ``NAME``, ``out_dim``, ``fs`` (the hop), ``_flags()``, its plan
    (``_plan_id`` / ``_plan_build``), its C entry points (``_call_dense`` / ``_call_padded``) and ``_check``."""
    NAME = "?"

    def __init__(self):
        super().__init__()
        self._plan = None
        self._plan_key = None

    def _plan_id(self, device):
        """What the cached plan depends on."""
        return str(device)

    def plan(self, device):
        """Device-resident plan blob (window, twiddles, filterbank; LFCC: DCT)."""
        key = self._plan_id(device)
        if self._plan is None or self._plan_key != key:
            self._plan = self._plan_build(_hip.lib()).to(device)
            self._plan_key = key
        return self._plan

    def _check_x(self, x):
        if x.dim() != 2:
            raise ValueError("%s expects (batch, length), got %s" % (self.NAME, tuple(x.shape)))
        if not x.is_cuda:
            raise _hip.AirError("%s HIP path needs a GPU tensor; there is no CPU fallback" % self.NAME)

    def _check_lengths(self, host, Lcap):
        """Host-side lengths beyond the [1, Lcap] check of ``ragged.device_lengths``."""

    def _dense(self, x):
        """(B, L) float32 or int16 on the GPU -> ((B, T, out_dim), the tensor the kernel read).  Does not mutate ``x``."""
        B, L = x.shape
        self._check_lengths(torch.tensor([L]), L)
        src = _pcm_source(x)
        out = torch.empty((B, 1 + L // self.fs, self.out_dim), device=x.device, dtype=torch.float32)
        self._call_dense(_hip.lib(), src, _hip.ci(B), _hip.ci(L), _hip.dptr(out),
                         _hip.dptr(self.plan(x.device), torch.uint8), _hip.ci(self._flags()))
        return out, src

    def _emphasise(self, x, src):
        """The reference emphasises the caller's tensor in place; the kernel read the original samples, so this follows
        it.  (Integers: nothing to mutate - the reference never sees them.)"""
        if self.with_emphasis and self.mutate_input and x.dtype != torch.int16:
            preemph_inplace_(src)
            if src is not x:
                x.copy_(src)

    def _padded(self, x, lengths, feat_len, start, mode):
        B, Lcap = x.shape
        if start is not None and not (torch.is_tensor(start) and start.is_cuda):
            start = torch.as_tensor(start, dtype=torch.int32).to(x.device)
        src = _pcm_source(x)
        out = torch.empty((B, self.out_dim, feat_len), device=x.device, dtype=torch.float32)
        # (pcm, pcm16, B, L), the row lengths or None, (out, feat_len, start, plan, flags, pad_mode)
        self._call_padded(_hip.lib(), (*pcm_pointers(src), _hip.ci(B), _hip.ci(Lcap)), lengths,
                          (_hip.dptr(out), _hip.ci(feat_len), _hip.dptr(start, torch.int32, True),
                           _hip.dptr(self.plan(x.device), torch.uint8), _hip.ci(self._flags()), _hip.ci(mode)),
                          mode, x.device)
        return out

    def forward_padded(self, x, feat_len=750, start=None, padding="repeat"):
        """Fused front-end -> pad / chop -> transpose: (B, L) -> (B, out_dim, feat_len), i.e. what dataset.py:62-79 +
        main_train.py:338 build on the host.  Does not mutate ``x``.  ``start``: optional int32 (B,) crop offsets for
        T > feat_len.  ``padding``: the reference's ``--padding`` choices 'repeat' | 'zero' | 'silence'
        (main_train.py:45; 'silence' is LFCC's alone, NotImplementedError elsewhere); anything else raises ValueError
        like dataset.py:79."""
        mode = self._check(x, padding)
        self._check_lengths(torch.tensor([x.shape[1]]), x.shape[1])
        return self._padded(x, None, feat_len, start, mode)

    def forward_ragged(self, x, lengths, feat_len=750, start=None, padding="repeat"):
        """A batch of utterances of DIFFERENT lengths in one launch: ``x`` (B, Lcap) float32 or int16 on the GPU, row b
        holding ``lengths[b]`` samples (what follows them is never read) -> (B, out_dim, feat_len), row b being what
        ``forward_padded`` gives for that utterance alone.  Does not mutate ``x``.  ``lengths``: int32 (B,); a GPU tensor is
        used as is (the kernel clamps it to [1, Lcap]), a host tensor or list is checked (ValueError) and uploaded.
        ``start`` / ``padding``: as in ``forward_padded``, each row's offset clamped to its own [0, T_b - feat_len]."""
        mode = self._check(x, padding)
        B, Lcap = x.shape
        lengths = device_lengths(lengths, B, Lcap, x.device, extra_check=self._check_lengths)
        return self._padded(x, lengths, feat_len, start, mode)


class LFCC(_FrontEnd):
    """LFCC(fl, fs, fn, sr, filter_num, with_energy=False, with_emphasis=True, with_delta=True)."""
    NAME = "LFCC"

    def __init__(self, fl, fs, fn, sr, filter_num, with_energy=False, with_emphasis=True,
                 with_delta=True):
        super().__init__()
        self.fl, self.fs, self.fn, self.sr, self.filter_num = fl, fs, fn, sr, filter_num
        f = (sr / 2) * torch.linspace(0, 1, fn // 2 + 1)
        bands = torch.linspace(min(f), max(f), filter_num + 2)
        fb = torch.zeros([fn // 2 + 1, filter_num])
        for idx in range(filter_num):
            fb[:, idx] = trimf(f, [bands[idx], bands[idx + 1], bands[idx + 2]])
        self.lfcc_fb = nn.Parameter(fb, requires_grad=False)
        self.l_dct = LinearDCT(filter_num, "dct", norm="ortho")
        self.with_energy = with_energy
        self.with_emphasis = with_emphasis
        self.with_delta = with_delta
        self.mutate_input = True  # reference behaviour (feature_extraction.py:106)

    @property
    def out_dim(self):
        return self.filter_num * (3 if self.with_delta else 1)

    def _flags(self):
        return (1 if self.with_emphasis else 0) | (2 if self.with_delta else 0)

    def _plan_id(self, device):
        return (str(device), self.lfcc_fb._version, self.l_dct.weight._version,
                self.lfcc_fb.data_ptr(), self.l_dct.weight.data_ptr())

    def _plan_build(self, lib):
        host = torch.zeros(lib.air_lfcc_plan_bytes(), dtype=torch.uint8)
        fb = self.lfcc_fb.detach().float().cpu().contiguous()
        dct = self.l_dct.weight.detach().float().cpu().contiguous()
        win = torch.hamming_window(self.fl).contiguous()
        _hip.check(lib.air_lfcc_plan_build(_hip.hptr(fb), _hip.ci(fb.shape[0]), _hip.ci(fb.shape[1]),
                                           _hip.hptr(dct), _hip.hptr(win), _hip.ci(self.fl),
                                           _hip.ci(self.fs), _hip.ci(self.fn),
                                           _hip.hptr(host, torch.uint8)), "air_lfcc_plan_build")
        return host

    def _check(self, x, padding="repeat"):
        if self.with_energy:
            raise NotImplementedError("with_energy=True is not on the hot path (dead branch, "
                                      "feature_extraction.py:123-127)")
        self._check_x(x)
        return pad_mode_id(padding)

    def _call_dense(self, lib, src, B, L, out, plan, flags):
        if src.dtype == torch.int16:  # 16-bit PCM straight from the wav/flac samples (x = s / 32768 inside the kernel)
            no_start = _hip.dptr(None, torch.int32, True)  # (feat_len 0: the (B, T, D) layout of air_lfcc_fwd)
            _hip.check(lib.air_lfcc_fwd_padded_i16(_hip.dptr(src, torch.int16), B, L, out, _hip.ci(0), no_start, plan, flags,
                                                   _hip.stream()), "air_lfcc_fwd_padded_i16")
        else:
            _hip.check(lib.air_lfcc_fwd(_hip.dptr(src), B, L, out, plan, flags, _hip.stream()), "air_lfcc_fwd")

    def _call_padded(self, lib, rows, lengths, tail, mode, device):
        sil = _hip.dptr(self.silence_row(device) if mode == 2 else None, allow_none=True)
        if lengths is None:
            _hip.check(lib.air_lfcc_fwd_padded_ex(*rows, *tail, sil, _hip.stream()), "air_lfcc_fwd_padded_ex")
        else:
            _hip.check(lib.air_lfcc_fwd_ragged(*rows, _hip.dptr(lengths, torch.int32), *tail, sil, _hip.stream()),
                       "air_lfcc_fwd_ragged")

    def forward(self, x):
        self._check(x)
        out, src = self._dense(x)
        self._emphasise(x, src)
        return out

    def silence_row(self, device):
        """The frame the reference prepends under ``--padding silence``: frame 0 of the LFCC of 3200 zero
        samples (dataset.py:13-16), computed once per device by this module's own kernel."""
        key = (str(device), self._plan_key)
        if getattr(self, "_silence", None) is None or self._silence_key != key:
            mut, self.mutate_input = self.mutate_input, False
            try:
                row = self.forward(torch.zeros(1, 3200, device=device))[0, 0].contiguous()
            finally:
                self.mutate_input = mut
            self._silence, self._silence_key = row, (str(device), self._plan_key)
        return self._silence


class _Spectral(_FrontEnd):
    """The two spectrogram front-ends (csrc/spectral.hip, ``air_spec_*``).  ``KIND`` / ``out_dim`` / ``fs`` (the hop) /
    ``NAME`` come from the subclass."""
    KIND = 0

    def _flags(self):
        return 0

    def _plan_build(self, lib):
        host = torch.zeros(lib.air_spec_plan_bytes(), dtype=torch.uint8)
        _hip.check(lib.air_spec_plan_build(_hip.ci(self.KIND), _hip.hptr(host, torch.uint8)), "air_spec_plan_build")
        return host

    def _check(self, x, padding="repeat"):
        mode = pad_mode_id(padding)
        if mode == 2:
            raise NotImplementedError("padding='silence' prepends an LFCC frame (dataset.py:13-16) and is served by LFCC "
                                      "only; %s pads with 'repeat' or 'zero'" % self.NAME)
        self._check_x(x)
        return mode

    def _call_dense(self, lib, src, B, L, out, plan, flags):
        _hip.check(lib.air_spec_fwd(_hip.ci(self.KIND), *pcm_pointers(src), B, L, out, plan, flags, _hip.stream()),
                   "air_spec_fwd")

    def _call_padded(self, lib, rows, lengths, tail, mode, device):
        _hip.check(lib.air_spec_fwd_ragged(_hip.ci(self.KIND), *rows, _hip.dptr(lengths, torch.int32, True), *tail,
                                           _hip.stream()), "air_spec_fwd_ragged")


class STFT(_Spectral):
    """STFT(fl, fs, fn, sr, with_emphasis=True): drop-in for the reference's power spectrogram
    (feature_extraction.py:141-165).  ``forward(x:(B, L)) -> (B, 1 + L // fs, fn // 2 + 1)``, |X|^2 without a log, with the
    reference's in-place pre-emphasis of the caller's tensor (:157) unless ``mutate_input`` is False.  One fused HIP
    kernel (csrc/spectral.hip); only the geometry the reference uses, (320, 160, 512) (preprocess.py:40), is built."""
    KIND, NAME = 1, "STFT"

    def __init__(self, fl, fs, fn, sr, with_emphasis=True):
        super().__init__()
        if (fl, fs, fn) != (320, 160, 512):
            raise NotImplementedError("STFT is built for (fl, fs, fn) = (320, 160, 512) only (preprocess.py:40), got %s"
                                      % ((fl, fs, fn),))
        self.fl, self.fs, self.fn, self.sr = fl, fs, fn, sr
        self.with_emphasis = with_emphasis
        self.mutate_input = True  # reference behaviour (feature_extraction.py:157)

    @property
    def out_dim(self):
        return self.fn // 2 + 1

    def _flags(self):
        return 1 if self.with_emphasis else 0

    def forward(self, x):
        self._check(x)
        out, src = self._dense(x)
        self._emphasise(x, src)
        return out


class Melspec(_Spectral):
    """Melspec(): the reference's mel spectrogram (feature_extraction.py:168-176), i.e.
    ``librosa.feature.melspectrogram(y, sr=16000, n_fft=512, hop_length=128)``: 128 Slaney bands of the power
    spectrogram, no log.  ``forward(x)`` reads ``x[0]`` only and returns (128, T) like the reference (:175-176);
    ``forward_batch(x)`` returns (B, 128, T).  ``pad_mode``: 'reflect' (librosa's default when the reference was
    written) or 'constant' (its default since 0.10).  Defined by the formulas in csrc/spectral.hip; parity with librosa
    itself is not pinned."""
    KIND, NAME = 2, "Melspec"
    fs = 128       # hop
    out_dim = 128

    def __init__(self, pad_mode="reflect"):
        super().__init__()
        if pad_mode not in ("reflect", "constant"):
            raise ValueError("pad_mode must be 'reflect' or 'constant', got %r" % (pad_mode,))
        self.pad_mode = pad_mode

    def _flags(self):
        return 2 if self.pad_mode == "reflect" else 0

    def _check_lengths(self, host, Lcap):
        if self.pad_mode == "reflect" and host.numel() and int(host.min()) < 257:
            raise ValueError("pad_mode='reflect' reflects 256 samples at either end and needs utterances of at least 257 "
                             "samples (numpy raises too), got %d; use pad_mode='constant'" % int(host.min()))

    def forward_frames(self, x):
        """(B, L) -> (B, T, 128): the frame-major layout of ``LFCC.forward`` / ``STFT.forward``."""
        self._check(x)
        return self._dense(x)[0]

    def forward_batch(self, x):
        """(B, L) -> (B, 128, T), written in that layout by the kernel (``forward_padded`` at feat_len = T)."""
        self._check(x)
        return self.forward_padded(x, 1 + x.shape[1] // self.fs)

    def forward(self, x):
        return self.forward_batch(x[:1])[0]


class CQCC(_FrontEnd):
    """CQCC(sr=16000, bins_per_octave=96, n_octaves=9, hop=160, n_coef=20, d=16, eps=2**-52): constant-Q cepstral
    coefficients, the reference's second feature (``--feat CQCC``), on the kernels of csrc/cqcc.hip.  The reference
    ships no CQCC code: the feature is defined by the formulas of include/air_hip.h ("CQCC front-end") and pinned by a
    numpy fp64 oracle; parity with the challenge's MATLAB toolbox is not claimed ("CQCC").

    ``forward(x:(B, L)) -> (B, 1 + L // hop, 3 * n_coef)``, columns [static, delta, delta-delta] - the shape ``LFCC``
    feeds to the models and the GMMs; ``forward_padded`` / ``forward_ragged`` as in the other front-ends ('repeat' and
    'zero' padding; 'silence' is LFCC's and raises ValueError); ``forward_spectrum`` returns the (B, T, K) log power
    the cepstra are projected from.  fp32 or int16 PCM; ``x`` is never modified.  Built: 96 bins per octave, up to 9
    octaves, hop <= 160, n_coef <= 32."""
    NAME = "CQCC"
    with_emphasis = False
    mutate_input = False

    def __init__(self, sr=16000, bins_per_octave=96, n_octaves=9, hop=160, n_coef=20, d=16, eps=2.0 ** -52):
        super().__init__()
        if bins_per_octave != 96 or not 1 <= n_octaves <= 9 or not 1 <= hop <= 160 or not 1 <= n_coef <= 32:
            raise NotImplementedError("CQCC is built for 96 bins per octave, 1..9 octaves, hop <= 160 and n_coef <= 32, "
                                      "got %s" % ((bins_per_octave, n_octaves, hop, n_coef),))
        if d < 1 or eps < 0:
            raise ValueError("CQCC needs d >= 1 and eps >= 0")
        self.sr, self.bins_per_octave, self.n_octaves, self.n_coef, self.d, self.eps = (
            sr, bins_per_octave, n_octaves, n_coef, d, eps)
        self.fs = hop  # the hop, under the name the other front-ends give it

    @property
    def out_dim(self):
        return 3 * self.n_coef

    @property
    def n_bins(self):
        return self.bins_per_octave * self.n_octaves

    def _flags(self):
        return 0

    def _plan_id(self, device):
        return (str(device), self.n_octaves, self.fs, self.n_coef, self.d, self.eps)

    def _plan_build(self, lib):
        import ctypes
        host = torch.zeros(lib.air_cqcc_plan_bytes(), dtype=torch.uint8)
        _hip.check(lib.air_cqcc_plan_build(_hip.ci(self.bins_per_octave), _hip.ci(self.n_octaves), _hip.ci(self.fs),
                                           _hip.ci(self.n_coef), _hip.ci(self.d), ctypes.c_double(self.eps),
                                           _hip.hptr(host, torch.uint8)), "air_cqcc_plan_build")
        return host

    def _check(self, x, padding="repeat"):
        mode = pad_mode_id(padding)
        if mode == 2:
            raise ValueError("padding='silence' prepends an LFCC frame (dataset.py:13-16) and is served by LFCC only; "
                             "CQCC pads with 'repeat' or 'zero' (AIR_EUNSUPPORTED)")
        self._check_x(x)
        return mode

    def _geometry(self):
        return _hip.ci(self.n_octaves), _hip.ci(self.fs), _hip.ci(self.n_coef)

    def _workspace(self, lib, B, Lcap, device):
        """Scratch of one call (pyramid, log spectrum, statics): a function of (B, Lcap) only, taken from the stream's
        growing buffer like every other op's, so a captured step points into it."""
        from . import ops
        nbytes = lib.air_cqcc_ws_bytes(B, Lcap, *self._geometry())
        ws = ops.workspace(nbytes, device)
        return _hip.dptr(ws, torch.uint8), _hip.csz(nbytes)

    def _call_dense(self, lib, src, B, L, out, plan, flags):
        _hip.check(lib.air_cqcc_fwd(*pcm_pointers(src), B, L, out, plan, *self._geometry(),
                                    *self._workspace(lib, B, L, src.device), _hip.stream()), "air_cqcc_fwd")

    def _call_padded(self, lib, rows, lengths, tail, mode, device):
        out, feat_len, start, plan, _flags, pad = tail
        _hip.check(lib.air_cqcc_fwd_ragged(*rows, _hip.dptr(lengths, torch.int32, True), out, feat_len, start, plan,
                                           *self._geometry(), pad, *self._workspace(lib, rows[2], rows[3], device),
                                           _hip.stream()), "air_cqcc_fwd_ragged")

    def forward(self, x):
        self._check(x)
        return self._dense(x)[0]

    def forward_spectrum(self, x, lengths=None):
        """(B, L) -> (B, 1 + L // hop, K) log power S[k, t] = log(|X|^2 + eps), K = bins_per_octave * n_octaves, bin 0
        the lowest.  ``lengths``: the batch is ragged; frames at or behind a row's own count are zero."""
        self._check(x)
        B, Lcap = x.shape
        lib = _hip.lib()
        if lengths is not None:
            lengths = device_lengths(lengths, B, Lcap, x.device)
        src = _pcm_source(x)
        shape = (B, 1 + Lcap // self.fs, self.n_bins)
        out = (torch.empty if lengths is None else torch.zeros)(shape, device=x.device, dtype=torch.float32)
        _hip.check(lib.air_cqcc_spectrum(*pcm_pointers(src), _hip.ci(B), _hip.ci(Lcap),
                                         _hip.dptr(lengths, torch.int32, True), _hip.dptr(out),
                                         _hip.dptr(self.plan(x.device), torch.uint8), *self._geometry(),
                                         *self._workspace(lib, _hip.ci(B), _hip.ci(Lcap), x.device), _hip.stream()),
                   "air_cqcc_spectrum")
        return out
