"""On-the-fly channel (impulse-response) augmentation in the HIP front-end
(BASELINE.json configs[4]).

The reference augments its corpora offline with idiap/acoustic-simulator
(channel_simulation/simulated_device.py:16-61: one random device IR per utterance, written back
as wav files).  Here the same operation runs on the GPU between the PCM batch and the LFCC
kernel: ``y = (x * h)[:L]`` rescaled to the input peak, one IR per utterance drawn from a bank
(``random.choice`` semantics, seeded), with probability ``p`` per utterance.  The tool's ``.ir``
files are not distributable with the reference, so ``synthetic_ir_bank`` provides device-like
(short, coloured) and room-like (exponentially decaying noise tail) responses; a real bank loads
with ``ChannelAugment(irs=tensor)``.  Arithmetic spec and parity status: oracle/channel.py.
"""
import numpy as np
import torch

from . import _hip, ops
from .ragged import PinnedUpload, device_lengths, pcm_pointers


def synthetic_ir_bank(n_device=27, n_space=3, taps=1024, sr=16000, seed=688):
    """(n_device + n_space, taps) float32.  Counts follow simulated_device.py:38-39
    (``random.sample(recDevices, 27)``, ``random.sample(recSpace, 3)``).
    Device IRs: direct path + a few early taps + a two-pole resonance within ~4 ms;
    space IRs: direct path + exponentially decaying noise, RT60 in 0.15-0.5 s (cut at ``taps``)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    bank = np.zeros((n_device + n_space, taps), dtype=np.float64)
    n = np.arange(taps)
    for i in range(n_device):
        h = np.zeros(taps)
        h[0] = 1.0
        k = min(taps, 64)
        fc, bw = rng.uniform(300.0, 6000.0), rng.uniform(200.0, 2000.0)
        r = np.exp(-np.pi * bw / sr)
        res = (r ** n[:k]) * np.cos(2 * np.pi * fc / sr * n[:k] + rng.uniform(0, np.pi))
        h[:k] += rng.uniform(0.2, 0.9) * res
        h[1:k] += 0.05 * rng.standard_normal(k - 1) * np.exp(-n[1:k] / 8.0)
        bank[i] = h
    for i in range(n_space):
        rt60 = rng.uniform(0.15, 0.5)
        decay = np.exp(-6.907755 * n / (rt60 * sr))
        h = 0.3 * rng.standard_normal(taps) * decay
        h[: int(0.002 * sr)] *= 0.1
        h[0] = 1.0
        bank[n_device + i] = h
    bank /= np.sqrt((bank ** 2).sum(1, keepdims=True))
    return torch.from_numpy(bank.astype(np.float32))


MAX_BANK_TAPS = 65536  # air_ir_bank_convolve's limit per response


class IRBank:
    """Impulse responses of different lengths (device responses of a few milliseconds beside room responses of seconds),
    for ``ir_convolve`` / ``ChannelAugment``: ``air_ir_bank_convolve`` charges each row of a batch for the response it
    drew.  ``responses``: a sequence of 1-D arrays or tensors, each of 1 .. 65 536 taps (ValueError otherwise).
    ``irs`` (n_ir, Hmax) float32, padded with zeros; ``taps`` (n_ir,) int32, the lengths - both move with ``to(device)``,
    the kernel reads the tap counts on the device."""

    def __init__(self, responses):
        rows = [torch.as_tensor(np.asarray(r.detach().cpu() if torch.is_tensor(r) else r)).to(torch.float32) for r in responses]
        if not rows:
            raise ValueError("an IRBank needs at least one response")
        for i, r in enumerate(rows):
            if r.dim() != 1 or r.numel() < 1:
                raise ValueError("response %d is empty or not 1-D: shape %s" % (i, tuple(r.shape)))
            if r.numel() > MAX_BANK_TAPS:
                raise ValueError("response %d has %d taps, above the limit of %d" % (i, r.numel(), MAX_BANK_TAPS))
        self.taps = torch.tensor([r.numel() for r in rows], dtype=torch.int32)
        self.irs = torch.zeros((len(rows), int(self.taps.max())), dtype=torch.float32)
        for i, r in enumerate(rows):
            self.irs[i, : r.numel()] = r

    def __len__(self):
        return self.irs.shape[0]

    def to(self, device):
        other = object.__new__(IRBank)
        other.irs = self.irs.to(device=device, dtype=torch.float32).contiguous()
        other.taps = self.taps.to(device=device, dtype=torch.int32).contiguous()
        return other


def synthetic_room_bank(n_device=27, n_space=3, sr=16000, seed=688, rt60=(0.2, 1.0)):
    """``IRBank`` of ``n_device`` device responses - drawn as in ``synthetic_ir_bank``, 1024 taps - and ``n_space`` room
    responses that run to their own -60 dB point: direct path + exponentially decaying noise of ``rt60 * sr`` taps, RT60
    uniform in ``rt60`` seconds (3 200 .. 16 000 taps at 16 kHz).  Every response has unit energy."""
    rows = list(synthetic_ir_bank(n_device, 0, 1024, sr, seed)) if n_device else []
    rng = np.random.Generator(np.random.PCG64([seed, 1]))
    for _ in range(n_space):
        t60 = rng.uniform(rt60[0], rt60[1])
        taps = min(max(int(round(t60 * sr)), 1), MAX_BANK_TAPS)
        n = np.arange(taps)
        h = 0.3 * rng.standard_normal(taps) * np.exp(-6.907755 * n / (t60 * sr))
        h[: int(0.002 * sr)] *= 0.1
        h[0] = 1.0
        rows.append(torch.from_numpy((h / np.sqrt((h ** 2).sum())).astype(np.float32)))
    return IRBank(rows)


def _checked(what, pcm, lengths, out, others=(), dense_fp32=False):
    """The argument checks of the library entry points here -> (B, L, lengths on the device or None, y): GPU tensors
    only, PCM float32 or int16 (``dense_fp32``: a dense call's dtype is left to the pointer check), host lengths checked
    (ValueError) and uploaded, ``out`` or a fresh fp32 result."""
    if not pcm.is_cuda or any(t is not None and not t.is_cuda for t in others):
        raise _hip.AirError("%s needs GPU tensors; there is no CPU fallback" % what)
    if not (dense_fp32 and lengths is None) and pcm.dtype not in (torch.float32, torch.int16):
        raise _hip.AirError("PCM is float32 or int16, got %s" % pcm.dtype)
    B, L = pcm.shape
    if lengths is not None:
        lengths = device_lengths(lengths, B, L, pcm.device)
    return B, L, lengths, out if out is not None else torch.empty(pcm.shape, dtype=torch.float32, device=pcm.device)


def _call_tail(idx, normalize, y, n):
    """(idx, normalize, y, workspace, its bytes, stream): what ends the argument lists of the convolution entry points."""
    return (_hip.dptr(idx, torch.int32, True), _hip.ci(1 if normalize else 0), _hip.dptr(y),
            _hip.dptr(ops.workspace(n, y.device), torch.uint8), _hip.csz(n), _hip.stream())


def ir_convolve(pcm, irs, idx=None, normalize=True, out=None, lengths=None):
    """pcm (B, L) fp32 GPU, irs (n_ir, H) fp32 GPU, idx (B,) int32 GPU or None -> (B, L).

    ``lengths`` (B,) int32: a ragged batch in one launch (``air_ir_convolve_ragged``) - row b of ``pcm`` (B, Lcap), fp32
    or int16 (s / 32768), holds lengths[b] samples; what follows them is never read.  Row b of the fp32 result is, bit
    for bit, what the dense call gives for that utterance alone (convolved, truncated and peak-normalised over its own
    samples), followed by zeros.  A GPU tensor is used as is, host values are checked (ValueError) and uploaded.

    ``irs`` may be an ``IRBank`` (on the GPU): ``air_ir_bank_convolve``, dense or ragged, every row against the leading
    ``taps`` columns of the response it drew - up to 65 536 of them."""
    if isinstance(irs, IRBank):
        return _bank_convolve(pcm, irs, idx, normalize, out, lengths)
    B, L, lengths, y = _checked("ir_convolve", pcm, lengths, out, (irs,), dense_fp32=True)
    n_ir, H = irs.shape
    lib = _hip.lib()
    n = lib.air_ir_convolve_ws_bytes_ex(_hip.ci(B), _hip.ci(n_ir), _hip.ci(H))  # (+ the FFT tables when H qualifies)
    tail = (_hip.dptr(irs), _hip.ci(n_ir), _hip.ci(H)) + _call_tail(idx, normalize, y, n)
    if lengths is None:
        _hip.check(lib.air_ir_convolve(_hip.dptr(pcm), _hip.ci(B), _hip.ci(L), *tail), "air_ir_convolve")
    else:
        _hip.check(lib.air_ir_convolve_ragged(*pcm_pointers(pcm), _hip.ci(B), _hip.ci(L), _hip.dptr(lengths, torch.int32), *tail),
                   "air_ir_convolve_ragged")
    return y


def _bank_convolve(pcm, bank, idx, normalize, out, lengths):
    B, L, lengths, y = _checked("ir_convolve", pcm, lengths, out, (bank.irs, bank.taps))
    n_ir, H = bank.irs.shape
    lib = _hip.lib()
    n = lib.air_ir_bank_ws_bytes(_hip.ci(B), _hip.ci(L), _hip.ci(n_ir), _hip.ci(H))
    _hip.check(lib.air_ir_bank_convolve(*pcm_pointers(pcm), _hip.ci(B), _hip.ci(L), _hip.dptr(lengths, torch.int32, True),
                                        _hip.dptr(bank.irs), _hip.ci(n_ir), _hip.ci(H), _hip.dptr(bank.taps, torch.int32),
                                        *_call_tail(idx, normalize, y, n)), "air_ir_bank_convolve")
    return y


class _RandomAugment:
    """What the augmenters share: per utterance one of ``len(getattr(self, CHOICES))`` choices, applied with probability
    ``p``, drawn from one ``np.random.Generator(PCG64(seed))``; host arrays go up through ``self._upload``."""

    supports_lengths = True  # __call__(pcm, lengths=...) augments a ragged batch over each row's own samples (Trainer.step)
    CHOICES = None           # the attribute that holds the choices: "irs" | "laws" | "algos"

    def __init__(self, p, seed):
        self.p = float(p)
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self._upload = PinnedUpload()

    def draw(self, batch):
        """(B,) int32 indices into the choices, -1 = leave the utterance unchanged."""
        idx = self.rng.integers(0, len(getattr(self, self.CHOICES)), size=batch).astype(np.int32)
        if self.p < 1.0:
            idx[self.rng.random(batch) >= self.p] = -1
        return idx

    def _begin(self, pcm, idx, lengths):
        """The head of every ``__call__`` -> (idx, lengths on the device): the lengths are checked ahead of the draw - a
        refused batch must not advance the generator."""
        if lengths is not None:
            lengths = device_lengths(lengths, pcm.shape[0], pcm.shape[1], pcm.device)
        return (self.draw(pcm.shape[0]) if idx is None else idx), lengths


class ChannelAugment(_RandomAugment):
    """Per-utterance random IR from a bank - a (n_ir, H) tensor or an ``IRBank`` - applied with probability ``p``."""

    CHOICES = "irs"

    def __init__(self, irs=None, p=1.0, seed=688, normalize=True, device="cuda"):
        super().__init__(p, seed)
        if isinstance(irs, IRBank):
            self.irs = irs.to(device)
        else:
            self.irs = (irs if irs is not None else synthetic_ir_bank()).to(device=device, dtype=torch.float32).contiguous()
        self.normalize = normalize

    def __call__(self, pcm, idx=None, lengths=None):
        """``lengths``: int32 (B,), a ragged batch (``ir_convolve``): fp32 or int16 in, fp32 out, the rows' tails zero."""
        idx, lengths = self._begin(pcm, idx, lengths)
        if not torch.is_tensor(idx):
            idx = self._upload(np.asarray(idx, dtype=np.int32), pcm.device)
        return ir_convolve(pcm, self.irs, idx.to(device=pcm.device, dtype=torch.int32).contiguous(), self.normalize,
                           lengths=lengths)


# ------------------------------------------------------------------------------------------------ transmission codec
LAWS = ("ulaw", "alaw")  # air_g711_ragged's law indices


def _lowpass64(ntaps, cutoff_hz, sr, beta):
    """The float64 design behind ``codec_lowpass``."""
    if ntaps < 1 or ntaps % 2 == 0:
        raise ValueError("ntaps must be odd and positive, got %d" % ntaps)
    fc = 2.0 * cutoff_hz / sr  # of Nyquist
    n = np.arange(ntaps, dtype=np.float64) - (ntaps - 1) / 2.0
    h = fc * np.sinc(fc * n) * np.kaiser(ntaps, beta)
    return h / h.sum()


def codec_lowpass(ntaps=63, cutoff_hz=3680.0, sr=16000, beta=8.0):
    """The low-pass both resamplers of ``g711_codec`` use: a Kaiser-windowed sinc of ``ntaps`` (odd) coefficients, cut
    off at ``cutoff_hz`` of a ``sr`` Hz signal, unit DC gain.  Designed in float64 (numpy), returned as float32."""
    return torch.from_numpy(_lowpass64(ntaps, cutoff_hz, sr, beta).astype(np.float32))


def g711_codec(pcm, law_idx=None, lengths=None, fir=None, resample=True, normalize=True, out=None, return_codes=False):
    """pcm (B, L) fp32 or int16 GPU -> (B, L) fp32: each row through a G.711 telephone channel (``air_g711_ragged``):
    low-pass and decimate to half the rate, quantise to 16 bits, code and decode, interpolate back, rescale to the input
    peak.  ``law_idx`` (B,) int32 GPU: 0 mu-law, 1 A-law, < 0 leaves the row unchanged; None is mu-law for all.
    ``lengths`` as in ``ir_convolve``: row b holds lengths[b] samples, its tail is never read and comes back zero.
    ``fir``: the low-pass (odd, at most 127 taps; default ``codec_lowpass()``).  ``resample=False`` codes every sample
    at its own rate.  ``return_codes``: also the uint8 codes, (B, (L + 1) // 2) or, without resampling, (B, L)."""
    B, L, lengths, y = _checked("g711_codec", pcm, lengths, out, (fir, law_idx))
    if law_idx is not None and law_idx.numel() != B:
        raise ValueError("law_idx must have %d entries, got %d" % (B, law_idx.numel()))
    if fir is None:
        fir = _default_fir(pcm.device)
    codes = torch.empty((B, (L + 1) // 2 if resample else L), dtype=torch.uint8, device=pcm.device) if return_codes else None
    lib = _hip.lib()
    n = lib.air_g711_ws_bytes(_hip.ci(B))
    ws = ops.workspace(n, pcm.device)
    _hip.check(lib.air_g711_ragged(*pcm_pointers(pcm), _hip.ci(B), _hip.ci(L), _hip.dptr(lengths, torch.int32, True), _hip.dptr(fir),
                                   _hip.ci(fir.numel()), _hip.dptr(law_idx, torch.int32, True), _hip.ci(1 if resample else 0),
                                   _hip.ci(1 if normalize else 0), _hip.dptr(y), _hip.dptr(codes, torch.uint8, True),
                                   _hip.dptr(ws, torch.uint8), _hip.csz(n), _hip.stream()), "air_g711_ragged")
    return (y, codes) if return_codes else y


_FIR = {}


def _default_fir(device):
    key = str(device)
    if key not in _FIR:
        _FIR[key] = codec_lowpass().to(device)
    return _FIR[key]


class CodecAugment(_RandomAugment):
    """Per-utterance random G.711 law out of ``laws``, applied with probability ``p`` (the sample-parallel entries of the
    reference's ``codec_landline`` list; channel_simulation/simulated_channel.py degrades the corpus with them offline)."""

    CHOICES = "laws"

    def __init__(self, laws=("ulaw", "alaw"), p=1.0, seed=688, normalize=True, fir=None, device="cuda"):
        if not laws or any(name not in LAWS for name in laws):
            raise ValueError("laws must be taken from %s, got %s" % (LAWS, laws))
        super().__init__(p, seed)
        self.laws = tuple(laws)
        self._kernel_law = np.array([LAWS.index(name) for name in self.laws], dtype=np.int32)
        self.normalize = normalize
        self.device = device
        self.fir = None if fir is None else fir.to(device=device, dtype=torch.float32).contiguous()

    def __call__(self, pcm, idx=None, lengths=None):
        idx, lengths = self._begin(pcm, idx, lengths)
        if not torch.is_tensor(idx):
            idx = np.asarray(idx, dtype=np.int32)
            idx = self._upload(np.where(idx < 0, -1, self._kernel_law[np.maximum(idx, 0)]).astype(np.int32), pcm.device)
        elif self.laws != LAWS:
            raise ValueError("device indices are the kernel's own (0 mu-law, 1 A-law): pass host indices with laws=%s" % (self.laws,))
        return g711_codec(pcm, idx.to(device=pcm.device, dtype=torch.int32).contiguous(), lengths=lengths, fir=self.fir,
                          normalize=self.normalize)


class AugmentChain:
    """Transmission codec, then recording device - the order of channel_simulation/simulated_device_channel.py:47-54.
    Either stage may be None.  ``prepare(batch)`` draws for the next call and returns what was drawn as the channel
    classes of ``AdversarialTrainer.step(..., channels=)``: 0 = unchanged (the reference's ``no_channel``), index + 1
    otherwise; (B, 2) int64 (codec, device) with both stages, (B,) with one.  ``waveform`` (a ``RawBoostAugment``), when
    given, is applied first - it degrades the source signal, ahead of the channel - and adds its own label column in
    front: 0 = unchanged, index into its ``algos`` + 1."""

    supports_lengths = True

    def __init__(self, codec=None, device=None, waveform=None):
        if codec is None and device is None and waveform is None:
            raise ValueError("AugmentChain needs a codec stage, a device stage, or both")
        self.stages = [s for s in (waveform, codec, device) if s is not None]
        self.codec, self.device, self.waveform = codec, device, waveform
        self._prepared = None

    def prepare(self, batch):
        self._prepared = [np.asarray(s.draw(batch)) for s in self.stages]
        labels = np.stack([np.where(i < 0, 0, i.astype(np.int64) + 1) for i in self._prepared], axis=1)
        return torch.from_numpy(labels[:, 0].copy() if len(self.stages) == 1 else labels)

    def __call__(self, pcm, lengths=None):
        if lengths is not None:  # ahead of any draw
            lengths = device_lengths(lengths, pcm.shape[0], pcm.shape[1], pcm.device)
        drawn, self._prepared = self._prepared, None
        if drawn is not None and len(drawn[0]) != pcm.shape[0]:
            raise ValueError("prepared for a batch of %d, called with %d" % (len(drawn[0]), pcm.shape[0]))
        for k, stage in enumerate(self.stages):
            pcm = stage(pcm, None if drawn is None else drawn[k], lengths=lengths)
        return pcm


# ---------------------------------------------------------------------------------------------------------- RawBoost
# Layout of the parameter table (include/air_hip.h, "RawBoost"): (B, 164) float64, every entry exact in a double.
RB_HDR, RB_FILTERS, RB_NF, RB_MAXBANDS, RB_MAXTAPS = 8, 6, 5, 8, 512
RB_FREC = 2 + 3 * RB_MAXBANDS
RB_ROW = RB_HDR + RB_FILTERS * RB_FREC
RB_MAXL = 1 << 20                # samples per row the ISD stream reserves; air_rawboost_ragged refuses a longer Lcap
RB_KEY_TAG = 0x5242 << 36        # Philox keys: RB_KEY_TAG | seed << 1 | {0: ISD, 1: SSI}
RB_LNL, RB_ISD, RB_SSI = (0, 3, 4, 5, 7), (1, 3, 4, 6, 7), (2, 3, 5, 6)
RB_DEFAULTS = dict(nBands=5, minF=20.0, maxF=8000.0, minBW=100.0, maxBW=1000.0, minCoeff=10, maxCoeff=100, minG=0.0, maxG=0.0,
                   minBiasLinNonLin=5.0, maxBiasLinNonLin=20.0, N_f=5, P=10.0, g_sd=2.0, SNRmin=10.0, SNRmax=40.0)


def _rb_table(table, B, device):
    if not (torch.is_tensor(table) and table.is_cuda):
        raise _hip.AirError("the RawBoost table must be a GPU tensor; there is no CPU fallback")
    if table.dtype != torch.float64 or tuple(table.shape) != (B, RB_ROW):
        raise ValueError("the RawBoost table is (%d, %d) float64, got %s %s" % (B, RB_ROW, tuple(table.shape), table.dtype))
    return table.contiguous()


def rawboost_design(table):
    """table (B, 164) float64 GPU -> (taps (B, 6, 512) fp32, lens (B, 6) int32): the notch cascades ``rawboost`` filters
    with (``air_rawboost_design``: designed in fp64 on the device, rounded once), zero behind each length."""
    B = table.shape[0]
    table = _rb_table(table, B, table.device)
    taps = torch.empty((B, RB_FILTERS, RB_MAXTAPS), dtype=torch.float32, device=table.device)
    lens = torch.empty((B, RB_FILTERS), dtype=torch.int32, device=table.device)
    _hip.check(_hip.lib().air_rawboost_design(_hip.dptr(table, torch.float64), _hip.ci(B), _hip.dptr(taps),
                                              _hip.dptr(lens, torch.int32), _hip.stream()), "air_rawboost_design")
    return taps, lens


def rawboost(pcm, table, lengths=None, out=None):
    """pcm (B, L) fp32 or int16 GPU, table (B, 164) float64 GPU (``RawBoostAugment.params``) -> (B, L) fp32: RawBoost
    (``air_rawboost_ragged``) - per row one of LnL (0), ISD (1), SSI (2), their chains (3 - 6) or the parallel form (7);
    any other algorithm entry copies the row.  ``lengths`` as in ``ir_convolve``: row b holds lengths[b] samples, its tail
    is never read and comes back zero, and the row carries the bits of the dense call on that utterance alone."""
    B, L, lengths, y = _checked("rawboost", pcm, lengths, out)
    if L > RB_MAXL:
        raise ValueError("rows of at most %d samples, got %d" % (RB_MAXL, L))
    table = _rb_table(table, B, pcm.device)
    lib = _hip.lib()
    n = lib.air_rawboost_ws_bytes(_hip.ci(B), _hip.ci(L))
    ws = ops.workspace(n, pcm.device)
    _hip.check(lib.air_rawboost_ragged(*pcm_pointers(pcm), _hip.ci(B), _hip.ci(L), _hip.dptr(lengths, torch.int32, True),
                                       _hip.dptr(table, torch.float64), _hip.dptr(y), _hip.dptr(ws, torch.uint8), _hip.csz(n),
                                       _hip.stream()), "air_rawboost_ragged")
    return y


class RawBoostAugment(_RandomAugment):
    """RawBoost (Tak et al., ICASSP 2022), per utterance one algorithm out of ``algos`` (0 LnL, 1 ISD, 2 SSI, 3 all three in
    series, 4 LnL -> ISD, 5 LnL -> SSI, 6 ISD -> SSI, 7 LnL and ISD in parallel), applied with probability ``p``.
    ``config`` overrides the authors' defaults (``RB_DEFAULTS``).  A configuration whose cascade could exceed 512 taps,
    more than 8 bands or more than 5 LnL filters: ValueError.

    One ``np.random.Generator(PCG64(seed))`` serves every draw, each as ``lo + (hi - lo) * rng.random()`` (``U``):
      ``draw(B)``    ``rng.integers(0, len(algos), B)``, then, with p < 1, ``rng.random(B) >= p`` marks the unchanged rows;
      ``params(idx)`` rows in order, a row of algorithm a: with LnL, filter i = 0 .. N_f - 1: its nBands bands - fc =
                     U(minF, maxF), bw = U(minBW, maxBW), c = int(U(minCoeff, maxCoeff)), + 1 if even - then G = U(minG,
                     maxG) for i = 0 and U(minG - minBias, maxG - maxBias) behind it; with ISD, beta = U(0, P); with SSI,
                     the bands, G = U(minG, maxG), SNR = U(SNRmin, SNRmax).  Unchanged rows draw nothing.
    Nothing depends on the rows' lengths.  The Philox counter bases of the two noise stages are held here and advance per
    ``params`` call by what a batch of B rows of the longest admissible length would use (B 2^20 ISD counters, B 2^18 SSI
    quads), the two stages under different keys: no two streams of any two calls overlap."""

    CHOICES = "algos"

    def __init__(self, algos=(0, 1, 2), p=1.0, seed=688, device="cuda", **config):
        algos = tuple(int(a) for a in algos)
        if not algos or any(a < 0 or a > 7 for a in algos):
            raise ValueError("algos must be taken from 0 .. 7, got %s" % (algos,))
        unknown = sorted(set(config) - set(RB_DEFAULTS))
        if unknown:
            raise ValueError("unknown RawBoost parameters: %s" % unknown)
        cfg = dict(RB_DEFAULTS, **config)
        cfg["nBands"], cfg["N_f"] = int(cfg["nBands"]), int(cfg["N_f"])
        if not 1 <= cfg["nBands"] <= RB_MAXBANDS or not 1 <= cfg["N_f"] <= RB_NF:
            raise ValueError("nBands in [1, %d] and N_f in [1, %d], got %d and %d" % (RB_MAXBANDS, RB_NF, cfg["nBands"], cfg["N_f"]))
        if not 1 <= cfg["minCoeff"] <= cfg["maxCoeff"]:
            raise ValueError("1 <= minCoeff <= maxCoeff, got %s and %s" % (cfg["minCoeff"], cfg["maxCoeff"]))
        c_up = int(cfg["maxCoeff"]) + (1 if int(cfg["maxCoeff"]) % 2 == 0 else 0)
        if cfg["nBands"] * c_up - (cfg["nBands"] - 1) > RB_MAXTAPS:
            raise ValueError("%d bands of up to %d coefficients give a cascade of %d taps, above the limit of %d" % (
                cfg["nBands"], c_up, cfg["nBands"] * c_up - (cfg["nBands"] - 1), RB_MAXTAPS))
        if not 0 <= int(seed) < 1 << 35:
            raise ValueError("seed in [0, 2^35), got %s" % seed)
        super().__init__(p, seed)
        self.algos, self.config, self.seed, self.device = algos, cfg, int(seed), device
        self._kernel_algo = np.array(algos, dtype=np.int32)
        self.isd_base = self.ssi_base = 0

    def _u(self, lo, hi):
        return lo + (hi - lo) * self.rng.random()

    def _bands(self):
        cfg, out = self.config, []
        for _ in range(cfg["nBands"]):
            fc, bw = self._u(cfg["minF"], cfg["maxF"]), self._u(cfg["minBW"], cfg["maxBW"])
            c = int(self._u(cfg["minCoeff"], cfg["maxCoeff"]))
            out += [fc, bw, c + 1 if c % 2 == 0 else c]
        return out

    def params(self, idx):
        """idx (B,) host indices into ``algos`` (-1 unchanged) -> the (B, 164) float64 host table of ``rawboost``."""
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        B, cfg = idx.size, self.config
        if self.isd_base + B * RB_MAXL >= 1 << 53:
            raise OverflowError("the RawBoost noise streams are exhausted: start a new augmenter (another seed)")
        t = np.zeros((B, RB_ROW), dtype=np.float64)
        t[:, 0] = np.where(idx < 0, -1, self._kernel_algo[np.clip(idx, 0, len(self.algos) - 1)])
        t[:, 3], t[:, 4] = self.isd_base, self.ssi_base
        t[:, 6], t[:, 7] = RB_KEY_TAG | (self.seed << 1), RB_KEY_TAG | (self.seed << 1) | 1
        for row in t:
            a = int(row[0])
            if a in RB_LNL:
                for i in range(cfg["N_f"]):
                    rec = row[RB_HDR + i * RB_FREC: RB_HDR + (i + 1) * RB_FREC]
                    rec[2: 2 + 3 * cfg["nBands"]] = self._bands()
                    rec[1] = cfg["nBands"]
                    rec[0] = self._u(cfg["minG"], cfg["maxG"]) if i == 0 else self._u(
                        cfg["minG"] - cfg["minBiasLinNonLin"], cfg["maxG"] - cfg["maxBiasLinNonLin"])
            if a in RB_ISD:
                row[1] = np.floor(self._u(0.0, cfg["P"]) / 100.0 * 4294967296.0)
                row[2] = cfg["g_sd"]
            if a in RB_SSI:
                rec = row[RB_HDR + RB_NF * RB_FREC:]
                rec[2: 2 + 3 * cfg["nBands"]] = self._bands()
                rec[1] = cfg["nBands"]
                rec[0] = self._u(cfg["minG"], cfg["maxG"])
                row[5] = self._u(cfg["SNRmin"], cfg["SNRmax"])
        self.isd_base += B * RB_MAXL
        self.ssi_base += B * (RB_MAXL // 4)
        return t

    def __call__(self, pcm, idx=None, lengths=None):
        if pcm.dim() != 2 or pcm.shape[1] > RB_MAXL:
            raise ValueError("PCM is (B, L) with L <= %d, got %s" % (RB_MAXL, tuple(pcm.shape)))
        idx, lengths = self._begin(pcm, idx, lengths)
        if torch.is_tensor(idx):
            idx = idx.cpu().numpy()
        if len(idx) != pcm.shape[0]:
            raise ValueError("idx must have %d entries, got %d" % (pcm.shape[0], len(idx)))
        return rawboost(pcm, self._upload(self.params(idx), pcm.device), lengths=lengths)
