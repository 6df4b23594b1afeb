"""Sample-rate conversion on the device: ragged PCM of any served rate -> a ragged batch at 16 kHz.

The reference resamples on the host (``librosa.load(path, sr=16000)``, raw_dataset.py:20-28).  Here the conversion is the
band-limited sinc interpolation defined in include/air_hip.h ("WAV decode / resample"): the parameters of the
``kaiser_best`` filter, every coefficient evaluated exactly at its phase in fp64 on the host
(``air_resample_table_host``), rounded once to fp32, accumulated in fp32 on the device (csrc/resample.hip).  Parity with
librosa's own resampler is not pinned: the tests hold the device to an fp64 statement of these formulas.

``Resampler.resample`` serves PCM that already lies on the device (``FlacDecoder.decode`` of a file that is not at
16 kHz); ``wav.WavDecoder`` runs the same kernel straight from the bytes of ``.wav`` files.  Both take the rows' source
rates as HOST integers (they come from the file headers): the kernel's per-rate records and tables are looked up without
reading device memory, so neither synchronises.
"""
import ctypes

import numpy as np
import torch

from . import _hip
from .ragged import RAGGED_ROUND, DeviceRing, check_status, round_capacity  # noqa: F401  (RAGGED_ROUND, DeviceRing: re-exported)

TARGET_SR = 16000
MAX_RATES = 8           # AIR_RESAMPLE_MAX_RATES: distinct source rates of one batch
# sample kinds of include/air_hip.h (AIR_PCM_*) and their bytes per sample
U8, S16, S24, S32, F32, F64 = range(6)
KIND_BYTES = {U8: 1, S16: 2, S24: 3, S32: 4, F32: 4, F64: 8}
# row status (AIR_WAV_*)
OK, LENGTH_MISMATCH, BAD_FORMAT = range(3)
STATUS = {OK: "OK", LENGTH_MISMATCH: "LENGTH_MISMATCH", BAD_FORMAT: "BAD_FORMAT"}


class AirResampleRate(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("L", "M", "K", "table_off")]


class AirResampleDesc(ctypes.Structure):
    _fields_ = [("nrates", ctypes.c_int), ("rate", AirResampleRate * MAX_RATES)]


def geometry(sr, target=TARGET_SR, name=None):
    """(L, M, K) of the conversion ``sr`` -> ``target`` (K = 0: the identity).  ValueError, naming the file and the
    rate, for what the device path does not serve (a non-positive rate, target / gcd > 640, a rate above 16 x target)."""
    L, M, K = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    ok = 0 < int(sr) < 2 ** 31 and 0 < int(target) < 2 ** 31
    if not ok or _hip.lib().air_resample_geometry(_hip.ci(int(sr)), _hip.ci(int(target)), ctypes.byref(L), ctypes.byref(M),
                                                   ctypes.byref(K)) != 0:
        raise ValueError("%s: sample_rate = %s: not served by the device resampler to %d Hz (%d / gcd must not exceed 640, "
                         "the rate not 16 x the target)" % (name or "<pcm>", sr, target, target))
    return L.value, M.value, K.value


def out_length(n, sr, target=TARGET_SR):
    """Samples the conversion of ``n`` samples at ``sr`` yields: ceil(n L / M).  ``n``: an int or an integer array."""
    L, M, _ = geometry(sr, target)
    if isinstance(n, (int, np.integer)):
        return -(-int(n) * L // M)
    return -(-np.asarray(n, dtype=np.int64) * L // M)


def host_table(sr, target=TARGET_SR):
    """The (L, K) fp32 coefficient table of ``sr`` -> ``target`` as a CPU tensor (None for the identity)."""
    L, M, K = geometry(sr, target)
    if K == 0:
        return None
    t = torch.empty((L, K), dtype=torch.float32)
    _hip.check(_hip.lib().air_resample_table_host(_hip.ci(int(sr)), _hip.ci(int(target)), _hip.hptr(t)), "air_resample_table_host")
    return t


def rate_list(rates, B):
    """``rates`` (one int for every row, or a sequence / host array of B ints) -> a tuple of B ints.  A device tensor
    is refused: reading it would synchronise, and the rates come from file headers on the host anyway."""
    if torch.is_tensor(rates):
        if rates.is_cuda:
            raise ValueError("rates are host integers (from the file headers), not a device tensor")
        rates = rates.reshape(-1).tolist()
    elif isinstance(rates, (int, np.integer)):
        rates = [int(rates)] * B
    rates = tuple(int(r) for r in rates)
    if len(rates) != B:
        raise ValueError("rates has %d entries for %d rows" % (len(rates), B))
    return rates


def distinct(rates):
    """The distinct rates of a batch in order of first appearance.  ValueError beyond MAX_RATES."""
    seen = list(dict.fromkeys(int(r) for r in rates))
    if len(seen) > MAX_RATES:
        raise ValueError("a batch mixes %d distinct source rates %s: the device resampler serves at most %d per launch"
                         % (len(seen), seen, MAX_RATES))
    return seen


class RateBank(DeviceRing):
    """The per-rate coefficient tables on the device and the per-batch records.  A table is computed once per rate
    (host, fp64 -> fp32) and appended to one device buffer; a batch's record list, its per-row index and per-row L / M
    tensors are cached by the batch's rate tuple (a corpus has one rate: one entry)."""

    PLAN_CACHE = 64

    def __init__(self, device="cuda", depth=4, target_sr=TARGET_SR):
        super().__init__(device, depth)
        self.target_sr = int(target_sr)
        self._geom, self._off = {}, {}
        self._tables, self._used = None, 0
        self._retired = []  # earlier table buffers: launches already enqueued may still read them
        self._plans = {}

    def _table_off(self, sr):
        off = self._off.get(sr)
        if off is None:
            t = host_table(sr, self.target_sr).reshape(-1)
            need = self._used + t.numel()
            if self._tables is None or need > self._tables.numel():
                grown = torch.zeros(max(need, 2 * self._used, 1 << 16), dtype=torch.float32, device=self.device)
                if self._tables is not None:
                    grown[:self._used].copy_(self._tables[:self._used])
                    self._retired.append(self._tables)
                self._tables = grown
            self._tables[self._used:need].copy_(t, non_blocking=True)
            off = self._off[sr] = self._used
            self._used = need
        return off

    def plan(self, rates):
        """-> (desc, rate_idx (B) int32, L (B) int64, M (B) int64 on the device, tables, table_elems)."""
        hit = self._plans.get(rates)
        if hit is None:
            seen = distinct(rates)
            desc = AirResampleDesc()
            desc.nrates = len(seen)
            geo = []
            for r, sr in enumerate(seen):
                L, M, K = self._geom.get(sr) or self._geom.setdefault(sr, geometry(sr, self.target_sr))
                geo.append((L, M))
                desc.rate[r] = AirResampleRate(L, M, K, self._table_off(sr) if K else 0)
            idx = [seen.index(r) for r in rates]
            dev = lambda v, dt: torch.tensor(v, dtype=dt).to(self.device, non_blocking=True)
            if len(self._plans) >= self.PLAN_CACHE:
                self._plans.clear()
            hit = self._plans[rates] = (desc, dev(idx, torch.int32), dev([geo[i][0] for i in idx], torch.int64),
                                        dev([geo[i][1] for i in idx], torch.int64))
        if self._tables is None:  # identity records only: the kernel reads no table
            self._tables = torch.zeros(1 << 16, dtype=torch.float32, device=self.device)
        # a plan made before the table buffer grew keeps valid offsets: tables are only ever appended
        return hit + (self._tables, self._used)

    def host_lengths(self, n, rates):
        """ceil(n L / M) per row on the host (``n``: B ints)."""
        return [out_length(int(v), sr, self.target_sr) for v, sr in zip(n, rates)]


class ResampleError(RuntimeError):
    """Rows of a batch the device refused: ``rows`` = [(row, status code), ...]."""

    def __init__(self, rows, what="resample"):
        self.rows = list(rows)
        super().__init__("%s failed for %d row(s): %s" % (what, len(self.rows), ", ".join(
            "row %d %s" % (r, STATUS.get(c, "status %d" % c)) for r, c in self.rows)))


def check(status, what="resample"):
    """Copy ``status`` to the host (synchronises) and raise ResampleError listing the rows that are not OK."""
    check_status(status, OK, lambda rows: ResampleError(rows, what))


_check = check


class Resampler(RateBank):
    """``resample(pcm, lengths, rates)``: a ragged (B, Lcap_in) int16 / float32 batch on the device, row b holding
    ``lengths[b]`` samples at ``rates[b]`` Hz -> the (B, Lcap) batch at ``target_sr``."""

    def __init__(self, device="cuda", target_sr=TARGET_SR, depth=4):
        super().__init__(device, depth, target_sr)

    def resample(self, pcm, lengths, rates, Lcap=None, dtype=torch.float32, check=False, out=None):
        """-> (pcm (B, Lcap) ``dtype``, out_lengths (B,) int32), both on the device; tails are zero.  int16 input is
        sample / 32768; int16 output the saturating round-half-even of 32768 y.  Never synchronises when ``Lcap`` is
        given; ``Lcap=None`` takes the longest output row rounded up to RAGGED_ROUND, which reads ``lengths``.  The row
        status of the call stays in ``last_status`` (``check=True`` reads it: synchronous)."""
        if pcm.dim() != 2 or pcm.dtype not in (torch.int16, torch.float32):
            raise ValueError("pcm is a (B, Lcap) int16 or float32 tensor")
        B, Lcap_in = int(pcm.shape[0]), int(pcm.shape[1])
        if lengths.shape[0] != B:
            raise ValueError("lengths has B entries")
        rates = rate_list(rates, B)
        desc, idx, Lrow, Mrow, tables, used = self.plan(rates)
        if Lcap is None:
            Lcap = round_capacity(max(self.host_lengths(lengths.detach().cpu().tolist(), rates)))
        Lcap = int(Lcap)
        lengths = lengths.to(self.device, non_blocking=True)
        if lengths.dtype != torch.int32:
            lengths = lengths.to(torch.int32)
        y, status, p16, p32 = self._output(B, Lcap, dtype, out)
        kind = S16 if pcm.dtype == torch.int16 else F32
        _hip.check(_hip.lib().air_resample_ragged(
            _hip.dptr(pcm, pcm.dtype), _hip.ci(kind), _hip.ci(B), _hip.ci(Lcap_in), _hip.dptr(lengths, torch.int32),
            _hip.dptr(idx, torch.int32), ctypes.byref(desc), _hip.dptr(tables), _hip.csz(used), p16, p32, _hip.ci(Lcap),
            _hip.dptr(status, torch.int32), _hip.stream()), "air_resample_ragged")
        out_lengths = ((lengths.to(torch.int64) * Lrow + (Mrow - 1)) // Mrow).to(torch.int32)
        self.last_status = status
        if check:
            _check(status)
        return y, out_lengths
