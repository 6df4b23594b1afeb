"""Reading the corpus: ``.wav`` files of any served rate -> ragged PCM batches at 16 kHz, converted on the GPU.

The reference reads a waveform with ``librosa.load(path, sr=16000)`` (raw_dataset.py:20-28): mono, float, 16 kHz whatever
the file holds.  Here the host parses the RIFF header (``parse``) and ships the file's ``data`` payload as it is;
``WavDecoder.decode`` converts the sample format, mixes the channels down and resamples a whole batch in one launch
(csrc/resample.hip, the conversion defined in resample.py / include/air_hip.h) into the (B, Lcap) layout
``Trainer.step(pcm, labels, start=, lengths=)`` reads.  This module mirrors flac.py: the same pinned ring and ``byte_off``
layout (``flac.pack_rows``), the same rings of ``depth`` output / status slots, the same status protocol.

Served: RIFF/WAVE with format tag 1 (PCM: 8, 16, 24, 32 bit), 3 (IEEE float: 32, 64 bit) or 0xFFFE (extensible, with the
PCM or IEEE-float sub-format), 1 - 8 channels, every rate the resampler serves.  ``parse`` refuses everything else on the
host, naming the file and the field; the device reports per row what it could not serve (``STATUS``), never faults.
"""
import collections
import ctypes
import struct

import numpy as np
import torch

from . import _hip, flac, ragged, resample
from .resample import BAD_FORMAT, F32, F64, KIND_BYTES, LENGTH_MISMATCH, OK, S16, S24, S32, STATUS, U8  # noqa: F401

WavInfo = collections.namedtuple("WavInfo", "kind channels sample_rate bits block_align frames data_offset")

KIND_NAMES = {U8: "u8", S16: "s16", S24: "s24", S32: "s32", F32: "f32", F64: "f64"}
_PCM_KINDS = {8: U8, 16: S16, 24: S24, 32: S32}
_FLOAT_KINDS = {32: F32, 64: F64}
# the tail of KSDATAFORMAT_SUBTYPE_PCM / _IEEE_FLOAT: the first two bytes are the format tag
_GUID_TAIL = bytes([0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71])
MAX_CHANNELS = 8


class WavError(resample.ResampleError):
    """Rows of a batch the device refused: ``rows`` = [(row, status code), ...]."""

    def __init__(self, rows):
        super().__init__(rows, "WAV decode")


def fmt_code(kind, channels):
    """AIR_WAV_FMT(kind, bytes per sample, channels)."""
    return int(kind) | (KIND_BYTES[int(kind)] << 4) | (int(channels) << 8)


def parse(buf, name="<buffer>"):
    """A RIFF/WAVE file -> WavInfo.  Chunks come in any order, unknown ones are skipped, odd-sized ones are padded to
    even.  A ``data`` size of 0xFFFFFFFF, or one that runs past the end of the file, means the whole frames actually
    present.  ValueError, naming the file and the field, for what the device path does not serve."""
    buf = memoryview(buf).cast("B") if not isinstance(buf, (bytes, bytearray)) else buf
    n = len(buf)
    magic = bytes(buf[:4])
    if magic in (b"RIFX", b"RF64", b"BW64"):
        raise ValueError("%s: container: %s is not served (little-endian RIFF only)" % (name, magic.decode()))
    if n < 12 or magic != b"RIFF" or bytes(buf[8:12]) != b"WAVE":
        raise ValueError("%s: container: not a RIFF/WAVE file" % name)
    pos, fmt, data = 12, None, None
    while pos + 8 <= n:
        cid = bytes(buf[pos:pos + 4])
        size = struct.unpack_from("<I", buf, pos + 4)[0]
        body = pos + 8
        if cid == b"fmt " and fmt is None:
            if size not in (16, 18, 40) or body + size > n:
                raise ValueError("%s: fmt: a chunk of %d bytes (16, 18 or 40 are served)%s" % (
                    name, size, ", truncated" if body + size > n else ""))
            fmt = (body, size)
        elif cid == b"data" and data is None:
            data = (body, min(size, n - body))
            if size == 0xFFFFFFFF or body + size > n:
                break  # the payload runs to the end of the file
        pos = body + size + (size & 1)
    if fmt is None:
        raise ValueError("%s: fmt: chunk missing" % name)
    if data is None:
        raise ValueError("%s: data: chunk missing" % name)
    tag, channels, rate, _, block_align, bits = struct.unpack_from("<HHIIHH", buf, fmt[0])
    if tag == 0xFFFE:
        if fmt[1] != 40:
            raise ValueError("%s: fmt: an extensible format in a chunk of %d bytes" % (name, fmt[1]))
        valid_bits = struct.unpack_from("<H", buf, fmt[0] + 18)[0]
        guid = bytes(buf[fmt[0] + 24:fmt[0] + 40])
        sub = struct.unpack_from("<H", guid, 0)[0]
        if guid[2:] != _GUID_TAIL or sub not in (1, 3):
            raise ValueError("%s: sub_format = %s: the PCM and IEEE-float sub-formats are served" % (name, guid.hex()))
        if valid_bits not in (0, bits):
            raise ValueError("%s: valid_bits = %d in a container of %d bits" % (name, valid_bits, bits))
        tag = sub
    if tag not in (1, 3):
        raise ValueError("%s: format_tag = 0x%04X: PCM (1), IEEE float (3) and extensible (0xFFFE) are served%s" % (
            name, tag, {6: " (A-law is not)", 7: " (mu-law is not)"}.get(tag, "")))
    kind = (_PCM_KINDS if tag == 1 else _FLOAT_KINDS).get(bits)
    if kind is None:
        raise ValueError("%s: bits = %d: %s" % (name, bits, "PCM of 8, 16, 24 or 32 bits is served" if tag == 1 else
                                                "IEEE float of 32 or 64 bits is served"))
    if not 1 <= channels <= MAX_CHANNELS:
        raise ValueError("%s: channels = %d: 1 to %d are served" % (name, channels, MAX_CHANNELS))
    if block_align != channels * KIND_BYTES[kind]:
        raise ValueError("%s: block_align = %d for %d channel(s) of %d bytes" % (name, block_align, channels, KIND_BYTES[kind]))
    if rate < 1:
        raise ValueError("%s: sample_rate = %d" % (name, rate))
    frames = data[1] // block_align
    if frames == 0:
        raise ValueError("%s: frames = 0: the data chunk holds no whole frame" % name)
    return WavInfo(kind, channels, rate, bits, block_align, frames, data[0])


class WavSource:
    """``.wav`` files as payload rows, after the pattern of flac.FlacSource."""

    def __init__(self, paths, target_sr=resample.TARGET_SR):
        self.files = list(paths)
        self.target_sr = int(target_sr)

    def __len__(self):
        return len(self.files)

    def path(self, i):
        return self.files[i]

    def take(self, keep):
        self.files = [self.files[i] for i in keep]

    def item(self, i):
        """(the whole frames of file i's ``data`` chunk as a uint8 tensor, its WavInfo).  ValueError, naming the file,
        for a rate the resampler does not serve."""
        with open(self.files[i], "rb") as f:
            buf = f.read()
        info = parse(buf, self.files[i])
        resample.geometry(info.sample_rate, self.target_sr, self.files[i])
        row = np.frombuffer(buf, dtype=np.uint8, count=info.frames * info.block_align, offset=info.data_offset).copy()
        return torch.from_numpy(row), info


def pack(items, bytes_round=65536, target_sr=resample.TARGET_SR):
    """[(payload uint8, WavInfo), ...] -> (bytes, byte_off, frames, fmt, rate, lengths).  ``bytes`` / ``byte_off``:
    ``flac.pack_rows``.  ``frames`` / ``fmt`` (int32, B): the rows' frame counts and format codes.  ``rate``: a TUPLE of
    the rows' source rates in Hz - host integers, which pass through DevicePrefetcher untouched, so the decoder picks the
    rows' tables without reading device memory.  ``lengths`` (int32, B): the OUTPUT lengths ceil(n L / M), from the
    headers alone - nothing downstream has to wait for the device to learn them.  ValueError for more than 8 distinct
    rates or a rate the resampler does not serve."""
    if not items:
        raise ValueError("pack() needs at least one row")
    rate = tuple(int(i.sample_rate) for _, i in items)
    resample.distinct(rate)
    lengths = [resample.out_length(int(i.frames), int(i.sample_rate), target_sr) for _, i in items]
    for row, i in items:
        if int(row.numel()) != int(i.frames) * int(i.block_align):
            raise ValueError("a row of %d bytes for %d frames of %d bytes" % (row.numel(), i.frames, i.block_align))
    buf, off = flac.pack_rows([row for row, _ in items], bytes_round)
    frames = torch.tensor([int(i.frames) for _, i in items], dtype=torch.int32)
    fmt = torch.tensor([fmt_code(i.kind, i.channels) for _, i in items], dtype=torch.int32)
    return buf, off, frames, fmt, rate, torch.tensor(lengths, dtype=torch.int32)


class WavDecoder(resample.RateBank):
    """The device decoder: format conversion, down-mix and resampling of a packed batch in one launch.  The per-rate
    coefficient tables are cached on the device (resample.RateBank)."""

    def decode(self, bytes_dev, byte_off, frames, fmt, rate, Lcap=None, dtype=torch.float32, check=False, out=None):
        """-> (pcm (B, Lcap) float32 | int16, status (B,) int32), both on the device.  float32 is what a libsndfile float
        read gives (s16: sample / 32768), mixed down and resampled to ``target_sr``; int16 the saturating round-half-even
        of 32768 x that - for a 16-bit mono file at the target rate the file's samples.  Tails beyond the row's output
        length are zero.  Never synchronises when ``Lcap`` is given; ``Lcap=None`` takes the longest output row rounded up
        to RAGGED_ROUND, which reads ``frames`` (a copy if they live on the device).  ``check=True`` calls
        ``check(status)`` (synchronous)."""
        B = int(frames.shape[0])
        if byte_off.shape[0] != B + 1 or fmt.shape[0] != B:
            raise ValueError("byte_off has B + 1 entries, frames and fmt B")
        rate = resample.rate_list(rate, B)
        desc, idx, _, _, tables, used = self.plan(rate)
        if Lcap is None:
            Lcap = ragged.round_capacity(max(self.host_lengths(frames.detach().cpu().tolist(), rate)))
        Lcap = int(Lcap)
        dev = self.device
        byte_off, frames, fmt = (t.to(dev, non_blocking=True) for t in (byte_off, frames, fmt))
        pcm, status, p16, p32 = self._output(B, Lcap, dtype, out)
        _hip.check(_hip.lib().air_wav_decode(
            _hip.dptr(bytes_dev, torch.uint8), _hip.csz(int(bytes_dev.numel())), _hip.dptr(byte_off, torch.int32),
            _hip.dptr(frames, torch.int32), _hip.dptr(fmt, torch.int32), _hip.dptr(idx, torch.int32), _hip.ci(B),
            ctypes.byref(desc), _hip.dptr(tables), _hip.csz(used), p16, p32, _hip.ci(Lcap),
            _hip.dptr(status, torch.int32), _hip.stream()), "air_wav_decode")
        if check:
            self.check(status)
        return pcm, status

    @staticmethod
    def check(status):
        """Copy ``status`` to the host (synchronises) and raise WavError listing the rows that are not OK.  Once per
        epoch over the concatenated statuses is enough."""
        ragged.check_status(status, OK, WavError)


def check(status):
    WavDecoder.check(status)
