"""Reading the corpus: ``.flac`` files -> ragged PCM batches, decoded on the GPU.

The reference reads a waveform with ``librosa.load`` / ``sf.read`` (raw_dataset.py:20-28).  Here the host only parses the
few dozen bytes of metadata (``parse_stream``) and ships the COMPRESSED audio frames; ``FlacDecoder.decode`` locates and
decodes the frames of a whole batch on the device (csrc/flac.hip) into the (B, Lcap) layout ``_collate_ragged`` produces
and ``Trainer.step(pcm, labels, start=, lengths=)`` / ``LFCC.forward_ragged`` read.  The arithmetic is integer, the samples
are the encoder's bit for bit; ``verify_md5`` holds a decoded row against the MD5 its encoder stored in STREAMINFO.

Served: 16-bit mono streams of one block size (what the ASVspoof 2019 / 2021 corpora ship).  ``parse_stream`` refuses
everything else on the host, by name; the device reports per row what it could not decode (``STATUS``), never faults.
"""
import collections
import hashlib

import numpy as np
import torch

from . import _hip
from .ragged import RAGGED_ROUND, DeviceRing, PinnedRing, check_status, round_capacity  # noqa: F401  (RAGGED_ROUND: re-exported)

FlacInfo = collections.namedtuple("FlacInfo", "min_blocksize max_blocksize min_framesize max_framesize sample_rate "
                                  "channels bits_per_sample total_samples md5 audio_offset")

# status codes of include/air_hip.h (AIR_FLAC_*)
OK, LOST_SYNC, BAD_CRC16, UNSUPPORTED, LENGTH_MISMATCH, CANDIDATE_OVERFLOW = range(6)
STATUS = {OK: "OK", LOST_SYNC: "LOST_SYNC", BAD_CRC16: "BAD_CRC16", UNSUPPORTED: "UNSUPPORTED",
          LENGTH_MISMATCH: "LENGTH_MISMATCH", CANDIDATE_OVERFLOW: "CANDIDATE_OVERFLOW"}


class FlacError(RuntimeError):
    """Rows of a batch the device could not decode: ``rows`` = [(row, status code), ...]."""

    def __init__(self, rows):
        self.rows = list(rows)
        super().__init__("FLAC decode failed for %d row(s): %s" % (
            len(self.rows), ", ".join("row %d %s" % (r, STATUS.get(c, "status %d" % c)) for r, c in self.rows)))


def parse_stream(buf, name="<buffer>"):
    """The ``fLaC`` marker and the metadata blocks of a stream -> FlacInfo (STREAMINFO and the offset of the first audio
    frame).  ValueError, naming the file and the field, for what the device path does not serve."""
    buf = memoryview(buf).cast("B") if not isinstance(buf, (bytes, bytearray)) else buf
    if len(buf) < 4 or bytes(buf[:4]) != b"fLaC":
        raise ValueError("%s: marker: not a FLAC stream (no 'fLaC' at offset 0)" % name)
    pos, info = 4, None
    while True:
        if pos + 4 > len(buf):
            raise ValueError("%s: STREAMINFO: metadata truncated at byte %d" % (name, pos))
        last, kind = buf[pos] >> 7, buf[pos] & 0x7F
        size = int.from_bytes(bytes(buf[pos + 1:pos + 4]), "big")
        if pos == 4 and (kind != 0 or size < 34):
            raise ValueError("%s: STREAMINFO: the first metadata block is not a STREAMINFO block" % name)
        if pos + 4 + size > len(buf):
            raise ValueError("%s: STREAMINFO: metadata block of %d bytes truncated at byte %d" % (name, size, pos))
        if kind == 0 and info is None:
            v = int.from_bytes(bytes(buf[pos + 4:pos + 22]), "big")
            info = dict(total_samples=v & ((1 << 36) - 1), bits_per_sample=((v >> 36) & 31) + 1,
                        channels=((v >> 41) & 7) + 1, sample_rate=(v >> 44) & 0xFFFFF,
                        max_framesize=(v >> 64) & 0xFFFFFF, min_framesize=(v >> 88) & 0xFFFFFF,
                        max_blocksize=(v >> 112) & 0xFFFF, min_blocksize=(v >> 128) & 0xFFFF,
                        md5=bytes(buf[pos + 22:pos + 38]))
        pos += 4 + size
        if last:
            break
    if info is None:
        raise ValueError("%s: STREAMINFO: absent" % name)
    if info["channels"] != 1:
        raise ValueError("%s: channels = %d: the device decoder serves mono streams" % (name, info["channels"]))
    if info["bits_per_sample"] != 16:
        raise ValueError("%s: bits_per_sample = %d: the device decoder serves 16-bit streams" % (name, info["bits_per_sample"]))
    if info["total_samples"] == 0:
        raise ValueError("%s: total_samples = 0 (length unknown): the row capacity comes from STREAMINFO" % name)
    if info["min_blocksize"] != info["max_blocksize"]:
        raise ValueError("%s: min_blocksize = %d != max_blocksize = %d: a variable-block-size stream" % (
            name, info["min_blocksize"], info["max_blocksize"]))
    return FlacInfo(audio_offset=pos, **info)


class FlacSource:
    """``.flac`` files as compressed rows, after the pattern of dataset.PCMSource / FileSource."""

    def __init__(self, paths):
        self.files = list(paths)

    def __len__(self):
        return len(self.files)

    def path(self, i):
        return self.files[i]

    def take(self, keep):
        self.files = [self.files[i] for i in keep]

    def item(self, i):
        """(audio-frame bytes of file i as a uint8 tensor, metadata stripped; its FlacInfo)."""
        with open(self.files[i], "rb") as f:
            buf = f.read()
        info = parse_stream(buf, self.files[i])
        return torch.from_numpy(np.frombuffer(buf, dtype=np.uint8, offset=info.audio_offset).copy()), info


PINNED_RING = 6
_pin_ring = PinnedRing(PINNED_RING)


def _pinned_bytes(cap):
    """A pinned uint8 buffer out of the module's ring, per capacity."""
    return _pin_ring.take(cap, cap, torch.uint8)


def pack_rows(rows, bytes_round=65536):
    """[uint8 row, ...] -> (bytes, byte_off): the rows back to back in one pinned 1-D uint8 tensor whose capacity is a
    multiple of ``bytes_round`` (DevicePrefetcher's ring is keyed by shape: no allocation per batch), every row starting
    4-byte aligned.  ``byte_off`` (int32, B + 1): row b occupies ``[(byte_off[b] + 3) & ~3, byte_off[b + 1])`` -
    byte_off[b + 1] is the exact end of row b, the next row starts at the next multiple of 4.  (wav.pack shares it.)"""
    if not rows:
        raise ValueError("pack() needs at least one row")
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    for b, row in enumerate(rows):
        off[b + 1] = ((off[b] + 3) & ~3) + int(row.numel())
    used = int(off[-1])
    if used > 2 ** 31 - 1:
        raise ValueError("a batch of %d compressed bytes exceeds the int32 offsets" % used)
    cap = max(1, -(-used // int(bytes_round))) * int(bytes_round)
    buf = _pinned_bytes(cap)
    dst = buf.numpy()
    for b, row in enumerate(rows):
        s = (int(off[b]) + 3) & ~3
        dst[int(off[b]):s] = 0
        dst[s:int(off[b + 1])] = row.numpy()
    dst[used:] = 0
    return buf, torch.from_numpy(off.astype(np.int32))


def pack(items, bytes_round=65536):
    """[(frame bytes uint8, FlacInfo), ...] -> (bytes, byte_off, lengths, blocksize): ``pack_rows`` of the rows (the
    chain of frames has to end at byte_off[b + 1]); ``lengths`` / ``blocksize`` (int32, B) from STREAMINFO."""
    buf, off = pack_rows([row for row, _ in items], bytes_round)
    lengths = torch.tensor([int(i.total_samples) for _, i in items], dtype=torch.int32)
    blocksize = torch.tensor([int(i.max_blocksize) for _, i in items], dtype=torch.int32)
    return buf, off, lengths, blocksize


class FlacDecoder(DeviceRing):
    """The device decoder.  Output, status and workspace tensors come out of a ring of ``depth`` slots per shape
    (``ragged.DeviceRing``)."""

    def __init__(self, device="cuda", depth=4):
        super().__init__(device, depth)

    def decode(self, bytes_dev, byte_off, lengths, blocksize, Lcap=None, dtype=torch.int16, check=False, out=None):
        """-> (pcm (B, Lcap) int16 | float32 = sample / 32768, status (B,) int32), both on the device.  Tails beyond
        ``lengths[b]`` are zero.  Never synchronises when ``Lcap`` is given (training: a fixed capacity, as
        ``ragged_samples``); ``Lcap=None`` takes the longest length rounded up to RAGGED_ROUND, which reads ``lengths``
        (a copy if they live on the device).  ``check=True`` calls ``check(status)`` (synchronous).  ``out``: a
        contiguous (B, Lcap) device tensor of ``dtype`` to decode into instead of the ring's."""
        L = _hip.lib()
        B = int(lengths.shape[0])
        if byte_off.shape[0] != B + 1 or blocksize.shape[0] != B:
            raise ValueError("byte_off has B + 1 entries, lengths and blocksize B")
        if Lcap is None:
            Lcap = round_capacity(lengths.max())
        Lcap = int(Lcap)
        dev = self.device
        byte_off, lengths, blocksize = (t.to(dev, non_blocking=True) for t in (byte_off, lengths, blocksize))
        total = int(bytes_dev.numel())
        ws_bytes = L.air_flac_workspace_bytes(_hip.csz(total), _hip.ci(B))
        pcm, status, p16, p32 = self._output(B, Lcap, dtype, out)
        ws = self._slot(("ws", ws_bytes), lambda: torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev))
        _hip.check(L.air_flac_decode(_hip.dptr(bytes_dev, torch.uint8), _hip.csz(total), _hip.dptr(byte_off, torch.int32),
                                     _hip.dptr(lengths, torch.int32), _hip.dptr(blocksize, torch.int32), _hip.ci(B),
                                     _hip.ci(Lcap), p16, p32, _hip.dptr(status, torch.int32), _hip.dptr(ws, torch.uint8),
                                     _hip.csz(ws_bytes), _hip.stream()), "air_flac_decode")
        if check:
            self.check(status)
        return pcm, status

    @staticmethod
    def check(status):
        """Copy ``status`` to the host (synchronises) and raise FlacError listing the rows that are not OK.  Once per
        epoch over the concatenated statuses is enough."""
        check_status(status, OK, FlacError)


def check(status):
    FlacDecoder.check(status)


def verify_md5(pcm_row, info):
    """True when the MD5 of the row's first ``info.total_samples`` int16 samples (little-endian, as the format defines
    it) is the one the encoder stored in STREAMINFO.  This is the check that holds on files from a real encoder: the
    tests here pin the decoder against an oracle written from the format document, not against libFLAC."""
    row = pcm_row.detach().cpu().reshape(-1)[:int(info.total_samples)]
    if row.dtype != torch.int16:
        raise ValueError("verify_md5 takes the int16 samples")
    return hashlib.md5(row.numpy().astype("<i2").tobytes()).digest() == bytes(info.md5)
