"""WAV files for the tests, written from the format description (RIFF: 'RIFF' <u32 size> 'WAVE', then chunks of
<4-byte id> <u32 size> <body> padded to an even length; 'fmt ' = tag, channels, rate, bytes / s, block align, bits
[, cbSize [, valid bits, channel mask, 16-byte sub-format GUID]]; 'data' = interleaved little-endian frames).  The
standard library's ``wave`` module is the independent writer and reader for PCM of 8 / 16 / 24 / 32 bits.

Samples are kept as the file's own numbers (``raw``: (n, C) uint8 / int16 / int32 / float32 / float64); ``to_float``
states what a libsndfile float read returns for them, ``mono`` the reference's down-mix (librosa: np.mean(y.T, axis=0))."""
import io
import struct
import wave

import numpy as np

U8, S16, S24, S32, F32, F64 = range(6)
KINDS = {"u8": U8, "s16": S16, "s24": S24, "s32": S32, "f32": F32, "f64": F64}
BYTES = {U8: 1, S16: 2, S24: 3, S32: 4, F32: 4, F64: 8}
GUID_TAIL = bytes([0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71])


def signal(n, seed, C=1, amp=0.5, sr=16000):
    """(n, C) float64: seeded noise at ``amp`` full scale plus a 3 kHz tone (0.25), a different phase per channel."""
    rng = np.random.RandomState(seed)
    t = np.arange(n)[:, None] / float(sr)
    return amp * (2.0 * rng.rand(n, C) - 1.0) + 0.25 * np.sin(2 * np.pi * 3000.0 * t + np.arange(C)[None, :])


def quantise(x, kind):
    """float64 in about [-1, 1] -> the file's numbers for ``kind``."""
    x = np.asarray(x, dtype=np.float64)
    if kind == U8:
        return np.clip(np.round(x * 128.0) + 128, 0, 255).astype(np.uint8)
    if kind == S16:
        return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    if kind == S24:
        return np.clip(np.round(x * 8388608.0), -8388608, 8388607).astype(np.int32)
    if kind == S32:
        return np.clip(np.round(x * 2147483648.0), -2147483648, 2147483647).astype(np.int64).astype(np.int32)
    return x.astype(np.float32 if kind == F32 else np.float64)


def encode(raw, kind):
    """The ``data`` payload of (n, C) ``raw``."""
    raw = np.ascontiguousarray(raw)
    if kind == S24:
        b = raw.astype("<i4").reshape(-1, 1).view(np.uint8).reshape(-1, 4)[:, :3]
        return np.ascontiguousarray(b).tobytes()
    return raw.astype({U8: "u1", S16: "<i2", S32: "<i4", F32: "<f4", F64: "<f8"}[kind]).tobytes()


def to_float(raw, kind):
    """(n, C) float32: u8 (v - 128) / 128, s16 v / 2^15, s24 v / 2^23, s32 v / 2^31, f32 as is, f64 rounded."""
    if kind == U8:
        return (raw.astype(np.float32) - np.float32(128)) / np.float32(128)
    if kind in (S16, S24, S32):
        return raw.astype(np.float32) / np.float32(2.0 ** {S16: 15, S24: 23, S32: 31}[kind])
    return raw.astype(np.float32)


def mono(f):
    """(n, C) float32 -> (n,) float32: the only channel, or np.mean(frames.T, axis=0) in float32."""
    f = np.asarray(f, dtype=np.float32)
    if f.shape[1] == 1:
        return f[:, 0].copy()
    out = np.mean(f.T, axis=0)
    assert out.dtype == np.float32
    return out


def chunk(cid, body):
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def fmt_body(kind, channels, rate, size=16, extensible=False, tag=None, bits=None, block_align=None, guid=None, valid_bits=None):
    bps = BYTES[kind]
    bits = 8 * bps if bits is None else bits
    block_align = channels * bps if block_align is None else block_align
    base_tag = 3 if kind in (F32, F64) else 1
    if extensible:
        size = 40
    if tag is None:
        tag = 0xFFFE if extensible else base_tag
    body = struct.pack("<HHIIHH", tag, channels, rate, rate * block_align, block_align, bits)
    if size == 18:
        body += struct.pack("<H", 0)
    elif size == 40:
        body += struct.pack("<HHI", 22, bits if valid_bits is None else valid_bits, 0)
        body += guid if guid is not None else struct.pack("<H", base_tag) + GUID_TAIL
    return body


def wav_bytes(raw, kind, rate, before=(), between=(), after=(), data_first=False, data_size=None, riff=b"RIFF", **fmt_kw):
    """A whole file.  ``before`` / ``between`` / ``after``: extra (id, body) chunks in front of ``fmt ``, between ``fmt ``
    and ``data``, behind ``data``; ``data_first``: ``data`` ahead of ``fmt ``; ``data_size``: the size field of ``data``
    (the payload itself is written whole)."""
    raw = np.asarray(raw)
    if raw.ndim == 1:
        raw = raw[:, None]
    payload = encode(raw, kind)
    f = chunk(b"fmt ", fmt_body(kind, raw.shape[1], rate, **fmt_kw))
    d = chunk(b"data", payload)
    if data_size is not None:
        d = b"data" + struct.pack("<I", data_size) + payload
    parts = [chunk(c, b) for c, b in before]
    parts += [d] + [chunk(c, b) for c, b in between] + [f] if data_first else [f] + [chunk(c, b) for c, b in between] + [d]
    parts += [chunk(c, b) for c, b in after]
    body = b"WAVE" + b"".join(parts)
    return riff + struct.pack("<I", len(body)) + body


def wave_module_bytes(raw, kind, rate):
    """The same samples through the standard library's writer (PCM only)."""
    raw = np.asarray(raw)
    if raw.ndim == 1:
        raw = raw[:, None]
    bio = io.BytesIO()
    with wave.open(bio, "wb") as w:
        w.setnchannels(raw.shape[1])
        w.setsampwidth(BYTES[kind])
        w.setframerate(rate)
        w.writeframes(encode(raw, kind))
    return bio.getvalue()


def wave_module_read(buf):
    """(channels, rate, sample width, frames, payload) as the standard library reads the file."""
    with wave.open(io.BytesIO(buf), "rb") as w:
        return w.getnchannels(), w.getframerate(), w.getsampwidth(), w.getnframes(), w.readframes(w.getnframes())


# ---------------------------------------------------------------------------- the resampling rows of the GPU tests
TILE = 1024  # outputs per workgroup of csrc/resample.hip at every rate used here
RESAMPLE_RATES = [8000, 24000, 48000, 44100, 22050]  # L / M = 2/1, 2/3, 1/3, 160/441, 320/441
_rows = {}


def row_lengths(sr):
    """Input lengths: 1, 2, H - 1, H, H + 1 (rows shorter than the filter: the zero extension at both ends), the
    longest row of at most TILE - 1 outputs, the shortest of at least TILE and of at least TILE + 1 (the tile seam;
    when upsampling not every output count exists), and 7 samples beyond the shortest row of 3 tiles."""
    import resample_oracle as ro
    L, M, K = ro.geometry(sr)
    H = K // 2
    at_most = lambda t: t * M // L             # the largest n with ceil(n L / M) <= t
    at_least = lambda t: (t - 1) * M // L + 1  # the least n with ceil(n L / M) >= t
    out = [1, 2, H - 1, H, H + 1, at_most(TILE - 1), at_least(TILE), at_least(TILE + 1), at_least(3 * TILE) + 7]
    got = [ro.out_length(n, sr) for n in out]
    assert TILE - 3 <= got[5] <= TILE - 1 and TILE <= got[6] <= TILE + 1 < got[7] + 1 <= TILE + 3 and got[8] > 3 * TILE
    return out


def resample_rows(sr):
    """[(int16 row, oracle y, oracle bound), ...] for ``row_lengths(sr)``: seeded noise at 0.5 full scale plus a 3 kHz
    tone, quantised to 16 bits; the oracle runs on sample / 32768.  Computed once per rate."""
    import resample_oracle as ro
    if sr not in _rows:
        out = []
        for i, n in enumerate(row_lengths(sr)):
            x = quantise(signal(n, 1000 + i, 1, sr=sr), S16)[:, 0]
            y, bound = ro.resample(x.astype(np.float64) / 32768.0, sr)
            out.append((x, y, bound))
        _rows[sr] = out
    return _rows[sr]
