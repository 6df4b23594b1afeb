"""FLAC oracle written from the format document (RFC 9639): an encoder whose every choice the caller can make, and the
plain serial decoder.  Mono, 16 bit, fixed block size - the subset the device decoder serves (include/air_hip.h).

``encode(samples, blocksize, frames=[...])`` writes a complete stream (marker, STREAMINFO with the MD5 of the samples,
frames with correct CRC-8 / CRC-16).  ``frames`` is a list of per-frame specs, cycled over the frames; a spec is a dict:

    type        "constant" | "verbatim" | "fixed" | "lpc"            (default "fixed")
    order       predictor order (fixed 0..4, lpc 1..32)               (default 2; lpc: len(coefs))
    coefs, precision, shift        the LPC predictor, as written into the subframe
    wasted      wasted bits k: every sample of the frame must be a multiple of 2**k
    method      0 RICE (4-bit parameters) | 1 RICE2 (5-bit)           (default 0)
    partition_order               (default 0)
    params      per partition: a Rice parameter, ("esc", n) for an escape partition of raw n-bit values, or None for
                the cheapest parameter; one value stands for every partition          (default None)
    bs_code     force the header's block-size code: 6 (8-bit explicit) or 7 (16-bit explicit)
    sr_code     the header's sample-rate code (default 5 = 16 kHz; 0 = from STREAMINFO, 12 / 13 / 14 explicit forms)
    size_code   the header's sample-size code: 4 (16 bit, default) or 0 (from STREAMINFO)
    channel_code, unchecked       for streams OUTSIDE the served subset: the header's channel assignment (default 0 =
                mono); unchecked=True lets precision 16 (code 1111) and a negative shift through

A frame shorter than its spec's predictor order (the short last frame) is written VERBATIM.
``decode(buf)`` returns the int16 samples and raises ValueError on a CRC or MD5 mismatch.
"""
import hashlib

import numpy as np

FIXED_COEFS = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}
SR_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}


def _crc_table(poly, bits):
    top, mask = 1 << (bits - 1), (1 << bits) - 1
    tab = []
    for i in range(256):
        c = i << (bits - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        tab.append(c)
    return tab


_CRC8 = _crc_table(0x07, 8)
_CRC16 = _crc_table(0x8005, 16)


def crc8(data):
    c = 0
    for b in bytes(data):
        c = _CRC8[c ^ b]
    return c


def crc16(data):
    c = 0
    for b in bytes(data):
        c = ((c << 8) & 0xFFFF) ^ _CRC16[(c >> 8) ^ b]
    return c


# ------------------------------------------------------------------------------------------------ bit writer
class BitWriter:
    def __init__(self):
        self.parts = []

    def write(self, value, nbits):
        if nbits:
            v = int(value) & ((1 << nbits) - 1)
            self.parts.append(np.array([(v >> s) & 1 for s in range(nbits - 1, -1, -1)], dtype=np.uint8))

    def write_many(self, values, nbits):
        """Each of `values` as an nbits two's-complement field."""
        if nbits and len(values):
            v = np.asarray(values, dtype=np.int64) & ((1 << nbits) - 1)
            sh = np.arange(nbits - 1, -1, -1, dtype=np.int64)
            self.parts.append(((v[:, None] >> sh) & 1).astype(np.uint8).reshape(-1))

    def write_rice(self, residuals, k):
        r = np.asarray(residuals, dtype=np.int64)
        if not len(r):
            return
        u = np.where(r >= 0, 2 * r, -2 * r - 1)
        q = u >> k
        width = q + 1 + k
        start = np.concatenate(([0], np.cumsum(width)[:-1]))
        bits = np.zeros(int(width.sum()), dtype=np.uint8)
        bits[start + q] = 1
        for j in range(k):
            bits[start + q + 1 + j] = (u >> (k - 1 - j)) & 1
        self.parts.append(bits)

    def nbits(self):
        return sum(len(p) for p in self.parts)

    def align(self):
        pad = -self.nbits() % 8
        if pad:
            self.parts.append(np.zeros(pad, dtype=np.uint8))

    def tobytes(self):
        self.align()
        return np.packbits(np.concatenate(self.parts)).tobytes() if self.parts else b""


def utf8_number(v):
    if v < 0x80:
        return bytes([v])
    for n, lead in ((2, 0xC0), (3, 0xE0), (4, 0xF0), (5, 0xF8), (6, 0xFC), (7, 0xFE)):
        if v < 1 << (5 * n + 1 if n < 7 else 36):
            out = [0x80 | ((v >> (6 * i)) & 0x3F) for i in range(n - 1)][::-1]
            return bytes([lead | (v >> (6 * (n - 1)))] + out)
    raise ValueError("frame number too large")


def _bs_code(n):
    if n == 192:
        return 1
    for c in range(2, 6):
        if n == 576 << (c - 2):
            return c
    for c in range(8, 16):
        if n == 256 << (c - 8):
            return c
    return 6 if n <= 256 else 7


def best_rice(residuals, kmax=14):
    r = np.asarray(residuals, dtype=np.int64)
    if not len(r):
        return 0
    u = np.where(r >= 0, 2 * r, -2 * r - 1)
    cost = [int((u >> k).sum()) + (k + 1) * len(u) for k in range(kmax + 1)]
    return int(np.argmin(cost))


def residual_of(s, coefs, shift):
    """s (int64) -> residual of samples order .. n-1 under the predictor sum c[j] s[i-1-j] >> shift (arithmetic)."""
    order, n = len(coefs), len(s)
    pred = np.zeros(n - order, dtype=np.int64)
    for j, c in enumerate(coefs):
        pred += int(c) * s[order - 1 - j:n - 1 - j]
    return s[order:] - (pred >> max(shift, 0))  # (a negative shift is outside the subset: only `unchecked` writes one)


def encode_frame(samples, frame_number, spec=None, sample_rate=16000):
    """One frame (header .. CRC-16) of the int samples under `spec`."""
    spec = dict(spec or {})
    s = np.asarray(samples, dtype=np.int64)
    n = len(s)
    assert 1 <= n <= 65536
    hdr = bytearray([0xFF, 0xF8])
    bsc = spec.get("bs_code") or _bs_code(n)
    src = spec.get("sr_code", SR_CODES.get(sample_rate, 0))
    hdr.append((bsc << 4) | src)
    hdr.append((spec.get("channel_code", 0) << 4) | (spec.get("size_code", 4) << 1))
    hdr += utf8_number(frame_number)
    if bsc == 6:
        assert n <= 256
        hdr.append(n - 1)
    elif bsc == 7:
        hdr += (n - 1).to_bytes(2, "big")
    else:
        assert _bs_code(n) == bsc
    if src == 12:
        hdr.append(sample_rate // 1000)
    elif src == 13:
        hdr += sample_rate.to_bytes(2, "big")
    elif src == 14:
        hdr += (sample_rate // 10).to_bytes(2, "big")
    hdr.append(crc8(hdr))

    w = BitWriter()
    kind = spec.get("type", "fixed")
    wasted = int(spec.get("wasted", 0))
    if wasted:
        assert not np.any(s & ((1 << wasted) - 1)), "samples are not multiples of 2**wasted"
        s = s >> wasted
    bps = 16 - wasted
    assert np.all(s >= -(1 << (bps - 1))) and np.all(s < (1 << (bps - 1)))
    if kind == "lpc":
        coefs = [int(c) for c in spec["coefs"]]
        order = len(coefs)
    elif kind == "fixed":
        order = int(spec.get("order", 2))
        coefs = FIXED_COEFS[order]
    else:
        order, coefs = 0, []
    if kind in ("fixed", "lpc") and n < order:
        kind = "verbatim"
    code = {"constant": 0, "verbatim": 1}.get(kind)
    if code is None:
        code = 8 + order if kind == "fixed" else 31 + order
    w.write(0, 1)
    w.write(code, 6)
    w.write(1 if wasted else 0, 1)
    if wasted:
        w.write(1, wasted)  # unary: wasted - 1 zeros, then a one
    if kind == "constant":
        assert np.all(s == s[0])
        w.write(s[0], bps)
    elif kind == "verbatim":
        w.write_many(s, bps)
    else:
        w.write_many(s[:order], bps)
        shift = 0
        if kind == "lpc":
            prec, shift = int(spec["precision"]), int(spec["shift"])
            assert 1 <= order <= 32
            assert spec.get("unchecked") or (1 <= prec <= 15 and 0 <= shift <= 31)
            assert all(-(1 << (prec - 1)) <= c < (1 << (prec - 1)) for c in coefs)
            w.write(prec - 1, 4)
            w.write(shift, 5)
            w.write_many(coefs, prec)
        res = residual_of(s, coefs, shift)
        assert np.all(np.abs(res) < (1 << 31))
        method = int(spec.get("method", 0))
        po = int(spec.get("partition_order", 0))
        psize = n >> po
        assert psize << po == n and psize >= order, "partition order does not fit the block"
        params = spec.get("params")
        if not isinstance(params, list):
            params = [params] * (1 << po)
        assert len(params) == 1 << po
        w.write(method, 2)
        w.write(po, 4)
        pbits, esc = (5, 31) if method else (4, 15)
        at = 0
        for part, prm in enumerate(params):
            cnt = psize - order if part == 0 else psize
            r = res[at:at + cnt]
            at += cnt
            if isinstance(prm, tuple):
                nb = int(prm[1])
                assert prm[0] == "esc" and 0 <= nb <= 31
                if nb == 0:
                    assert not np.any(r)
                else:
                    assert np.all(r >= -(1 << (nb - 1))) and np.all(r < (1 << (nb - 1)))
                w.write(esc, pbits)
                w.write(nb, 5)
                w.write_many(r, nb)
            else:
                k = best_rice(r, esc - 1) if prm is None else int(prm)
                assert 0 <= k < esc
                w.write(k, pbits)
                w.write_rice(r, k)
    body = bytes(hdr) + w.tobytes()
    return body + crc16(body).to_bytes(2, "big")


def streaminfo(min_bs, max_bs, min_fs, max_fs, sample_rate, channels, bps, total, md5):
    v = (min_bs << 16 | max_bs) << 24 | min_fs
    v = (v << 24 | max_fs) << 20 | sample_rate
    v = ((v << 3 | (channels - 1)) << 5 | (bps - 1)) << 36 | total
    return v.to_bytes(18, "big") + md5


def metadata_block(kind, payload, last):
    return bytes([(0x80 if last else 0) | kind]) + len(payload).to_bytes(3, "big") + payload


def pcm_md5(samples):
    return hashlib.md5(np.asarray(samples, dtype="<i2").tobytes()).digest()


def encode(samples, blocksize, frames=None, sample_rate=16000, extra_blocks=(), info=None):
    """A complete FLAC stream.  extra_blocks: (type, payload) metadata blocks behind STREAMINFO; info: overrides of
    STREAMINFO fields (min_bs, max_bs, channels, bps, total, sample_rate) for streams the host parser must refuse."""
    s = np.asarray(samples)
    assert s.ndim == 1 and len(s) >= 1
    s = s.astype(np.int64)
    specs = list(frames) if frames else [None]
    out = []
    for f, at in enumerate(range(0, len(s), blocksize)):
        out.append(encode_frame(s[at:at + blocksize], f, specs[f % len(specs)], sample_rate))
    fields = dict(min_bs=blocksize, max_bs=blocksize, min_fs=min(map(len, out)), max_fs=max(map(len, out)),
                  sample_rate=sample_rate, channels=1, bps=16, total=len(s), md5=pcm_md5(s))
    fields.update(info or {})
    blocks = [(0, streaminfo(**fields))] + list(extra_blocks)
    head = b"fLaC" + b"".join(metadata_block(k, p, i == len(blocks) - 1) for i, (k, p) in enumerate(blocks))
    return head + b"".join(out)


# ------------------------------------------------------------------------------------------------ serial decoder
class BitReader:
    def __init__(self, buf, pos):
        self.buf, self.bit = bytes(buf), pos * 8

    def read(self, n):
        if n == 0:
            return 0
        if self.bit + n > 8 * len(self.buf):
            raise ValueError("read past the end of the stream")
        byte, off = self.bit >> 3, self.bit & 7
        chunk = int.from_bytes(self.buf[byte:byte + 8].ljust(8, b"\0"), "big")
        self.bit += n
        return (chunk >> (64 - off - n)) & ((1 << n) - 1)

    def read_signed(self, n):
        v = self.read(n)
        return v - (1 << n) if n and v >> (n - 1) else v

    def unary(self):
        q = 0
        while True:
            n = min(32, 8 * len(self.buf) - self.bit)
            if n <= 0:
                raise ValueError("unary run past the end of the stream")
            v = self.read(n)
            if v:
                z = n - v.bit_length()
                self.bit -= n - z - 1
                return q + z
            q += n

    def align(self):
        self.bit = (self.bit + 7) & ~7


def decode_frame(buf, pos, info):
    """-> (samples list, frame number, end offset).  Raises ValueError on anything wrong."""
    r = BitReader(buf, pos)
    if r.read(15) != 0x7FFC:
        raise ValueError("no fixed-block-size sync at %d" % pos)
    if r.read(1):
        raise ValueError("variable-block-size frame at %d" % pos)
    bsc, src = r.read(4), r.read(4)
    ch, size, res = r.read(4), r.read(3), r.read(1)
    if ch != 0 or size not in (0, 4) or res or bsc == 0 or src == 15:
        raise ValueError("unsupported frame header at %d" % pos)
    c0 = r.read(8)
    extra = 0
    while c0 & (0x80 >> extra):
        extra += 1
    fn = c0 & (0x7F >> extra) if extra else c0
    for _ in range(max(extra - 1, 0)):
        c = r.read(8)
        if c & 0xC0 != 0x80:
            raise ValueError("bad frame number")
        fn = fn << 6 | (c & 0x3F)
    if bsc == 1:
        n = 192
    elif bsc <= 5:
        n = 576 << (bsc - 2)
    elif bsc == 6:
        n = r.read(8) + 1
    elif bsc == 7:
        n = r.read(16) + 1
    else:
        n = 256 << (bsc - 8)
    if src == 12:
        r.read(8)
    elif src in (13, 14):
        r.read(16)
    if crc8(buf[pos:r.bit >> 3]) != r.read(8):
        raise ValueError("CRC-8 mismatch at %d" % pos)
    if r.read(1):
        raise ValueError("subframe padding bit")
    code = r.read(6)
    wasted = r.unary() + 1 if r.read(1) else 0
    bps = 16 - wasted
    if code == 0:
        s = [r.read_signed(bps)] * n
    elif code == 1:
        s = [r.read_signed(bps) for _ in range(n)]
    elif 8 <= code <= 12 or code >= 32:
        order = code - 8 if code < 32 else code - 31
        s = [r.read_signed(bps) for _ in range(order)]
        shift, coefs = 0, FIXED_COEFS.get(order)
        if code >= 32:
            prec = r.read(4) + 1
            shift = r.read_signed(5)
            if prec == 16 or shift < 0:
                raise ValueError("unsupported LPC parameters")
            coefs = [r.read_signed(prec) for _ in range(order)]
        method = r.read(2)
        if method > 1:
            raise ValueError("reserved residual coding method")
        po = r.read(4)
        psize = n >> po
        if psize << po != n or psize < order:
            raise ValueError("bad partition order")
        pbits, esc = (5, 31) if method else (4, 15)
        for part in range(1 << po):
            cnt = psize - order if part == 0 else psize
            k = r.read(pbits)
            nb = r.read(5) if k == esc else None
            for _ in range(cnt):
                if nb is not None:
                    res = r.read_signed(nb)
                else:
                    u = r.unary() << k | r.read(k)
                    res = (u >> 1) ^ -(u & 1)
                i = len(s)
                s.append(res + (sum(c * s[i - 1 - j] for j, c in enumerate(coefs)) >> shift))
    else:
        raise ValueError("reserved subframe type %d" % code)
    r.align()
    end = r.bit >> 3
    if crc16(buf[pos:end]) != r.read(16):
        raise ValueError("CRC-16 mismatch in the frame at %d" % pos)
    return [v << wasted for v in s], fn, end + 2


def read_streaminfo(buf):
    """-> (dict of STREAMINFO fields, offset of the first frame)."""
    if buf[:4] != b"fLaC":
        raise ValueError("no fLaC marker")
    pos, info = 4, None
    while True:
        last, kind = buf[pos] >> 7, buf[pos] & 0x7F
        size = int.from_bytes(buf[pos + 1:pos + 4], "big")
        if kind == 0:
            v = int.from_bytes(buf[pos + 4:pos + 22], "big")
            info = dict(total=v & (1 << 36) - 1, bps=(v >> 36 & 31) + 1, channels=(v >> 41 & 7) + 1,
                        sample_rate=v >> 44 & 0xFFFFF, max_fs=v >> 64 & 0xFFFFFF, min_fs=v >> 88 & 0xFFFFFF,
                        max_bs=v >> 112 & 0xFFFF, min_bs=v >> 128 & 0xFFFF, md5=bytes(buf[pos + 22:pos + 38]))
        pos += 4 + size
        if last:
            return info, pos


def decode(buf):
    buf = bytes(buf)
    info, pos = read_streaminfo(buf)
    out, expect = [], 0
    while pos < len(buf):
        s, fn, pos = decode_frame(buf, pos, info)
        if fn != expect:
            raise ValueError("frame number %d where %d was expected" % (fn, expect))
        expect += 1
        out += s
    pcm = np.array(out, dtype=np.int64)
    if len(pcm) != info["total"]:
        raise ValueError("%d samples, STREAMINFO says %d" % (len(pcm), info["total"]))
    if np.any(pcm < -32768) or np.any(pcm > 32767):
        raise ValueError("sample outside 16 bits")
    pcm = pcm.astype(np.int16)
    if pcm_md5(pcm) != info["md5"]:
        raise ValueError("MD5 mismatch")
    return pcm


def audio_frames(buf):
    """The stream's audio frames (metadata stripped)."""
    return bytes(buf)[read_streaminfo(bytes(buf))[1]:]
