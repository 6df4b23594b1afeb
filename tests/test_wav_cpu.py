"""CPU: the host side of the WAV path - ``wav.parse`` against the standard library's ``wave`` module and against files
written from the format description (tests/wav_cases.py), ``wav.pack``, ``wav.WavSource``, and the six ``.wav`` classes of
``raw_dataset`` pinned against the reference's own classes (tests/golden/raw_wav.json, recorded by
tests/golden/make_golden_raw_wav.py over the tree of tests/raw_wav_fixture.py).  Nothing here touches a GPU."""
import json
import os
import struct

import numpy as np
import pytest
import torch

import raw_wav_fixture as fx
import resample_oracle as ro
import wav_cases as wc

HERE = os.path.dirname(os.path.abspath(__file__))


def _raw(kind, n=37, C=1, seed=1):
    return wc.quantise(wc.signal(n, seed, C), kind)


# ---------------------------------------------------------------------------- parse
@pytest.mark.parametrize("kind", ["u8", "s16", "s24", "s32"])
@pytest.mark.parametrize("C", [1, 2, 5])
def test_parse_agrees_with_the_wave_module(kind, C):
    from asvspoof2021_air_amd import wav
    k = wc.KINDS[kind]
    raw = _raw(k, 41, C, seed=C)
    for buf in (wc.wave_module_bytes(raw, k, 22050), wc.wav_bytes(raw, k, 22050)):
        ch, rate, width, frames, payload = wc.wave_module_read(buf)
        info = wav.parse(buf, "a.wav")
        assert (info.channels, info.sample_rate, info.bits, info.frames) == (ch, rate, 8 * width, frames) == (C, 22050, 8 * wc.BYTES[k], 41)
        assert info.kind == k and info.block_align == C * width
        assert bytes(buf[info.data_offset:info.data_offset + frames * info.block_align]) == payload == wc.encode(raw, k)
    assert wav.parse(memoryview(buf)) == wav.parse(np.frombuffer(buf, dtype=np.uint8)) == info


def test_parse_float_extensible_chunk_order_and_padding():
    from asvspoof2021_air_amd import wav
    odd = (b"LIST", b"abc")          # 3 bytes: padded to 4
    junk = (b"junk", b"\0" * 10)
    for kind, bits in ((wc.F32, 32), (wc.F64, 64)):
        raw = _raw(kind, 19, 2)
        for size in (16, 18):
            info = wav.parse(wc.wav_bytes(raw, kind, 44100, size=size))
            assert (info.kind, info.bits, info.channels, info.frames, info.sample_rate) == (kind, bits, 2, 19, 44100)
        assert wav.parse(wc.wav_bytes(raw, kind, 44100, extensible=True)).kind == kind
    for kind in (wc.U8, wc.S16, wc.S24, wc.S32):
        raw = _raw(kind, 23, 3)
        plain = wav.parse(wc.wav_bytes(raw, kind, 48000))
        ext = wav.parse(wc.wav_bytes(raw, kind, 48000, extensible=True))
        assert ext[:6] == plain[:6] and ext.data_offset == plain.data_offset + 24
    raw = _raw(wc.S16, 11)  # 22 payload bytes
    base = wav.parse(wc.wav_bytes(raw, wc.S16, 8000))
    buf = wc.wav_bytes(raw, wc.S16, 8000, before=[odd], between=[junk, odd], after=[odd])
    info = wav.parse(buf)
    assert info[:6] == base[:6] and info.data_offset == base.data_offset + 12 + 18 + 12
    assert bytes(buf[info.data_offset:info.data_offset + 22]) == wc.encode(raw, wc.S16)
    buf = wc.wav_bytes(raw, wc.S16, 8000, data_first=True, between=[odd])
    info = wav.parse(buf)
    assert info[:6] == base[:6] and info.data_offset == 12 + 8
    raw = _raw(wc.U8, 7)  # an odd payload, padded, with a chunk behind it
    info = wav.parse(wc.wav_bytes(raw, wc.U8, 8000, after=[junk]))
    assert info.frames == 7 and info.kind == wc.U8


def test_parse_oversized_data_means_the_frames_present():
    from asvspoof2021_air_amd import wav
    raw = _raw(wc.S16, 13, 2)
    for size in (0xFFFFFFFF, 13 * 4 + 1000):
        info = wav.parse(wc.wav_bytes(raw, wc.S16, 16000, data_size=size))
        assert info.frames == 13
    buf = wc.wav_bytes(raw, wc.S16, 16000, data_size=0xFFFFFFFF) + b"\x01\x02\x03"  # 3 stray bytes: no whole frame
    assert wav.parse(buf).frames == 13
    assert wav.parse(buf + b"\x04").frames == 14


def _refusals():
    raw = _raw(wc.S16, 9)
    w = lambda **kw: wc.wav_bytes(kw.pop("raw", raw), kw.pop("kind", wc.S16), 16000, **kw)
    fmt_only = b"WAVE" + wc.chunk(b"fmt ", wc.fmt_body(wc.S16, 1, 16000))
    data_only = b"WAVE" + wc.chunk(b"data", b"\0" * 8)
    bad_guid = struct.pack("<H", 1) + bytes(14)
    return [
        ("RIFX", w(riff=b"RIFX"), "container"), ("RF64", w(riff=b"RF64"), "container"),
        ("not riff", b"fLaC" + w()[4:], "container"), ("short", b"RIFF", "container"),
        ("A-law", w(tag=6, raw=_raw(wc.U8, 9), kind=wc.U8), "format_tag"),
        ("mu-law", w(tag=7, raw=_raw(wc.U8, 9), kind=wc.U8), "format_tag"), ("adpcm", w(tag=2), "format_tag"),
        ("12 bit", w(bits=12), "bits"), ("float16", w(tag=3), "bits"), ("pcm 64", w(raw=_raw(wc.F64, 9), kind=wc.F64, tag=1), "bits"),
        ("0 channels", w(raw=np.zeros((9, 0), np.int16)), "channels"), ("9 channels", w(raw=_raw(wc.S16, 9, 9)), "channels"),
        ("block align", w(block_align=4), "block_align"),
        ("no fmt", b"RIFF" + struct.pack("<I", len(data_only)) + data_only, "fmt"),
        ("no data", b"RIFF" + struct.pack("<I", len(fmt_only)) + fmt_only, "data"),
        ("fmt of 20 bytes", b"RIFF" + struct.pack("<I", 100) + b"WAVE" + wc.chunk(b"fmt ", bytes(20)) + wc.chunk(b"data", bytes(8)), "fmt"),
        ("zero frames", w(raw=np.zeros((0, 1), np.int16)), "frames"),
        ("one byte of a frame", w(raw=_raw(wc.S16, 9, 2))[:-35], "frames"),
        ("sub-format", w(extensible=True, guid=bad_guid), "sub_format"),
        ("sub-format tag", w(extensible=True, guid=struct.pack("<H", 6) + wc.GUID_TAIL), "sub_format"),
        ("extensible in 16 bytes", w(tag=0xFFFE), "fmt"),
    ]


@pytest.mark.parametrize("what, buf, field", _refusals(), ids=[r[0] for r in _refusals()])
def test_parse_refuses_by_file_and_field(what, buf, field):
    from asvspoof2021_air_amd import wav
    with pytest.raises(ValueError, match=r"dir/x\.wav: %s" % field):
        wav.parse(buf, "dir/x.wav")


# ---------------------------------------------------------------------------- WavSource / pack
def test_wav_source_and_pack(tmp_path):
    from asvspoof2021_air_amd import wav
    specs = [(wc.S16, 1, 24000, 1001), (wc.S24, 2, 48000, 333), (wc.F32, 1, 44100, 441), (wc.U8, 1, 8000, 77), (wc.S16, 1, 16000, 5)]
    paths, raws = [], []
    for i, (kind, C, sr, n) in enumerate(specs):
        raws.append(_raw(kind, n, C, seed=i))
        p = tmp_path / ("f%d.wav" % i)
        p.write_bytes(wc.wav_bytes(raws[-1], kind, sr, after=[(b"LIST", b"xyz")]))
        paths.append(str(p))
    src = wav.WavSource(paths)
    assert len(src) == 5 and src.path(2) == paths[2]
    items = [src.item(i) for i in range(5)]
    for (row, info), raw, (kind, C, sr, n) in zip(items, raws, specs):
        assert row.dtype == torch.uint8 and bytes(row.numpy()) == wc.encode(raw, kind)  # the payload alone, whole frames
        assert (info.kind, info.channels, info.sample_rate, info.frames) == (kind, C, sr, n)
    assert any(int(r.numel()) % 4 for r, _ in items)
    by, off, frames, fmt, rate, lengths = wav.pack(items, bytes_round=4096)
    assert by.dtype == torch.uint8 and by.dim() == 1 and by.numel() % 4096 == 0 and by.numel() - int(off[-1]) < 4096
    assert off.dtype == frames.dtype == fmt.dtype == lengths.dtype == torch.int32 and off.shape == (6,) and int(off[0]) == 0
    assert frames.tolist() == [s[3] for s in specs] and rate == tuple(s[2] for s in specs)
    assert fmt.tolist() == [1 | 2 << 4 | 1 << 8, 2 | 3 << 4 | 2 << 8, 4 | 4 << 4 | 1 << 8, 0 | 1 << 4 | 1 << 8, 1 | 2 << 4 | 1 << 8]
    assert lengths.tolist() == [ro.out_length(s[3], s[2]) for s in specs] == [668, 111, 160, 154, 5]
    for b, (row, _) in enumerate(items):
        s = (int(off[b]) + 3) & ~3
        assert s % 4 == 0 and int(off[b + 1]) - s == row.numel() and torch.equal(by[s:int(off[b + 1])], row)
        assert torch.count_nonzero(by[int(off[b]):s]) == 0
    assert torch.count_nonzero(by[int(off[-1]):]) == 0
    assert wav.pack(items[:4])[0].shape == wav.pack(items[1:])[0].shape == (65536,)
    with pytest.raises(ValueError):
        wav.pack([])
    nine = [(items[4][0], items[4][1]._replace(sample_rate=sr)) for sr in (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000)]
    assert len(wav.pack(nine[:8])[4]) == 8
    with pytest.raises(ValueError, match="9 distinct"):
        wav.pack(nine)
    src.take([3, 0])
    assert len(src) == 2 and src.path(0) == paths[3]
    (tmp_path / "odd.wav").write_bytes(wc.wav_bytes(_raw(wc.S16, 9), wc.S16, 16001))
    with pytest.raises(ValueError, match=r"odd\.wav.*16001"):
        wav.WavSource([str(tmp_path / "odd.wav")]).item(0)


# ---------------------------------------------------------------------------- the six dataset classes
RATES = [24000, 16000, 48000, 8000, 44100]
FRAMES = [7000, 12 * 160 + 3, 30000, 59 * 80, 99 * 441]


def _write(path, k):
    kind, C = [(wc.S16, 1), (wc.S24, 2), (wc.F32, 1), (wc.U8, 1), (wc.S16, 2)][k % 5]
    raw = wc.quantise(wc.signal(FRAMES[k % 5] + k, k, C), kind)
    with open(path, "wb") as f:
        f.write(wc.wav_bytes(raw, kind, RATES[k % 5]))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("raw_wav"))
    fx.build(root, _write)
    with open(os.path.join(HERE, "golden", "raw_wav.json")) as f:
        return root, json.load(f)


def test_fixture_covers_every_class(tree):
    root, golden = tree
    from asvspoof2021_air_amd import raw_dataset
    assert sorted(golden) == sorted(fx.cases(raw_dataset, root))
    assert {n.split("/")[0] for n in golden} == set(fx.CLASSES)


@pytest.mark.parametrize("name", sorted(json.load(open(os.path.join(HERE, "golden", "raw_wav.json")))))
def test_wav_classes_equal_the_reference(tree, name):
    """Length, file order, tag / label tables and every item's metadata are the reference's; item 0 is the file's
    payload with its header attached."""
    root, golden = tree
    from asvspoof2021_air_amd import raw_dataset, wav
    ds = fx.cases(raw_dataset, root)[name]()
    got = fx.record(ds, root)
    assert got == golden[name]
    assert len(ds[0]) == {"VCC2020Raw": 4, "ASVspoof2015Raw": 4}.get(name.split("/")[0], 6 if "AndDevice" in name else 5)
    row = ds[len(ds) - 1][0]
    assert row.dtype == torch.uint8 and row.dim() == 1 and isinstance(row.wav_info, wav.WavInfo)
    assert row.numel() == row.wav_info.frames * row.wav_info.block_align and row.wav_info.sample_rate in RATES


def test_wav_collate_draws_start_from_the_output_length(tree):
    root, golden = tree
    from asvspoof2021_air_amd import raw_dataset
    ds = raw_dataset.ASVspoof2019LARaw_withTransmissionAndDevice(os.path.join(root, "aug2"), os.path.join(root, "proto"), "train",
                                                                  feat_len=40, bytes_round=4096)
    items = [ds[i] for i in range(len(ds))]
    np.random.seed(123)
    by, off, frames, fmt, rate, lengths, start, names, tag, label, channel, device = ds.collate_fn(items)
    infos = [it[0].wav_info for it in items]
    assert by.dtype == torch.uint8 and by.numel() % 4096 == 0 and off.shape == (len(ds) + 1,)
    assert frames.tolist() == [i.frames for i in infos] and rate == tuple(i.sample_rate for i in infos)
    want_len = [ro.out_length(i.frames, i.sample_rate) for i in infos]
    assert lengths.tolist() == want_len and len(set(rate)) > 1
    meta = golden["ASVspoof2019LARaw_withTransmissionAndDevice/train"]["meta"]
    assert [list(m) for m in zip(names, tag, label, channel, device)] == meta
    np.random.seed(123)
    want = []
    for n in want_len:  # np.random.randint(T - feat_len) in item order, only where T > feat_len
        T = 1 + n // 160
        want.append(np.random.randint(T - 40) if T > 40 else 0)
    assert start.dtype == torch.int32 and start.tolist() == want and sum(1 for v in want_len if 1 + v // 160 > 40) >= 2
    assert any(1 + v // 160 <= 40 for v in want_len)


def test_path_arguments_are_required():
    from asvspoof2021_air_amd import raw_dataset
    for name in fx.CLASSES:
        with pytest.raises(TypeError):
            getattr(raw_dataset, name)()
