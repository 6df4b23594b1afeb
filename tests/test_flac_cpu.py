"""CPU: the host side of the FLAC path - the oracle encoder / decoder (tests/flac_oracle.py) round-trips every stream the
GPU tests decode, ``flac.parse_stream`` / ``pack``, the ``raw_dataset`` classes over a tiny fabricated corpus, and the
argument checks of the two ABI calls.  Nothing here touches a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import flac_cases as fc
import flac_oracle as fo

FEAT_LEN = 40


# ---------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("name", fc.CASES)
def test_oracle_round_trip(name):
    for buf, x in fc.streams(name):
        y = fo.decode(buf)
        assert y.dtype == np.int16 and np.array_equal(y, x)


def test_oracle_crcs_and_refusals():
    # the check values of CRC-8 (poly 0x07) and CRC-16/BUYPASS (poly 0x8005, init 0) over "123456789"
    assert fo.crc8(b"123456789") == 0xF4 and fo.crc16(b"123456789") == 0xFEE8
    buf, x = fc.streams("fixed2")[4]
    bad = bytearray(buf)
    bad[-20] ^= 0x04
    with pytest.raises(ValueError):
        fo.decode(bytes(bad))
    with pytest.raises(ValueError):
        fo.decode(buf[:-5])
    for x, bs, specs in fc.unsupported_rows():
        with pytest.raises(ValueError, match="unsupported"):
            fo.decode(fo.encode(x, bs, specs))


def test_false_sync_stream_embeds_a_whole_valid_frame():
    (x, bs, specs), inner = fc.false_sync_row()
    buf = fo.encode(x, bs, specs)
    at = buf.find(inner)
    assert at > 0 and fo.crc8(inner[:6]) == inner[6] and fo.crc16(inner[:-2]) == int.from_bytes(inner[-2:], "big")
    got, fn, end = fo.decode_frame(buf, at, None)  # decodable on its own: 192 samples of FALSE_VALUE, frame number 1
    assert got == [fc.FALSE_VALUE] * 192 and fn == 1 and end == at + len(inner)
    assert np.array_equal(fo.decode(buf), x) and int((x == fc.FALSE_VALUE).sum()) == 1


# ---------------------------------------------------------------------------- parse_stream / pack
def test_parse_stream_fields():
    from asvspoof2021_air_amd import flac
    x = fc.signal(192 * 3 + 5, 1)
    pad = (1, b"\0" * 11)  # a PADDING block behind STREAMINFO: the metadata is walked, not assumed to be one block
    buf = fo.encode(x, 192, [dict(type="fixed", order=2)], extra_blocks=[pad, (4, b"\x00" * 8)])
    info = flac.parse_stream(buf, "a.flac")
    assert info.audio_offset == 4 + (4 + 34) + (4 + 11) + (4 + 8) and buf[info.audio_offset:info.audio_offset + 2] == b"\xff\xf8"
    assert (info.min_blocksize, info.max_blocksize, info.sample_rate, info.channels, info.bits_per_sample) == (192, 192, 16000, 1, 16)
    assert info.total_samples == len(x) and info.md5 == fo.pcm_md5(x)
    frames = fo.audio_frames(buf)
    sizes, pos = [], 0
    while pos < len(frames):
        end = fo.decode_frame(frames, pos, None)[2]
        sizes.append(end - pos)
        pos = end
    assert (info.min_framesize, info.max_framesize) == (min(sizes), max(sizes))
    assert flac.parse_stream(memoryview(buf)) == info and flac.parse_stream(np.frombuffer(buf, dtype=np.uint8)) == info


@pytest.mark.parametrize("over, field", [(dict(channels=2), "channels"), (dict(bps=24), "bits_per_sample"),
                                         (dict(total=0), "total_samples"), (dict(min_bs=16), "min_blocksize")])
def test_parse_stream_refuses_what_the_device_does_not_serve(over, field):
    from asvspoof2021_air_amd import flac
    buf = fo.encode(fc.signal(400, 2), 192, info=over)
    with pytest.raises(ValueError, match=r"LA_T_1.flac.*%s" % field):
        flac.parse_stream(buf, "LA_T_1.flac")


def test_parse_stream_refuses_truncated_or_absent_streaminfo():
    from asvspoof2021_air_amd import flac
    buf = fo.encode(fc.signal(400, 3), 192)
    for bad in (buf[:20], buf[:4], b"fLaC" + fo.metadata_block(1, b"\0" * 40, True) + buf[42:],
                b"fLaC" + fo.metadata_block(0, b"\0" * 10, True)):
        with pytest.raises(ValueError, match=r"x.flac.*STREAMINFO"):
            flac.parse_stream(bad, "x.flac")
    with pytest.raises(ValueError, match=r"x.flac.*marker"):
        flac.parse_stream(b"RIFF" + buf[4:], "x.flac")


def _items(streams):
    from asvspoof2021_air_amd import flac
    out = []
    for buf in streams:
        info = flac.parse_stream(buf)
        out.append((torch.from_numpy(np.frombuffer(buf, dtype=np.uint8, offset=info.audio_offset).copy()), info))
    return out


def test_pack_alignment_offsets_and_capacity():
    from asvspoof2021_air_amd import flac
    streams = [b for b, _ in fc.streams("ragged")]
    items = _items(streams)
    assert any(int(r.numel()) % 4 for r, _ in items)
    by, off, lengths, blocksize = flac.pack(items, bytes_round=4096)
    assert by.dtype == torch.uint8 and by.dim() == 1 and by.numel() % 4096 == 0 and by.numel() - int(off[-1]) < 4096
    assert off.dtype == lengths.dtype == blocksize.dtype == torch.int32 and off.shape == (6,) and int(off[0]) == 0
    assert lengths.tolist() == [len(x) for _, x in fc.streams("ragged")] and blocksize.tolist() == [16, 4096, 16, 192, 4096]
    for b, (row, _) in enumerate(items):
        s = (int(off[b]) + 3) & ~3
        assert s % 4 == 0 and int(off[b + 1]) - s == row.numel() and torch.equal(by[s:int(off[b + 1])], row)
        assert torch.count_nonzero(by[int(off[b]):s]) == 0
    assert torch.count_nonzero(by[int(off[-1]):]) == 0
    # one capacity for batches of similar size: DevicePrefetcher's ring is keyed by shape
    assert flac.pack(items[:4], bytes_round=65536)[0].shape == flac.pack(items[1:], bytes_round=65536)[0].shape == (65536,)
    with pytest.raises(ValueError):
        flac.pack([])


def test_flac_source(tmp_path):
    from asvspoof2021_air_amd import flac
    paths = []
    for i, (buf, _) in enumerate(fc.streams("ragged")[:3]):
        p = tmp_path / ("f%d.flac" % i)
        p.write_bytes(buf)
        paths.append(str(p))
    src = flac.FlacSource(paths)
    assert len(src) == 3 and src.path(1) == paths[1]
    row, info = src.item(1)
    assert row.dtype == torch.uint8 and bytes(row.numpy()) == fo.audio_frames(fc.streams("ragged")[1][0])
    assert info.total_samples == 3 * 4096 + 37
    src.take([2, 0])
    assert len(src) == 2 and src.path(0) == paths[2]
    (tmp_path / "stereo.flac").write_bytes(fo.encode(fc.signal(100, 4), 16, info=dict(channels=2)))
    with pytest.raises(ValueError, match=r"stereo.flac.*channels"):
        flac.FlacSource([str(tmp_path / "stereo.flac")]).item(0)


def test_status_names_mirror_the_header():
    from asvspoof2021_air_amd import flac
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "air_hip.h")).read()
    import re
    for code, name in flac.STATUS.items():
        assert re.search(r"#define AIR_FLAC_%s %d\b" % (name, code), text), name
    err = flac.FlacError([(1, flac.BAD_CRC16), (3, flac.LENGTH_MISMATCH)])
    assert "row 1 BAD_CRC16" in str(err) and "row 3 LENGTH_MISMATCH" in str(err) and err.rows[1] == (3, 4)


def test_verify_md5_on_host_rows():
    from asvspoof2021_air_amd import flac
    buf, x = fc.streams("ragged")[2]
    info = flac.parse_stream(buf)
    row = torch.zeros(200, dtype=torch.int16)
    row[:len(x)] = torch.from_numpy(x)
    assert flac.verify_md5(row, info)
    row[7] += 1
    assert not flac.verify_md5(row, info)


# ---------------------------------------------------------------------------- raw_dataset over a fabricated corpus
LENGTHS = [159, 40 * 160, 100 * 160 + 37, 77 * 160 + 3, 3000, 55 * 160]


def _corpus(root, access="LA"):
    """<db>/<access>/ASVspoof2019_<access>_<part>/flac/*.flac, protocols for train / dev under <proto>, for eval under
    <db>/<access>/ASVspoof2019_<access>_cm_protocols/ (raw_dataset.py:37-42)."""
    db, proto = root / "db", root / "proto"
    tags = ["-", "A01", "A07", "-", "A19", "A04"] if access == "LA" else ["-", "AA", "CB", "-", "CC", "BA"]
    waves = {}
    for part, letter in (("train", "T"), ("dev", "D"), ("eval", "E")):
        audio = db / access / ("ASVspoof2019_%s_%s" % (access, part)) / "flac"
        audio.mkdir(parents=True)
        pdir = proto if part != "eval" else db / access / ("ASVspoof2019_%s_cm_protocols" % access)
        pdir.mkdir(parents=True, exist_ok=True)
        lines = []
        for i, n in enumerate(LENGTHS):
            name = "%s_%s_%07d" % (access, letter, 1000000 + i)
            x = fc.signal(n, seed=10 * ("train", "dev", "eval").index(part) + i)
            (audio / (name + ".flac")).write_bytes(fo.encode(x, 4096 if i % 2 else 1152, [dict(type="fixed", order=2)]))
            waves[(part, i)] = x
            lines.append("%s_%04d %s - %s %s" % (access, i, name, tags[i], "bonafide" if tags[i] == "-" else "spoof"))
        (pdir / ("ASVspoof2019.%s.cm.%s.trl.txt" % (access, part))).write_text("\n".join(lines) + "\n")
    return str(db), str(proto), tags, waves


@pytest.mark.parametrize("access", ["LA", "PA"])
@pytest.mark.parametrize("part", ["train", "dev", "eval"])
def test_asvspoof2019raw_paths_protocol_and_tuples(tmp_path, access, part):
    from asvspoof2021_air_amd import dataset as air_ds, raw_dataset
    db, proto, tags, waves = _corpus(tmp_path, access)
    # the eval protocol is read from the database tree: a wrong path_to_protocol is then no obstacle
    ds = raw_dataset.ASVspoof2019Raw(access, db, proto if part != "eval" else str(tmp_path / "nowhere"), part)
    assert len(ds) == len(LENGTHS) and ds.path_to_audio.endswith("ASVspoof2019_%s_%s/flac/" % (access, part))
    assert ds.tag == (air_ds.TAG_LA19 if access == "LA" else air_ds.TAG_PA19) and ds.label == {"spoof": 1, "bonafide": 0}
    for i in (0, 2, 5):
        row, filename, tag, label = ds[i]
        letter = {"train": "T", "dev": "D", "eval": "E"}[part]
        assert filename == "%s_%s_%07d" % (access, letter, 1000000 + i) and tag == tags[i]
        assert label == ("bonafide" if tags[i] == "-" else "spoof") and tag in ds.tag
        assert row.dtype == torch.uint8 and row.flac_info.total_samples == LENGTHS[i]
        stream = open(os.path.join(ds.path_to_audio, filename + ".flac"), "rb").read()
        assert bytes(row.numpy()) == fo.audio_frames(stream) and np.array_equal(fo.decode(stream), waves[(part, i)])
    with pytest.raises(FileNotFoundError):
        raw_dataset.ASVspoof2019Raw(access, db, str(tmp_path / "nowhere"), "train")


def test_raw_collate_draws_start_like_collate_ragged(tmp_path):
    from asvspoof2021_air_amd import dataset as air_ds, raw_dataset
    db, proto, tags, waves = _corpus(tmp_path)
    ds = raw_dataset.ASVspoof2019Raw("LA", db, proto, "train", feat_len=FEAT_LEN, bytes_round=4096)
    np.random.seed(123)
    by, off, lengths, blocksize, start, names, tag, label = ds.collate_fn([ds[i] for i in range(len(ds))])
    assert by.dtype == torch.uint8 and by.numel() % 4096 == 0 and off.shape == (len(LENGTHS) + 1,)
    assert lengths.tolist() == LENGTHS and blocksize.tolist() == [4096 if i % 2 else 1152 for i in range(len(LENGTHS))]
    assert list(names) == ["LA_T_%07d" % (1000000 + i) for i in range(len(LENGTHS))] and list(tag) == tags
    assert list(label) == ["bonafide" if t == "-" else "spoof" for t in tags]
    # the same draws as the ragged PCM collate over the decoded waveforms, under the same seed
    items = [("%05d_LA_T_%07d_%s_%s" % (i, 1000000 + i, tags[i], "bonafide" if tags[i] == "-" else "spoof"), waves[("train", i)])
             for i in range(len(LENGTHS))]
    ref = air_ds.ASVspoof2019("LA", None, "train", feat_len=FEAT_LEN, source=air_ds.PCMSource(items, device="cpu"),
                              return_pcm="ragged")
    np.random.seed(123)
    pcm, ref_lengths, ref_start = ref.collate_fn([ref[i] for i in range(len(ref))])[:3]
    assert start.dtype == torch.int32 and torch.equal(start, ref_start) and torch.equal(lengths, ref_lengths)
    assert int(torch.count_nonzero(start)) >= 2 and int(start[1]) == 0  # (T = feat_len draws nothing)


def test_asvspoof2021evalraw_and_the_sample_rate_rule(tmp_path):
    from asvspoof2021_air_amd import raw_dataset
    d = tmp_path / "ASVspoof2021_LA_eval" / "flac"
    (d / "sub").mkdir(parents=True)
    names = ["LA_E_9000002", "LA_E_1000001", "sub/LA_E_5000003"]
    for i, n in enumerate(names):
        (d / (n + ".flac")).write_bytes(fo.encode(fc.signal(500 + i, 60 + i), 192))
    (d / "notes.txt").write_text("not audio")
    ds = raw_dataset.ASVspoof2021evalRaw(str(d))
    assert len(ds) == 3 and [os.path.basename(p) for p in ds.all_files] == [
        "LA_E_1000001.flac", "LA_E_9000002.flac", "LA_E_5000003.flac"]  # sorted by path
    row, filename = ds[0]
    assert filename == "LA_E_1000001" and row.flac_info.total_samples == 501
    by, off, lengths, blocksize, start, fns = ds.collate_fn([ds[0], ds[1]])
    assert lengths.tolist() == [501, 500] and list(fns) == ["LA_E_1000001", "LA_E_9000002"] and start.tolist() == [0, 0]
    (d / "LA_E_0000000.flac").write_bytes(fo.encode(fc.signal(300, 70), 192, sample_rate=8000))
    ds = raw_dataset.ASVspoof2021evalRaw(str(d))
    with pytest.raises(ValueError, match=r"LA_E_0000000.flac.*sample_rate = 8000"):
        ds[0]


# ---------------------------------------------------------------------------- the C-ABI without a GPU
@pytest.fixture(scope="module")
def lib():
    from asvspoof2021_air_amd import _hip
    return _hip.lib()


def test_workspace_query(lib):
    ws = lib.air_flac_workspace_bytes
    small, big = ws(ctypes.c_size_t(65536), ctypes.c_int(4)), ws(ctypes.c_size_t(4 * 65536), ctypes.c_int(4))
    # one bit per byte position and a 16-byte record per 4 bytes: a little over 4 bytes of workspace per byte
    assert 4 * 65536 < small < 5 * 65536 and 4 * 4 * 65536 < big < 5 * 4 * 65536 and small % 16 == 0
    assert ws(ctypes.c_size_t(65536), ctypes.c_int(64)) > small
    assert ws(ctypes.c_size_t(65536), ctypes.c_int(0)) == 0 and ws(ctypes.c_size_t(1 << 31), ctypes.c_int(1)) == 0


def test_decode_rejects_bad_arguments(lib):
    """AIR_EINVAL ahead of any device work: the (fake) device pointers are never dereferenced."""
    p = [ctypes.c_void_p(0x1000 * (k + 1)) for k in range(8)]
    null = ctypes.c_void_p(0)
    need = lib.air_flac_workspace_bytes(ctypes.c_size_t(4096), ctypes.c_int(2))

    def call(by=p[0], total=4096, off=p[1], ln=p[2], bs=p[3], B=2, Lcap=16000, y16=p[4], y32=null, st=p[5], ws=p[6], ws_bytes=need):
        return lib.air_flac_decode(by, ctypes.c_size_t(total), off, ln, bs, ctypes.c_int(B), ctypes.c_int(Lcap), y16, y32, st,
                                   ws, ctypes.c_size_t(ws_bytes), null)

    for bad in (dict(by=null), dict(off=null), dict(ln=null), dict(bs=null), dict(st=null), dict(ws=null),
                dict(y16=null, y32=null), dict(B=0), dict(B=-1), dict(Lcap=0), dict(total=0), dict(total=1 << 31),
                dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(by=ctypes.c_void_p(0x1002)), dict(ws=ctypes.c_void_p(0x7008))):
        assert call(**bad) == -1, bad
