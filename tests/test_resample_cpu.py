"""CPU: the host side of the resampler - ``air_resample_geometry`` / ``air_resample_table_host`` against the fp64 oracle
written from the formulas (tests/resample_oracle.py), the oracle's own signal properties, the argument checks of the two
device entries (AIR_EINVAL ahead of any HIP call), and the opt-in resampling of the FLAC dataset classes.  Nothing here
touches a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import flac_cases as fc
import flac_oracle as fo
import resample_oracle as ro

EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from asvspoof2021_air_amd import _hip
    return _hip.lib()


def _geometry(lib, sr, tg=16000):
    L, M, K = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    rc = lib.air_resample_geometry(ctypes.c_int(sr), ctypes.c_int(tg), ctypes.byref(L), ctypes.byref(M), ctypes.byref(K))
    return rc, (L.value, M.value, K.value)


# ---------------------------------------------------------------------------- geometry and table
@pytest.mark.parametrize("sr", [8000, 11025, 22050, 24000, 32000, 44100, 48000])
def test_geometry_equals_the_oracle(lib, sr):
    from asvspoof2021_air_amd import resample
    rc, got = _geometry(lib, sr)
    assert rc == 0 and got == ro.geometry(sr) == resample.geometry(sr)
    for n in (1, 2, 3, 441, 44100, 63999, 2 ** 30):
        assert resample.out_length(n, sr) == ro.out_length(n, sr) == -(-n * got[0] // got[1])
    assert resample.out_length(np.array([1, 441, 63999]), sr).tolist() == [ro.out_length(n, sr) for n in (1, 441, 63999)]


def test_geometry_values_and_refusals(lib):
    from asvspoof2021_air_amd import resample
    assert _geometry(lib, 24000) == (0, (2, 3, 192)) and _geometry(lib, 8000) == (0, (2, 1, 128))
    assert _geometry(lib, 48000) == (0, (1, 3, 384)) and _geometry(lib, 44100) == (0, (160, 441, 354))
    assert _geometry(lib, 22050) == (0, (320, 441, 178)) and _geometry(lib, 11025) == (0, (640, 441, 128))
    assert _geometry(lib, 16000) == (0, (1, 1, 0))  # the identity path: no table
    for sr in (16001, 0, -8000, 7999, 44101):
        assert _geometry(lib, sr)[0] == EINVAL, sr
    assert _geometry(lib, 24000, 0)[0] == EINVAL and _geometry(lib, 24000, -1)[0] == EINVAL
    assert _geometry(lib, 16000 * 17)[0] == EINVAL  # K beyond AIR_RESAMPLE_MAX_K
    assert lib.air_resample_geometry(ctypes.c_int(24000), ctypes.c_int(16000), None, None, None) == EINVAL
    with pytest.raises(ValueError, match=r"a/b\.wav.*16001"):
        resample.geometry(16001, name="a/b.wav")
    assert lib.air_resample_table_host(ctypes.c_int(16001), ctypes.c_int(16000), ctypes.c_void_p(0x1000)) == EINVAL
    assert lib.air_resample_table_host(ctypes.c_int(24000), ctypes.c_int(16000), None) == EINVAL


@pytest.mark.parametrize("sr", [24000, 8000, 44100])
def test_table_within_one_ulp_of_the_oracle(sr):
    from asvspoof2021_air_amd import resample
    got = resample.host_table(sr).numpy()
    want64 = ro.table(sr)
    assert got.shape == want64.shape == ro.geometry(sr)[:1] + ro.geometry(sr)[2:]
    want = want64.astype(np.float32)
    ulp = np.spacing(np.abs(want))  # the distance to the next fp32 value
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print("sr %d: %d of %d entries differ from the rounded oracle, max %.3g ulp" % (
        sr, int((got != want).sum()), got.size, float((err / ulp).max())))
    assert np.all(err <= ulp)
    assert resample.host_table(16000) is None


# ---------------------------------------------------------------------------- the oracle's own properties
def _tone(f, sr, n):
    return np.sin(2 * np.pi * f * np.arange(n) / sr + 0.3)


@pytest.mark.parametrize("sr", [8000, 24000, 44100, 48000])
def test_oracle_reproduces_tones_and_rejects_images(sr):
    n = int(0.1 * sr)
    edge = 400
    for f in (1000.0, 7000.0):
        if f >= sr / 2:
            continue
        y, _ = ro.resample(_tone(f, sr, n), sr)
        assert len(y) == ro.out_length(n, sr) == 1600
        want = _tone(f, 16000, len(y))
        err = np.abs(y - want)[edge:-edge].max()
        print("sr %d, %g Hz: max error %.3g" % (sr, f, err))
        assert err < 1e-6
    if sr / 2 > 9000:
        y, _ = ro.resample(_tone(9000.0, sr, n), sr)
        rms = np.sqrt(np.mean(y[edge:-edge] ** 2))
        print("sr %d, 9 kHz: rms %.3g" % (sr, rms))
        assert rms < 1e-4
    y, _ = ro.resample(np.ones(n), sr)
    assert np.abs(y[edge:-edge] - 1.0).max() < 1e-7


def test_oracle_bound_and_identity():
    x = fc.signal(700, 3).astype(np.float64) / 32768.0
    y, bound = ro.resample(x, 16000)
    assert np.array_equal(y, x) and not bound.any()
    y, bound = ro.resample(x, 24000)
    assert len(y) == ro.out_length(700, 24000) == 467 and np.all(bound > 0) and bound.max() < 1e-4
    # a row shorter than the filter: only the samples inside [0, n) contribute
    y1, _ = ro.resample(np.array([1.0]), 24000)
    c = ro.table(24000)
    assert len(y1) == 1 and y1[0] == c[0][ro.geometry(24000)[2] // 2 - 1]


# ---------------------------------------------------------------------------- the C-ABI without a GPU
def _desc(records, nrates=None):
    from asvspoof2021_air_amd import resample
    d = resample.AirResampleDesc()
    d.nrates = len(records) if nrates is None else nrates
    for r, rec in enumerate(records[:8]):
        d.rate[r] = resample.AirResampleRate(*rec)
    return d


GOOD = [(2, 3, 192, 0), (1, 1, 0, 0)]
TABLE_ELEMS = 2 * 192
BAD_DESCS = [
    dict(records=[]), dict(records=[(2, 3, 192, 0)] * 8, nrates=9), dict(records=GOOD, nrates=-1),
    dict(records=[(641, 3, 192, 0)]), dict(records=[(0, 3, 192, 0)]), dict(records=[(2, 0, 192, 0)]),
    dict(records=[(2, 3, 2050, 0)]), dict(records=[(2, 3, 191, 0)]), dict(records=[(2, 3, -2, 0)]),
    dict(records=[(2, 3, 0, 0)]), dict(records=[(1, 1, 128, 0)]), dict(records=[(2, 2, 0, 0)]),
    dict(records=[(2, 3, 192, 1)]), dict(records=[(2, 3, 192, -1)]),
]


def test_resample_ragged_rejects_bad_arguments(lib):
    """AIR_EINVAL ahead of any device work: the (fake) device pointers are never dereferenced."""
    from asvspoof2021_air_amd import resample
    p = [ctypes.c_void_p(0x1000 * (k + 1)) for k in range(8)]
    null = ctypes.c_void_p(0)

    def call(x=p[0], kind=resample.S16, B=2, Lcap_in=24000, ln=p[1], idx=p[2], desc=_desc(GOOD), tables=p[3],
             elems=TABLE_ELEMS, y16=null, y32=p[4], Lcap=16000, st=p[5]):
        d = ctypes.byref(desc) if desc is not None else None
        return lib.air_resample_ragged(x, ctypes.c_int(kind), ctypes.c_int(B), ctypes.c_int(Lcap_in), ln, idx, d, tables,
                                       ctypes.c_size_t(elems), y16, y32, ctypes.c_int(Lcap), st, null)

    for bad in (dict(x=null), dict(ln=null), dict(idx=null), dict(st=null), dict(y16=null, y32=null), dict(desc=None),
                dict(tables=null), dict(B=0), dict(B=-1), dict(Lcap_in=0), dict(Lcap=0), dict(Lcap=-5), dict(elems=TABLE_ELEMS - 1),
                dict(kind=resample.U8), dict(kind=resample.S24), dict(kind=resample.F64), dict(kind=6), dict(kind=-1),
                dict(x=ctypes.c_void_p(0x1002)), dict(y32=p[0])):
        assert call(**bad) == EINVAL, bad
    for bad in BAD_DESCS:
        assert call(desc=_desc(**bad)) == EINVAL, bad


def test_wav_decode_rejects_bad_arguments(lib):
    p = [ctypes.c_void_p(0x1000 * (k + 1)) for k in range(9)]
    null = ctypes.c_void_p(0)

    def call(by=p[0], total=4096, off=p[1], fr=p[2], fm=p[3], idx=p[4], B=2, desc=_desc(GOOD), tables=p[5], elems=TABLE_ELEMS,
             y16=p[6], y32=null, Lcap=16000, st=p[7]):
        d = ctypes.byref(desc) if desc is not None else None
        return lib.air_wav_decode(by, ctypes.c_size_t(total), off, fr, fm, idx, ctypes.c_int(B), d, tables, ctypes.c_size_t(elems),
                                  y16, y32, ctypes.c_int(Lcap), st, null)

    for bad in (dict(by=null), dict(off=null), dict(fr=null), dict(fm=null), dict(idx=null), dict(st=null), dict(desc=None),
                dict(y16=null, y32=null), dict(tables=null), dict(B=0), dict(B=-1), dict(Lcap=0), dict(total=0),
                dict(total=1 << 31), dict(elems=0), dict(by=ctypes.c_void_p(0x1002))):
        assert call(**bad) == EINVAL, bad
    for bad in BAD_DESCS:
        assert call(desc=_desc(**bad)) == EINVAL, bad
    # identity records alone need no table
    assert call(desc=_desc([(1, 1, 0, 0)]), tables=null, elems=0, B=0) == EINVAL  # (B = 0 is what is refused here)


def test_status_and_kind_names_mirror_the_header():
    from asvspoof2021_air_amd import resample, wav
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "air_hip.h")).read()
    for code, name in resample.STATUS.items():
        assert re.search(r"#define AIR_WAV_%s %d\b" % (name, code), text), name
    for code, name in wav.KIND_NAMES.items():
        assert re.search(r"#define AIR_PCM_%s %d\b" % (name.upper(), code), text), name
    assert re.search(r"#define AIR_RESAMPLE_MAX_RATES %d\b" % resample.MAX_RATES, text)
    assert wav.fmt_code(wav.S24, 2) == 2 | (3 << 4) | (2 << 8)
    err = wav.WavError([(1, wav.LENGTH_MISMATCH)])
    assert "row 1 LENGTH_MISMATCH" in str(err) and err.rows == [(1, 1)] and isinstance(err, resample.ResampleError)


def test_rate_lists():
    from asvspoof2021_air_amd import resample
    assert resample.rate_list(24000, 3) == (24000,) * 3 and resample.rate_list([8000, 16000], 2) == (8000, 16000)
    assert resample.rate_list(torch.tensor([8000, 16000]), 2) == (8000, 16000)
    with pytest.raises(ValueError):
        resample.rate_list([8000], 2)
    assert resample.distinct((8000, 16000, 8000)) == [8000, 16000]
    with pytest.raises(ValueError, match="9 distinct"):
        resample.distinct(range(8000, 8009))


# ---------------------------------------------------------------------------- the FLAC classes: opt-in resampling
def test_flac_classes_resample_is_opt_in(tmp_path):
    from asvspoof2021_air_amd import raw_dataset
    d = tmp_path / "ASVspoof2021_LA_eval" / "flac"
    d.mkdir(parents=True)
    lengths = {"LA_E_0000000": (300, 8000), "LA_E_1000001": (50 * 160 + 3, 16000), "LA_E_2000002": (45 * 160, 8000),
               "LA_E_3000003": (7000, 16000)}
    for i, (name, (n, sr)) in enumerate(lengths.items()):
        (d / (name + ".flac")).write_bytes(fo.encode(fc.signal(n, 70 + i), 192, sample_rate=sr))
    ds = raw_dataset.ASVspoof2021evalRaw(str(d))
    with pytest.raises(ValueError, match=r"LA_E_0000000.flac.*sample_rate = 8000"):
        ds[0]
    assert len(ds.collate_fn([ds[1], ds[3]])) == 6  # [bytes, byte_off, lengths, blocksize, start, names]
    ds = raw_dataset.ASVspoof2021evalRaw(str(d), feat_len=40, resample=True)
    row, name = ds[0]
    assert name == "LA_E_0000000" and row.flac_info.sample_rate == 8000
    np.random.seed(5)
    by, off, ln, bs, start, rate, out_ln, names = ds.collate_fn([ds[i] for i in range(4)])
    assert ln.tolist() == [300, 8003, 7200, 7000] and rate == (8000, 16000, 8000, 16000)
    assert out_ln.dtype == torch.int32 and out_ln.tolist() == [600, 8003, 14400, 7000] and list(names) == list(lengths)
    # start is drawn from the OUTPUT length, in item order: T = 1 + n // 160 = 4, 51, 91, 44 against feat_len 40
    np.random.seed(5)
    want = [0, np.random.randint(51 - 40), np.random.randint(91 - 40), np.random.randint(44 - 40)]
    assert start.dtype == torch.int32 and start.tolist() == want
    (d / "LA_E_9999999.flac").write_bytes(fo.encode(fc.signal(300, 80), 192, sample_rate=16001))
    ds = raw_dataset.ASVspoof2021evalRaw(str(d), resample=True)
    with pytest.raises(ValueError, match=r"LA_E_9999999.flac.*16001"):
        ds[len(ds) - 1]
