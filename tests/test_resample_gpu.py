"""GPU: csrc/resample.hip through ``resample.Resampler`` - PCM that already lies on the device (a dense ragged batch,
int16 or float32) against the fp64 oracle (tests/resample_oracle.py) within the bound it derives per sample, and against
``wav.WavDecoder`` over the same samples as files, bit for bit (one kernel, two fetches)."""
import numpy as np
import pytest
import torch

import resample_oracle as ro
import wav_cases as wc

pytestmark = pytest.mark.gpu

FILL = 12345.0
GUARD = 256


@pytest.fixture(scope="module")
def resampler():
    from asvspoof2021_air_amd import resample
    return resample.Resampler("cuda")


def _dense(rows, dtype, Lcap_in):
    x = np.full((len(rows), Lcap_in), 77, dtype=np.int16)  # the tails of the input are not zero: they must not be read
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    t = torch.from_numpy(x)
    return (t.to(torch.float32) / 32768.0 if dtype == torch.float32 else t).cuda()


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16])
@pytest.mark.parametrize("sr", wc.RESAMPLE_RATES)
def test_resample_dense_rows_within_the_derived_bound(resampler, sr, dtype):
    """The rows of wc.row_lengths(sr) in one dense batch whose capacity is odd (rows are then not 4-byte aligned in
    int16).  Every output within the oracle's bound, tails zero, lengths = ceil(n L / M), guards untouched."""
    rows = wc.resample_rows(sr)
    n = [len(x) for x, _, _ in rows]
    pcm = _dense([x for x, _, _ in rows], dtype, (max(n) + 3) | 1)
    assert pcm.shape[1] % 2 == 1
    B, Lcap = len(rows), max(len(y) for _, y, _ in rows) + 29
    whole = torch.full((B * Lcap + 2 * GUARD,), FILL, dtype=torch.float32, device="cuda")
    out = whole[GUARD:GUARD + B * Lcap].view(B, Lcap)
    y, out_ln = resampler.resample(pcm, torch.tensor(n, dtype=torch.int32), sr, Lcap=Lcap, out=out)
    assert y.data_ptr() == out.data_ptr() and out_ln.dtype == torch.int32 and out_ln.is_cuda
    assert out_ln.tolist() == [len(r[1]) for r in rows] == [ro.out_length(v, sr) for v in n]
    assert resampler.last_status.tolist() == [0] * B
    got = y.cpu().numpy()
    for b, (x, want, bound) in enumerate(rows):
        err = np.abs(got[b, :len(want)].astype(np.float64) - want)
        print("%d Hz %s row of %d: max error / bound %.3f" % (sr, dtype, len(x), float((err / bound).max())))
        assert np.all(err <= bound), "row %d" % b
        assert not got[b, len(want):].any(), "tail of row %d" % b
    assert bool((whole[:GUARD] == FILL).all()) and bool((whole[-GUARD:] == FILL).all())


def test_resampler_equals_wav_decoder(resampler):
    """Device int16 PCM at 24 kHz (and one row at 16 kHz, one at 44.1 kHz) = WavDecoder.decode of the same samples as
    WAV files, bit for bit, in float32 and in int16."""
    from asvspoof2021_air_amd import wav
    rates = [24000, 24000, 16000, 44100, 24000]
    xs = [wc.resample_rows(24000)[8][0], wc.resample_rows(24000)[3][0], wc.quantise(wc.signal(999, 5), wc.S16)[:, 0],
          wc.resample_rows(44100)[7][0], wc.resample_rows(24000)[6][0]]
    n = [len(x) for x in xs]
    items = []
    for x, sr in zip(xs, rates):
        buf = wc.wav_bytes(x, wc.S16, sr)
        info = wav.parse(buf)
        items.append((torch.from_numpy(np.frombuffer(buf, dtype=np.uint8, count=2 * len(x), offset=info.data_offset).copy()), info))
    by, off, fr, fm, rate, ln = wav.pack(items, bytes_round=256)
    dec = wav.WavDecoder("cuda")
    Lcap = int(ln.max()) + 5
    for dtype in (torch.float32, torch.int16):
        want, st = dec.decode(by.cuda(), off, fr, fm, rate, Lcap=Lcap, dtype=dtype, check=True)
        got, out_ln = resampler.resample(_dense(xs, torch.int16, max(n) + 1), torch.tensor(n, dtype=torch.int32), rates,
                                         Lcap=Lcap, dtype=dtype, check=True)
        assert got.dtype == dtype and torch.equal(got, want) and torch.equal(out_ln.cpu(), ln)
    # lengths on the device, the default capacity (reads the lengths), a single rate for every row
    y, out_ln = resampler.resample(_dense(xs[:2], torch.int16, max(n)), torch.tensor(n[:2], dtype=torch.int32).cuda(), 24000)
    assert y.shape == (2, 16000) and y.dtype == torch.float32 and out_ln.tolist() == ln[:2].tolist()
    assert torch.equal(y[:, :Lcap], dec.decode(by.cuda(), off, fr, fm, rate, Lcap=Lcap)[0][:2])


def test_resampler_refuses_and_reports(resampler):
    from asvspoof2021_air_amd import resample
    pcm = torch.zeros((2, 100), dtype=torch.int16, device="cuda")
    n = torch.tensor([100, 50], dtype=torch.int32)
    with pytest.raises(ValueError, match="16001"):
        resampler.resample(pcm, n, 16001, Lcap=200)
    with pytest.raises(ValueError, match="device tensor"):
        resampler.resample(pcm, n, torch.tensor([8000, 8000]).cuda(), Lcap=200)
    with pytest.raises(ValueError):
        resampler.resample(pcm.double(), n, 8000, Lcap=200)
    # a row longer than the input capacity, and one whose output exceeds Lcap: a status, zeros, nothing else
    y, out_ln = resampler.resample(pcm + 5, torch.tensor([101, 50], dtype=torch.int32), 8000, Lcap=150)
    assert resampler.last_status.tolist() == [resample.LENGTH_MISMATCH, resample.OK] and int(torch.count_nonzero(y[0])) == 0
    assert int(torch.count_nonzero(y[1, :100])) > 0 and int(torch.count_nonzero(y[1, 100:])) == 0
    y, out_ln = resampler.resample(pcm + 5, n, 8000, Lcap=150)
    assert resampler.last_status.tolist() == [resample.LENGTH_MISMATCH, resample.OK]
    with pytest.raises(resample.ResampleError, match="row 0 LENGTH_MISMATCH"):
        resample.check(resampler.last_status)
