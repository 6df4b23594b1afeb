"""GPU: csrc/resample.hip through ``wav.WavDecoder`` - the identity path bit for bit against the conversions a libsndfile
float read performs, the resampler against its fp64 oracle (tests/resample_oracle.py) within the bound the oracle
derives per sample, int16 output, a mixed batch, the length guard, and the corpus -> trainer path.

Outputs are pre-filled with FILL and carry GUARD canary samples on both sides, so a sample the kernel did not write, a
tail it did not zero or a store outside the output shows."""
import contextlib

import numpy as np
import pytest
import torch

import flac_cases as fc
import flac_oracle as fo
import resample_oracle as ro
import wav_cases as wc
from oracle.filler import fill_module_

pytestmark = pytest.mark.gpu

FILL = 12345
GUARD = 256


@pytest.fixture(scope="module")
def decoder():
    from asvspoof2021_air_amd import wav
    return wav.WavDecoder("cuda")


def _items(files):
    from asvspoof2021_air_amd import wav
    out = []
    for buf in files:
        info = wav.parse(buf)
        row = np.frombuffer(buf, dtype=np.uint8, count=info.frames * info.block_align, offset=info.data_offset).copy()
        out.append((torch.from_numpy(row), info))
    return out


def _decode(decoder, files, dtype=torch.float32, pad=37, frames=None):
    """Decode `files` as one batch into a pre-filled, guarded output -> (pcm, status, output lengths, guard tensor)."""
    from asvspoof2021_air_amd import wav
    by, off, fr, fm, rate, ln = wav.pack(_items(files), bytes_round=256)
    if frames is not None:
        fr = torch.tensor(frames, dtype=torch.int32)
    B, Lcap = len(files), int(ln.max()) + pad
    whole = torch.full((B * Lcap + 2 * GUARD,), FILL, dtype=dtype, device="cuda")
    out = whole[GUARD:GUARD + B * Lcap].view(B, Lcap)
    pcm, status = decoder.decode(by.cuda(), off, fr, fm, rate, Lcap=Lcap, dtype=dtype, out=out)
    assert pcm.data_ptr() == out.data_ptr() and status.dtype == torch.int32 and status.shape == (B,)
    return pcm, status, ln.tolist(), whole


def _guards_intact(whole):
    return bool((whole[:GUARD] == FILL).all()) and bool((whole[-GUARD:] == FILL).all())


def _within(got, y, bound, what):
    err = np.abs(got.astype(np.float64) - y)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if len(y) else 0.0
    print("%s: %d outputs, max error %.3g, max error / bound %.3f" % (what, len(y), float(err.max()) if len(y) else 0.0, worst))
    assert np.all(err <= bound), what


# ---------------------------------------------------------------------------- identity path
def test_identity_s16_mono_is_the_file(decoder):
    """16 kHz s16 mono: int16 output = the file's samples, float output = sample / 32768; rows of odd and even length."""
    raws = [wc.quantise(wc.signal(n, 7 + n), wc.S16) for n in (1, 2, 1025, 2049, 3333)]
    raws[2][:4, 0] = [-32768, 32767, 0, -1]
    files = [wc.wav_bytes(r, wc.S16, 16000) for r in raws]
    pcm, status, ln, whole = _decode(decoder, files, dtype=torch.int16)
    assert status.tolist() == [0] * 5 and ln == [len(r) for r in raws]
    for b, r in enumerate(raws):
        assert torch.equal(pcm[b, :ln[b]].cpu(), torch.from_numpy(r[:, 0])) and int(torch.count_nonzero(pcm[b, ln[b]:])) == 0
    assert _guards_intact(whole)
    f32, status, ln, whole = _decode(decoder, files)
    for b, r in enumerate(raws):
        assert torch.equal(f32[b, :ln[b]].cpu(), torch.from_numpy(r[:, 0]).to(torch.float32) / 32768.0)
        assert int(torch.count_nonzero(f32[b, ln[b]:])) == 0
    assert status.tolist() == [0] * 5 and _guards_intact(whole)


@pytest.mark.parametrize("kind", ["u8", "s16", "s24", "s32", "f32", "f64"])
def test_identity_conversions_and_downmix(decoder, kind):
    """Every sample kind, mono / 2 / 5 channels, in one batch: the conversions of a libsndfile float read and
    np.mean(frames.T, axis=0) in float32, bit for bit.  Extremes of the integer range included."""
    k = wc.KINDS[kind]
    raws = [wc.quantise(wc.signal(n, 31 + C, C, amp=0.7), k) for n, C in ((1031, 1), (2050, 2), (777, 5), (3, 2))]
    if k in (wc.U8, wc.S16, wc.S24, wc.S32):
        lo, hi = {wc.U8: (0, 255), wc.S16: (-32768, 32767), wc.S24: (-8388608, 8388607), wc.S32: (-2 ** 31, 2 ** 31 - 1)}[k]
        for r in raws[:3]:
            r[:4, 0] = [lo, hi, hi - 1, lo + 1]
            r[4:6, -1] = [hi, lo]
    files = [wc.wav_bytes(r, k, 16000, extensible=(i == 1)) for i, r in enumerate(raws)]
    pcm, status, ln, whole = _decode(decoder, files)
    assert status.tolist() == [0] * 4 and ln == [len(r) for r in raws]
    for b, r in enumerate(raws):
        want = wc.mono(wc.to_float(r, k))
        assert want.dtype == np.float32
        assert torch.equal(pcm[b, :ln[b]].cpu(), torch.from_numpy(want)), "row %d" % b
        assert int(torch.count_nonzero(pcm[b, ln[b]:])) == 0
    assert _guards_intact(whole)


# ---------------------------------------------------------------------------- resampling against the oracle
@pytest.mark.parametrize("sr", wc.RESAMPLE_RATES)
def test_resample_within_the_derived_bound(decoder, sr):
    """Nine rows per rate in one launch (wc.row_lengths: shorter than the filter, around one tile, three tiles and a
    bit).  Every output within (K + 3) 2^-24 sum |c x| + 2^-24 |y| of the fp64 oracle; tails zero."""
    rows = wc.resample_rows(sr)
    files = [wc.wav_bytes(x, wc.S16, sr) for x, _, _ in rows]
    pcm, status, ln, whole = _decode(decoder, files)
    assert status.tolist() == [0] * len(rows) and ln == [len(y) for _, y, _ in rows]
    got = pcm.cpu().numpy()
    for b, (x, y, bound) in enumerate(rows):
        _within(got[b, :ln[b]], y, bound, "%d Hz, row of %d samples" % (sr, len(x)))
        assert not got[b, ln[b]:].any(), "tail of row %d" % b
    assert _guards_intact(whole)


def test_resample_from_other_formats_within_the_bound(decoder):
    """The byte-wise fetches feed the same sum: 48 kHz s24 stereo, 44.1 kHz f32 mono, 24 kHz f64 with 3 channels, 8 kHz u8."""
    specs = [(wc.S24, 2, 48000, 3070 + 7), (wc.F32, 1, 44100, 2823), (wc.F64, 3, 24000, 1537), (wc.U8, 1, 8000, 513)]
    raws = [wc.quantise(wc.signal(n, 90 + i, C, sr=sr), k) for i, (k, C, sr, n) in enumerate(specs)]
    files = [wc.wav_bytes(r, k, sr) for r, (k, C, sr, n) in zip(raws, specs)]
    pcm, status, ln, whole = _decode(decoder, files)
    assert status.tolist() == [0] * 4
    got = pcm.cpu().numpy()
    for b, (r, (k, C, sr, n)) in enumerate(zip(raws, specs)):
        y, bound = ro.resample(wc.mono(wc.to_float(r, k)).astype(np.float64), sr)
        assert ln[b] == len(y)
        _within(got[b, :ln[b]], y, bound, "%s x %d at %d Hz" % (k, C, sr))
        assert not got[b, ln[b]:].any()
    assert _guards_intact(whole)


def _to_int16(y32):
    return np.clip(np.rint(y32.astype(np.float32) * np.float32(32768.0)), -32768, 32767).astype(np.int16)


def test_int16_output_is_the_rounded_float_output(decoder):
    """int16 = saturating round-half-even of 32768 x the float output of the same inputs, bit for bit - rows past full
    scale (a float file at 1.5) and exact halves (identity path) included."""
    loud = (6.0 * wc.signal(1500, 3, amp=0.05, sr=24000)).astype(np.float32)  # a 3 kHz tone of amplitude 1.5
    halves = (np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 32767.5, -32768.5, 40000.0, -40000.0, 32766.5]) / 32768.0).astype(np.float32)
    files = [wc.wav_bytes(loud, wc.F32, 24000), wc.wav_bytes(halves, wc.F32, 16000),
             wc.wav_bytes(wc.resample_rows(44100)[7][0], wc.S16, 44100), wc.wav_bytes(wc.resample_rows(8000)[8][0], wc.S16, 8000)]
    f32, st32, ln, whole32 = _decode(decoder, files)
    i16, st16, ln16, whole16 = _decode(decoder, files, dtype=torch.int16)
    assert st32.tolist() == st16.tolist() == [0] * 4 and ln == ln16 and _guards_intact(whole32) and _guards_intact(whole16)
    f, i = f32.cpu().numpy(), i16.cpu().numpy()
    assert np.abs(f[0]).max() > 1.0 and i[0].max() == 32767 and i[0].min() == -32768
    assert i[1, :11].tolist() == [0, 2, 2, 0, -2, -2, 32767, -32768, 32767, -32768, 32766]
    for b in range(4):
        assert np.array_equal(i[b], _to_int16(f[b])), "row %d" % b


# ---------------------------------------------------------------------------- mixed batch, guard
def _mixed():
    specs = [(wc.S16, 1, 16000, 2500), (wc.S24, 2, 24000, 1537 + 300), (wc.F32, 1, 44100, 2823 + 11), (wc.U8, 1, 8000, 600)]
    raws = [wc.quantise(wc.signal(n, 50 + i, C, sr=sr), k) for i, (k, C, sr, n) in enumerate(specs)]
    return specs, raws, [wc.wav_bytes(r, k, sr) for r, (k, C, sr, n) in zip(raws, specs)]


def test_mixed_batch_rows_equal_rows_alone(decoder):
    from asvspoof2021_air_amd import wav
    specs, raws, files = _mixed()
    pcm, status, ln, whole = _decode(decoder, files)
    assert status.tolist() == [0] * 4 and len(set(ln)) == 4 and _guards_intact(whole)
    first = pcm.clone()
    for b, f in enumerate(files):
        alone, st, l1, w1 = _decode(decoder, [f])
        assert st.tolist() == [0] and l1 == [ln[b]] and _guards_intact(w1)
        assert torch.equal(alone[0, :ln[b]], first[b, :ln[b]]), "row %d" % b
    got = first.cpu().numpy()
    for b, (r, (k, C, sr, n)) in enumerate(zip(raws, specs)):
        y, bound = ro.resample(wc.mono(wc.to_float(r, k)).astype(np.float64), sr)
        _within(got[b, :ln[b]], y, bound, "mixed row %d" % b)
    nine = [wc.wav_bytes(raws[0][:50], wc.S16, sr) for sr in (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000)]
    with pytest.raises(ValueError, match="9 distinct"):
        wav.pack(_items(nine))
    by, off, fr, fm, rate, l9 = wav.pack(_items(nine[:8]))
    with pytest.raises(ValueError, match="9 distinct"):
        decoder.decode(by.cuda(), torch.cat([off, off[-1:]]), torch.cat([fr, fr[:1]]), torch.cat([fm, fm[:1]]), rate + (48000,), Lcap=4000)
    pcm8, st8 = decoder.decode(by.cuda(), off, fr, fm, rate, Lcap=256)  # eight rates in one launch are served
    assert st8.tolist() == [0] * 8 and [int(torch.count_nonzero(pcm8[b, int(l9[b]):])) for b in range(8)] == [0] * 8


def test_length_guard(decoder):
    """Row 1's descriptor claims 8 frames more than its bytes hold: LENGTH_MISMATCH and zeros, the other rows bit-equal
    to the clean batch, check() names the row.  Then the last row of the buffer claiming a frame beyond the buffer's
    end, an output longer than the capacity, and an unknown format code."""
    from asvspoof2021_air_amd import wav
    specs, raws, files = _mixed()
    clean, st, ln, whole = _decode(decoder, files)
    clean = clean.clone()
    frames = [s[3] for s in specs]
    frames[1] += 8
    pcm, status, ln, whole = _decode(decoder, files, frames=frames)
    assert status.tolist() == [wav.OK, wav.LENGTH_MISMATCH, wav.OK, wav.OK] and _guards_intact(whole)
    assert int(torch.count_nonzero(pcm[1])) == 0
    for b in (0, 2, 3):
        assert torch.equal(pcm[b], clean[b])
    with pytest.raises(wav.WavError, match=r"row 1 LENGTH_MISMATCH") as e:
        wav.check(status)
    assert e.value.rows == [(1, wav.LENGTH_MISMATCH)]
    wav.check(status[:1])
    # the last row of the buffer claiming more than the buffer holds, and an output longer than the capacity
    by, off, fr, fm, rate, l4 = wav.pack(_items(files), bytes_round=1)
    fr2 = fr.clone()
    fr2[3] += 1
    assert int(l4.argmax()) == 0
    Lcap = int(l4.max()) - 1  # row 0 (the longest output) no longer fits
    whole = torch.full((4 * Lcap + 2 * GUARD,), FILL, dtype=torch.float32, device="cuda")
    out = whole[GUARD:GUARD + 4 * Lcap].view(4, Lcap)
    pcm, status = decoder.decode(by.cuda(), off, fr2, fm, rate, Lcap=Lcap, out=out)
    assert status.tolist() == [wav.LENGTH_MISMATCH, wav.OK, wav.OK, wav.LENGTH_MISMATCH] and _guards_intact(whole)
    assert int(torch.count_nonzero(pcm[0])) == 0 and int(torch.count_nonzero(pcm[3])) == 0
    assert torch.equal(pcm[1], clean[1, :Lcap]) and torch.equal(pcm[2], clean[2, :Lcap])
    # an unknown format code is a status too
    fm2 = fm.clone()
    fm2[0] = wav.fmt_code(wav.S16, 1) | (3 << 4)
    pcm, status = decoder.decode(by.cuda(), off, fr, fm2, rate, Lcap=int(l4.max()))
    assert status.tolist() == [wav.BAD_FORMAT, wav.OK, wav.OK, wav.OK] and int(torch.count_nonzero(pcm[0])) == 0


def test_default_capacity_and_the_ring(decoder):
    from asvspoof2021_air_amd import wav
    specs, raws, files = _mixed()
    by, off, fr, fm, rate, ln = wav.pack(_items(files))
    outs = [decoder.decode(by.cuda(), off, fr, fm, rate, check=True)[0] for _ in range(decoder.depth + 1)]
    assert outs[0].shape == (4, 16000) and outs[0].dtype == torch.float32
    assert len({o.data_ptr() for o in outs}) == decoder.depth and outs[0].data_ptr() == outs[-1].data_ptr()


# ---------------------------------------------------------------------------- corpus -> trainer
@contextlib.contextmanager
def no_host_sync():
    """Inside: Tensor.cpu / .item / .tolist / .numpy of a device tensor and every synchronize raise."""
    def refuse(name):
        def f(*a, **k):
            raise AssertionError("%s on the sync-free path" % name)
        return f

    def guard(name, orig):
        def f(self, *a, **k):
            if self.is_cuda:
                raise AssertionError("Tensor.%s of a device tensor on the sync-free path" % name)
            return orig(self, *a, **k)
        return f

    saved = {n: getattr(torch.Tensor, n) for n in ("cpu", "item", "tolist", "numpy")}
    sync = (torch.cuda.synchronize, torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize)
    try:
        for n, o in saved.items():
            setattr(torch.Tensor, n, guard(n, o))
        torch.cuda.synchronize = refuse("torch.cuda.synchronize")
        torch.cuda.Stream.synchronize = refuse("Stream.synchronize")
        torch.cuda.Event.synchronize = refuse("Event.synchronize")
        yield
    finally:
        for n, o in saved.items():
            setattr(torch.Tensor, n, o)
        torch.cuda.synchronize, torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize = sync


def _trainer(feat_len=96, seed=4242):
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.resnet import ResNet
    from asvspoof2021_air_amd.train import Trainer
    m = ResNet(3, 256, resnet_type="18", nclasses=2)
    fill_module_(m)
    m = m.cuda()
    m._noise_seed = seed
    m.overlap_wgrad = False
    lossm = AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)
    fill_module_(lossm)
    return m, Trainer(m, loss_module=lossm, feat_len=feat_len)


def test_no_host_sync_guard_works():
    with no_host_sync():
        with pytest.raises(AssertionError):
            torch.zeros(1, device="cuda").item()
        with pytest.raises(AssertionError):
            torch.cuda.synchronize()
        assert torch.zeros(1).item() == 0.0
    assert torch.zeros(1, device="cuda").item() == 0.0


def test_vcc2020_to_train_step(tmp_path, decoder):
    """VCC2020Raw -> DataLoader(collate_fn) -> DevicePrefetcher -> WavDecoder.decode(Lcap=16000) -> Trainer.step: six
    24 kHz files of 0.3 - 0.6 s, two steps, finite losses; the decoded batch within the bound of the oracle; no .cpu(),
    .item() or synchronise inside decode."""
    from torch.utils.data import DataLoader
    from asvspoof2021_air_amd import dataset as air_ds, raw_dataset
    seconds = [0.3, 0.36, 0.42, 0.48, 0.54, 0.6]
    rel = ["bonafide/source/SEF1/E10001", "bonafide/source/SEF2/E10002", "bonafide/target/TEF1/E20001",
           "spoof/T01/TEF1-SEF1/E30001", "spoof/T02/TEF1-SEF1/E30002", "spoof/T03/TEF1-SEF2/E30003"]
    waves = []
    for i, (r, s) in enumerate(zip(rel, seconds)):
        x = wc.quantise(wc.signal(int(s * 24000) + i, 200 + i, sr=24000), wc.S16)
        (tmp_path / r).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / (r + ".wav")).write_bytes(wc.wav_bytes(x, wc.S16, 24000))
        waves.append(x[:, 0])
    raw = raw_dataset.VCC2020Raw(str(tmp_path / "spoof"), str(tmp_path / "bonafide"), feat_len=96)
    assert len(raw) == 6
    m, tr = _trainer()
    np.random.seed(6)
    steps, k = [], 0
    for by, off, fr, fm, rate, ln, start, names, tag, label in air_ds.DevicePrefetcher(
            DataLoader(raw, batch_size=3, shuffle=False, collate_fn=raw.collate_fn, num_workers=0), "cuda"):
        assert by.is_cuda and by.dtype == torch.uint8 and ln.is_cuda and start.is_cuda and rate == (24000,) * 3
        assert list(label) == (["bonafide"] * 3 if k == 0 else ["spoof"] * 3)
        y = torch.tensor([{"bonafide": 0, "spoof": 1}[v] for v in label]).cuda()
        with no_host_sync():
            pcm, status = decoder.decode(by, off, fr, fm, rate, Lcap=16000)
        loss, neg = tr.step(pcm, y, start=start, lengths=ln)
        steps.append((loss.clone(), pcm.clone(), ln.clone(), status.clone()))
        k += 1
    assert len(steps) == 2
    for s, (loss, pcm, ln, status) in enumerate(steps):
        assert bool(torch.isfinite(loss).all()) and status.tolist() == [0, 0, 0] and pcm.shape == (3, 16000)
        got = pcm.cpu().numpy()
        for b in range(3):
            y, bound = ro.resample(waves[3 * s + b].astype(np.float64) / 32768.0, 24000)
            assert int(ln[b]) == len(y)
            _within(got[b, :len(y)], y, bound, "step %d row %d" % (s, b))
            assert not got[b, len(y):].any()
    w = raw.waveform(4)  # the reference's item[0]: (1, L) float at 16 kHz
    y, bound = ro.resample(waves[4].astype(np.float64) / 32768.0, 24000)
    assert w.shape == (1, len(y)) and w.dtype == torch.float32
    _within(w[0].cpu().numpy(), y, bound, "waveform(4)")


def test_8khz_flac_to_train_step(tmp_path):
    """ASVspoof2021evalRaw(resample=True) over 8 kHz FLAC: FlacDecoder.decode -> Resampler.resample(Lcap=16000) ->
    Trainer.step; both device calls free of host synchronisation."""
    from torch.utils.data import DataLoader
    from asvspoof2021_air_amd import dataset as air_ds, flac, raw_dataset, resample
    d = tmp_path / "flac"
    d.mkdir()
    waves = []
    for i, n in enumerate([2400, 3100, 4001, 4800]):  # 0.3 - 0.6 s at 8 kHz
        x = fc.signal(n, 300 + i)
        (d / ("LA_E_%07d.flac" % i)).write_bytes(fo.encode(x, 1152, [dict(type="fixed", order=2)], sample_rate=8000))
        waves.append(x)
    raw = raw_dataset.ASVspoof2021evalRaw(str(d), feat_len=96, resample=True)
    dec, rs = flac.FlacDecoder("cuda"), resample.Resampler("cuda")
    m, tr = _trainer()
    np.random.seed(6)
    steps = []
    for by, off, ln, bs, start, rate, out_ln, names in air_ds.DevicePrefetcher(
            DataLoader(raw, batch_size=2, shuffle=False, collate_fn=raw.collate_fn, num_workers=0), "cuda"):
        assert rate == (8000, 8000) and out_ln.is_cuda
        y = torch.tensor([0, 1]).cuda()
        with no_host_sync():
            pcm8, status = dec.decode(by, off, ln, bs, Lcap=8000)
            pcm, got_ln = rs.resample(pcm8, ln, rate, Lcap=16000)
        assert torch.equal(got_ln, out_ln)
        loss, neg = tr.step(pcm, y, start=start, lengths=out_ln)
        steps.append((loss.clone(), pcm.clone(), status.clone(), rs.last_status.clone()))
    assert len(steps) == 2
    for s, (loss, pcm, st, rst) in enumerate(steps):
        assert bool(torch.isfinite(loss).all()) and st.tolist() == [0, 0] and rst.tolist() == [0, 0]
        got = pcm.cpu().numpy()
        for b in range(2):
            y, bound = ro.resample(waves[2 * s + b].astype(np.float64) / 32768.0, 8000)
            _within(got[b, :len(y)], y, bound, "step %d row %d" % (s, b))
            assert not got[b, len(y):].any()
    w = raw.waveform(2)
    y, bound = ro.resample(waves[2].astype(np.float64) / 32768.0, 8000)
    assert w.shape == (1, len(y))
    _within(w[0].cpu().numpy(), y, bound, "waveform(2)")
