"""GPU: csrc/flac.hip (``flac.FlacDecoder``) against the oracle written from the format document (tests/flac_oracle.py).

FLAC decoding is integer arithmetic: every comparison here is exact (``torch.equal``).  The output and its padding are
pre-filled with 0x7fff, so a sample the decoder did not write, or a tail it did not zero, shows.  The streams are those of
tests/flac_cases.py; tests/test_flac_cpu.py round-trips each through the oracle encoder and decoder first."""
import numpy as np
import pytest
import torch

import flac_cases as fc
import flac_oracle as fo
from oracle.filler import fill_module_, synth_pcm

pytestmark = pytest.mark.gpu

FILL = 0x7fff
GUARD = 256  # canary samples in front of and behind the output


def _items(streams):
    from asvspoof2021_air_amd import flac
    out = []
    for buf in streams:
        info = flac.parse_stream(buf)
        out.append((torch.from_numpy(np.frombuffer(buf, dtype=np.uint8, offset=info.audio_offset).copy()), info))
    return out


@pytest.fixture(scope="module")
def decoder():
    from asvspoof2021_air_amd import flac
    return flac.FlacDecoder("cuda")


def _decode(decoder, streams, dtype=torch.int16, pad=37, lengths=None):
    """Decode `streams` as one batch into a pre-filled, guarded output -> (pcm, status, lengths list, guard tensor)."""
    from asvspoof2021_air_amd import flac
    items = _items(streams)
    by, off, ln, bs = flac.pack(items, bytes_round=256)
    if lengths is not None:
        ln = torch.tensor(lengths, dtype=torch.int32)
    B, Lcap = len(items), int(ln.max()) + pad
    fill = FILL if dtype == torch.int16 else float(FILL)
    whole = torch.full((B * Lcap + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    out = whole[GUARD:GUARD + B * Lcap].view(B, Lcap)
    pcm, status = decoder.decode(by.cuda(), off, ln, bs, Lcap=Lcap, dtype=dtype, out=out)
    assert pcm.data_ptr() == out.data_ptr() and status.dtype == torch.int32 and status.shape == (B,)
    return pcm, status, ln.tolist(), whole


def _check_rows(pcm, status, lengths, whole, want):
    """Every row OK, equal to `want` up to its length, zero beyond it; the guards untouched."""
    assert status.tolist() == [0] * len(want)
    for b, x in enumerate(want):
        n = lengths[b]
        assert n == len(x)
        assert torch.equal(pcm[b, :n].cpu(), torch.from_numpy(np.ascontiguousarray(x))), "row %d" % b
        assert int(torch.count_nonzero(pcm[b, n:])) == 0, "tail of row %d" % b
    assert bool((whole[:GUARD] == FILL).all()) and bool((whole[-GUARD:] == FILL).all())


@pytest.mark.parametrize("name", fc.SUBFRAME_TYPES + ["accumulator", "residual", "wasted", "header", "frame_numbers"])
def test_decode_equals_the_oracle(decoder, name):
    """Subframes (CONSTANT, VERBATIM, FIXED 0..4, LPC 1 / 8 / 32 at block sizes 16 / 192 / 4096 and lengths k bs, + 1, + 37),
    the 64-bit accumulator, the residual codings, wasted bits, every header code, 2,049 frame numbers: one launch per
    case over all its streams."""
    ss = fc.streams(name)
    want = [fo.decode(buf) for buf, _ in ss]
    for w, (_, x) in zip(want, ss):
        assert np.array_equal(w, x)
    _check_rows(*_decode(decoder, [buf for buf, _ in ss]), want)


def test_accumulator_case_needs_64_bits():
    """(the case is what it claims: the prediction sum leaves 32 bits, the residuals do not)"""
    x, bs, specs = fc.case("accumulator")[0]
    s = x[:192].astype(np.int64)
    c = specs[0]["coefs"]
    sums = [sum(c[j] * int(s[i - 1 - j]) for j in range(32)) for i in range(32, 192)]
    assert max(abs(v) for v in sums) > 1.6e10
    assert np.abs(fo.residual_of(s, c, 14)).max() < 2 ** 31


def test_false_sync_is_never_decoded(decoder):
    (x, bs, specs), inner = fc.false_sync_row()
    buf = fc.streams("false_sync")[0][0]
    assert inner in buf
    pcm, status, lengths, whole = _decode(decoder, [buf])
    _check_rows(pcm, status, lengths, whole, [fo.decode(buf)])
    # the embedded frame would decode to 192 samples of FALSE_VALUE at frame 1: the value appears once, as payload
    assert int((pcm[0] == fc.FALSE_VALUE).sum()) == 1 == int((x == fc.FALSE_VALUE).sum())


def test_ragged_batch(decoder):
    """B = 5 rows of different lengths (1 sample .. 3 x 4096 + 37) and block sizes in one launch; each row alone and a
    second call give the same bits; float32 is int16 / 32768 exactly."""
    ss = fc.streams("ragged")
    bufs = [buf for buf, _ in ss]
    want = [fo.decode(buf) for buf in bufs]
    assert [len(w) for w in want] == [1, 3 * 4096 + 37, 83, 192 * 7, 4096]
    pcm, status, lengths, whole = _decode(decoder, bufs)
    _check_rows(pcm, status, lengths, whole, want)
    first = pcm.clone()
    again = _decode(decoder, bufs)
    _check_rows(*again, want)
    assert torch.equal(again[0], first)
    for b, buf in enumerate(bufs):
        alone = _decode(decoder, [buf])
        _check_rows(*alone, [want[b]])
        assert torch.equal(alone[0][0, :lengths[b]], first[b, :lengths[b]])
    f32 = _decode(decoder, bufs, dtype=torch.float32)
    assert f32[1].tolist() == [0] * 5 and f32[0].dtype == torch.float32
    assert torch.equal(f32[0], first.to(torch.float32) / 32768.0)
    assert bool((f32[3][:GUARD] == float(FILL)).all()) and bool((f32[3][-GUARD:] == float(FILL)).all())


def test_default_capacity_and_the_ring(decoder):
    from asvspoof2021_air_amd import flac
    bufs = [buf for buf, _ in fc.streams("ragged")]
    by, off, ln, bs = flac.pack(_items(bufs))
    outs = [decoder.decode(by.cuda(), off, ln, bs, check=True)[0] for _ in range(decoder.depth + 1)]
    assert outs[0].shape == (5, 16000) and outs[0].dtype == torch.int16  # the longest row rounded up to RAGGED_ROUND
    assert len({o.data_ptr() for o in outs}) == decoder.depth and outs[0].data_ptr() == outs[-1].data_ptr()
    for b, buf in enumerate(bufs):
        assert flac.verify_md5(outs[-1][b], flac.parse_stream(buf))


def test_errors_stay_errors(decoder):
    """Row 1: one flipped residual bit; row 2: cut 5 bytes short; row 3: an inflated length.  Row 0 is intact and exact,
    every tail is zero, check() names rows 1 - 3.  Ordinary inputs to a bounds-checked parser."""
    from asvspoof2021_air_amd import flac
    ss = fc.streams("ragged")
    bufs = [ss[3][0], ss[1][0], ss[2][0][:-5], ss[4][0]]
    flipped = bytearray(bufs[1])
    flipped[len(flipped) // 2] ^= 0x10
    bufs[1] = bytes(flipped)
    lengths = [len(ss[3][1]), len(ss[1][1]), len(ss[2][1]), len(ss[4][1]) + 1]
    pcm, status, ln, whole = _decode(decoder, bufs, lengths=lengths)
    st = status.tolist()
    assert st[0] == flac.OK and st[1] in (flac.BAD_CRC16, flac.LOST_SYNC) and st[2] == flac.LOST_SYNC
    assert st[3] == flac.LENGTH_MISMATCH
    assert torch.equal(pcm[0, :lengths[0]].cpu(), torch.from_numpy(fo.decode(ss[3][0])))
    for b, n in enumerate(lengths):
        assert int(torch.count_nonzero(pcm[b, n:])) == 0
    assert bool((whole[:GUARD] == FILL).all()) and bool((whole[-GUARD:] == FILL).all())
    with pytest.raises(flac.FlacError, match=r"row 1 .*row 2 LOST_SYNC.*row 3 LENGTH_MISMATCH") as e:
        decoder.check(status)
    assert [r for r, _ in e.value.rows] == [1, 2, 3]
    decoder.check(status[:1])


def test_damaged_last_row_reads_nothing_behind_the_buffer(decoder):
    """The row cut 5 bytes short is the LAST of the buffer, and the 5 missing bytes (+ canaries) lie right behind the
    declared total_bytes: a reader that ran past the end would find them and report the row OK.  The neighbouring
    row's output and the guards around the output are untouched."""
    from asvspoof2021_air_amd import flac
    ss = fc.streams("ragged")
    good, cut = ss[3][0], ss[2][0]
    items = _items([good, cut[:-5]])
    by, off, ln, bs = flac.pack(items, bytes_round=1)
    total = int(off[-1])
    assert by.numel() == total
    behind = torch.cat([by, torch.from_numpy(np.frombuffer(cut[-5:], dtype=np.uint8).copy()),
                        torch.full((59,), 0xA5, dtype=torch.uint8)]).cuda()
    B, Lcap = 2, int(ln.max()) + 5
    whole = torch.full((B * Lcap + 2 * GUARD,), FILL, dtype=torch.int16, device="cuda")
    out = whole[GUARD:GUARD + B * Lcap].view(B, Lcap)
    pcm, status = decoder.decode(behind[:total], off, ln, bs, Lcap=Lcap, out=out)
    assert status.tolist() == [flac.OK, flac.LOST_SYNC]
    n = int(ln[0])
    assert torch.equal(pcm[0, :n].cpu(), torch.from_numpy(fo.decode(good))) and int(torch.count_nonzero(pcm[0, n:])) == 0
    assert int(torch.count_nonzero(pcm[1, int(ln[1]):])) == 0
    assert bool((whole[:GUARD] == FILL).all()) and bool((whole[-GUARD:] == FILL).all())
    assert bool((behind[total + 5:] == 0xA5).all())
    # the whole stream, declared whole, decodes
    _check_rows(*_decode(decoder, [good, cut]), [fo.decode(good), fo.decode(cut)])


def test_unsupported_frames_are_a_status(decoder):
    """Stereo assignment, negative LPC shift, precision code 1111, another sample size - each in the middle frame of a
    stream - are UNSUPPORTED; the intact row beside them decodes."""
    from asvspoof2021_air_amd import flac
    bufs = [fo.encode(x, bs, specs) for x, bs, specs in fc.unsupported_rows()] + [fc.streams("ragged")[2][0]]
    pcm, status, lengths, whole = _decode(decoder, bufs)
    assert status.tolist() == [flac.UNSUPPORTED] * 4 + [flac.OK]
    assert torch.equal(pcm[4, :lengths[4]].cpu(), torch.from_numpy(fc.streams("ragged")[2][1]))
    for b, n in enumerate(lengths):
        assert int(torch.count_nonzero(pcm[b, n:])) == 0


def test_verify_md5(decoder):
    from asvspoof2021_air_amd import flac
    bufs = [buf for buf, _ in fc.streams("wasted")]
    pcm, status, lengths, whole = _decode(decoder, bufs)
    assert status.tolist() == [0] * len(bufs)
    for b, buf in enumerate(bufs):
        assert flac.verify_md5(pcm[b], flac.parse_stream(buf))
    pcm[2, 5] += 1
    assert not flac.verify_md5(pcm[2], flac.parse_stream(bufs[2]))


# ---------------------------------------------------------------------------- corpus -> trainer
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


def test_corpus_to_train_step(tmp_path, decoder):
    """raw_dataset collate -> DevicePrefetcher -> decode -> Trainer.step(start=, lengths=) gives the loss and the scores,
    bit for bit, of the same step fed by PCMSource(return_pcm='ragged') over the oracle-decoded int16 waveforms."""
    from torch.utils.data import DataLoader
    from asvspoof2021_air_amd import dataset as air_ds, raw_dataset
    lengths = [8000, 12345, 16000, 19200]  # 0.5 - 1.2 s; 96 frames = 15360 samples: two rows are cropped
    cap = 32000
    wav = (synth_pcm(4, max(lengths), seed=55) * 32768.0).round().clamp(-32768, 32767).to(torch.int16).numpy()
    tags = ["-", "A03", "A11", "-"]
    labels = ["bonafide" if t == "-" else "spoof" for t in tags]
    audio = tmp_path / "db" / "LA" / "ASVspoof2019_LA_train" / "flac"
    audio.mkdir(parents=True)
    (tmp_path / "proto").mkdir()
    mixed = [dict(type="fixed", order=2), fc.lpc_spec(8, 9), dict(type="fixed", order=3, partition_order=4), fc.lpc_spec(32, 9)]
    lines, items = [], []
    for i, n in enumerate(lengths):
        name = "LA_T_%07d" % (1000000 + i)
        buf = fo.encode(wav[i, :n], 4096, mixed)
        (audio / (name + ".flac")).write_bytes(buf)
        lines.append("LA_%04d %s - %s %s" % (i, name, tags[i], labels[i]))
        items.append(("%05d_%s_%s_%s" % (i, name, tags[i], labels[i]), torch.from_numpy(fo.decode(buf))))
    (tmp_path / "proto" / "ASVspoof2019.LA.cm.train.trl.txt").write_text("\n".join(lines) + "\n")

    raw = raw_dataset.ASVspoof2019Raw("LA", str(tmp_path / "db"), str(tmp_path / "proto"), "train", feat_len=96)
    m, tr = _trainer()
    np.random.seed(6)
    got = None
    for by, off, ln, bs, start, names, tag, label in air_ds.DevicePrefetcher(
            DataLoader(raw, batch_size=4, shuffle=False, collate_fn=raw.collate_fn, num_workers=0), "cuda"):
        assert by.is_cuda and by.dtype == torch.uint8 and start.is_cuda and list(names) == [l.split()[1] for l in lines]
        pcm, status = decoder.decode(by, off, ln, bs, Lcap=cap)
        y = torch.tensor([raw.label[v] for v in label]).cuda()
        loss, neg = tr.step(pcm, y, start=start, lengths=ln)
        decoder.check(status)
        got = (loss.clone(), neg.clone(), pcm.clone(), start.clone())
    assert int(torch.count_nonzero(got[3])) >= 1

    ref = air_ds.ASVspoof2019("LA", None, "train", feat_len=96, source=air_ds.PCMSource(items), return_pcm="ragged")
    ref.ragged_samples = cap
    m2, tr2 = _trainer()
    np.random.seed(6)
    for pcm, ln, start, names, tag, label in air_ds.DevicePrefetcher(
            DataLoader(ref, batch_size=4, shuffle=False, collate_fn=ref.collate_fn, num_workers=0), "cuda"):
        assert torch.equal(pcm, got[2]) and torch.equal(start, got[3])
        loss, neg = tr2.step(pcm, label, start=start, lengths=ln)
        assert torch.equal(loss, got[0]) and torch.equal(neg, got[1])
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
    # the reference's item[0]: one file to the (1, L) float waveform
    w = raw.waveform(1)
    assert w.shape == (1, lengths[1]) and w.dtype == torch.float32
    assert torch.equal(w[0].cpu(), torch.from_numpy(wav[1, :lengths[1]]).to(torch.float32) / 32768.0)
