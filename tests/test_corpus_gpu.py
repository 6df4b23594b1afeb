"""GPU: the device corpus (corpus.py, csrc/corpus.hip) against tests/corpus_oracle.py - every comparison exact."""
import numpy as np
import pytest
import torch

import corpus_oracle as co
import flac_cases as fc
import flac_oracle as fo
from oracle.filler import fill_module_, synth_pcm

pytestmark = pytest.mark.gpu

SEED = 688
LCAP = 8192
DTYPES = [torch.int16, torch.float32]


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------- permutation
def test_permutation_equals_the_oracle():
    from asvspoof2021_air_amd import _hip, ops
    E = _hip.lib().air_eval_sort_block()
    for n in (1, 2, 3, E - 1, E, E + 1, 2 * E + 1, 25380):
        for lo, generation, flow in ((0, 0, 0), (1000, 7, 1)):
            got = ops.corpus_permutation(lo, n, SEED, ops.corpus_stream(generation, flow))
            assert got.dtype == torch.int64 and np.array_equal(_np(got), co.permutation(lo, n, SEED, generation, flow)), (n, lo)
    with pytest.raises(ValueError):
        ops.corpus_permutation(0, (1 << 20) + 1, SEED, 0)
    out = torch.empty(4, dtype=torch.int64, device="cuda")
    import ctypes
    rc = _hip.lib().air_corpus_permutation(ctypes.c_int64(0), _hip.ci((1 << 20) + 1), ctypes.c_uint64(SEED), ctypes.c_uint32(0),
                                           _hip.dptr(out, torch.int64), _hip.dptr(out, torch.int64), _hip.csz(32),
                                           ctypes.c_void_p(0))
    assert rc == -2  # AIR_EUNSUPPORTED: refused before anything is launched


# ---------------------------------------------------------------------------- pack and gather
def _lengths(dtype):
    from asvspoof2021_air_amd import ops
    tile = ops.corpus_copy_tile(dtype)
    assert tile + 1 < LCAP
    # the edges the issue names, then T == feat_len (1440 .. 1599) and T == feat_len + 1 (1600 .. 1759) at feat_len 10
    return [1, 7, 8, 9, 15, 16, 17, 159, 160, 161, tile - 1, tile, tile + 1, LCAP - 1, LCAP,
            1440, 1599, 1600, 1759, 1760, 3001, 5000, 6007, 64]


def _utterances(dtype, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for n in _lengths(dtype):
        if dtype == torch.int16:
            v = rng.integers(1, 32767, n).astype(np.int16) * rng.choice(np.array([-1, 1], dtype=np.int16), n)
        else:
            v = (rng.standard_normal(n) + 3.0).astype(np.float32)
        assert np.all(v != 0)
        out.append(v)
    return out


def _meta(n):
    labels = (np.arange(n) * 7 + 1) % 2
    tags = (np.arange(n) * 5) % 20
    channels = np.stack([(np.arange(n) * 3) % 59, (np.arange(n) * 11) % 13], axis=1)
    return labels, tags, channels


def _ragged(rows, cap, dtype, fill=77):
    """A (B, cap) device batch whose tails hold ``fill``: append must not care what lies behind a row's length."""
    host = np.full((len(rows), cap), fill, dtype=rows[0].dtype)
    for b, r in enumerate(rows):
        host[b, :len(r)] = r
    return torch.from_numpy(host).to("cuda")


def _build(dtype, with_channels=True):
    from asvspoof2021_air_amd.corpus import DeviceCorpus
    utts = _utterances(dtype)
    labels, tags, channels = _meta(len(utts))
    corpus = DeviceCorpus(dtype)
    # three appends: B = 10 / 9 / 5, source capacities 8192 / 8197 (rows off the 16-byte grid: the element-wise route) / 8200
    lo = 0
    for B, cap in ((10, 8192), (9, 8197), (5, 8200)):
        rows = utts[lo:lo + B]
        first = corpus.append(_ragged(rows, cap, dtype), [len(r) for r in rows], torch.from_numpy(labels[lo:lo + B]),
                              tags[lo:lo + B], channels[lo:lo + B] if with_channels else None)
        assert first == lo
        lo += B
    assert lo == len(utts) == len(corpus)
    return corpus, utts, labels, tags, channels


@pytest.fixture(scope="module", params=DTYPES, ids=["int16", "float32"])
def built(request):
    return (request.param,) + _build(request.param)


def test_store_layout(built):
    dtype, corpus, utts, labels, tags, channels = built
    lens = np.array([len(u) for u in utts])
    assert np.array_equal(_np(corpus.offsets), co.store_offsets(lens)) and corpus.offsets.dtype == torch.int64
    assert np.all(_np(corpus.offsets) % 8 == 0)
    assert corpus.lengths.dtype == torch.int32 and np.array_equal(_np(corpus.lengths), lens)
    assert np.array_equal(corpus.host_lengths, lens)
    for name, want in (("labels", labels), ("tags", tags), ("index", np.arange(len(utts))), ("channels", channels)):
        t = getattr(corpus, name)
        assert t.dtype == torch.int64 and np.array_equal(_np(t), want), name
    for i, u in enumerate(utts):
        assert np.array_equal(_np(corpus.row(i)), u), i
    assert corpus.samples.numel() == co.store_offsets(lens)[-1] and corpus.samples.dtype == dtype


def _check_batch(batch, want, dtype):
    assert batch.pcm.dtype == dtype and batch.lengths.dtype == torch.int32 and batch.start.dtype == torch.int32
    for name in ("pcm", "labels", "start", "lengths", "tags", "channels", "index"):
        got = getattr(batch, name)
        if want[name] is None:
            assert got is None, name
        else:
            assert np.array_equal(_np(got), want[name]), name


def test_round_trip_and_crop(built):
    """Every gathered row equals its source, [len, Lcap) is zero over a pre-filled buffer, the tables and the crop
    offsets (feat_len 10) are the oracle's."""
    from asvspoof2021_air_amd import ops
    dtype, corpus, utts, labels, tags, channels = built
    n, feat_len = len(utts), 10
    lens = np.array([len(u) for u in utts])
    sampler = corpus.sampler(n, seed=SEED, shuffle=False, Lcap=LCAP, feat_len=feat_len)
    assert len(sampler) == 1
    batches = list(sampler.epoch())
    assert len(batches) == 1
    want = co.gather(np.arange(n), utts, labels, tags, channels, LCAP, SEED, [0] * n, feat_len)
    _check_batch(batches[0], want, dtype)
    # the crop rule at its edges
    T = 1 + lens // 160
    start = _np(batches[0].start)
    assert np.all(start[T <= feat_len + 1] == 0) and np.any(T == feat_len) and np.any(T == feat_len + 1)
    assert np.all((start >= 0) & (start < np.maximum(T - feat_len, 1))) and np.any(start > 0)
    # shuffled, into a buffer that held something else: the same rows in the permutation's order
    for generation in (0, 1):
        perm = ops.corpus_permutation(0, n, SEED, ops.corpus_stream(generation, 0))
        junk = torch.full((n, LCAP), 23130 if dtype == torch.int16 else 1.5, dtype=dtype, device="cuda")
        c = corpus
        out = ops.corpus_gather(c.samples, c.offsets, c.lengths, c.labels, c.tags, c.index, c.channels, n,
                                [(perm, 0, n, generation)], SEED, feat_len, 160, LCAP, pcm=junk)
        assert out[0] is junk
        rows = co.permutation(0, n, SEED, generation, 0)
        want = co.gather(rows, utts, labels, tags, channels, LCAP, SEED, [generation] * n, feat_len)
        got = dict(zip(("pcm", "labels", "start", "lengths", "tags", "channels", "index"), out))
        for name, w in want.items():
            assert np.array_equal(_np(got[name]), w), (name, generation)


@pytest.mark.parametrize("dtype", DTYPES, ids=["int16", "float32"])
def test_gather_masks_by_length(dtype):
    """A hand-built store whose alignment gaps hold a non-zero value: nothing of them reaches a batch."""
    from asvspoof2021_air_amd import ops
    utts = _utterances(dtype, seed=9)
    n = len(utts)
    labels, tags, _ = _meta(n)
    lens = np.array([len(u) for u in utts], dtype=np.int32)
    off = co.store_offsets(lens)
    host = np.full(off[-1], 30583 if dtype == torch.int16 else -7.25, dtype=utts[0].dtype)
    for i, u in enumerate(utts):
        host[off[i]:off[i] + len(u)] = u
    dev = [torch.from_numpy(a).cuda() for a in (host, off, lens, labels.astype(np.int64), tags.astype(np.int64),
                                                 np.arange(n, dtype=np.int64) + 100)]
    rows = np.array([n - 1, 0, 5, 13, 14, 2, 10, 11, 12], dtype=np.int64)
    perm = torch.from_numpy(rows).cuda()
    junk = torch.full((len(rows), LCAP), 21845 if dtype == torch.int16 else 9.0, dtype=dtype, device="cuda")
    out = ops.corpus_gather(dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], None, n, [(perm, 0, 4, 2), (perm, 4, 5, 3)],
                            SEED, 10, 160, LCAP, pcm=junk)
    want = co.gather(rows, utts, labels, tags, None, LCAP, SEED, [2] * 4 + [3] * 5, 10)
    want["index"] = rows + 100
    got = dict(zip(("pcm", "labels", "start", "lengths", "tags", "channels", "index"), out))
    assert got["channels"] is None
    for name, w in want.items():
        if w is not None:
            assert np.array_equal(_np(got[name]), w), name
    # the copy on its own, packing rows that sit off the 16-byte grid into a strided destination
    src = _ragged(utts[:6], LCAP + 3, dtype)
    dst = torch.full((6, LCAP), 21845 if dtype == torch.int16 else 9.0, dtype=dtype, device="cuda")
    ops.corpus_copy_rows(src, dst, dev[2][:6].contiguous(), int(lens[:6].max()), src_stride=LCAP + 3, dst_stride=LCAP,
                         dst_cap=LCAP)
    assert np.array_equal(_np(dst), co.gather(np.arange(6), utts, labels, tags, None, LCAP, SEED, [0] * 6, 10)["pcm"])


def test_refusals(built):
    dtype, corpus = built[0], built[1]
    with pytest.raises(ValueError):
        corpus.sampler(4, Lcap=LCAP + 4)
    with pytest.raises(ValueError):
        corpus.sampler(4, Lcap=LCAP - 8)
    with pytest.raises(ValueError):
        corpus.sampler(4, ranges=[(0, len(corpus) + 1)])
    with pytest.raises(ValueError):
        corpus.append(torch.zeros((2, 16), dtype=dtype, device="cuda"), [4, 17], [0, 1], channels=[1, 2])
    with pytest.raises(ValueError):
        corpus.append(torch.zeros((2, 16), dtype=dtype, device="cuda"), torch.tensor([4, 5]).cuda(), [0, 1], channels=[[1, 2]] * 2)
    assert corpus.sampler(4, ranges=[(0, 3)]).Lcap == 16000


# ---------------------------------------------------------------------------- epochs, ranks, flows
@pytest.fixture(scope="module")
def small():
    """33 short utterances (8 .. 200 samples), grown from an unreserved store."""
    from asvspoof2021_air_amd.corpus import DeviceCorpus
    rng = np.random.default_rng(11)
    utts = [rng.integers(-3000, 3000, int(n)).astype(np.int16) for n in rng.integers(8, 200, 33)]
    labels = np.arange(33) % 2
    corpus = DeviceCorpus(torch.int16)
    for lo in range(0, 33, 11):
        rows = utts[lo:lo + 11]
        corpus.append(_ragged(rows, 200, torch.int16), [len(r) for r in rows], labels[lo:lo + 11])
    assert corpus.channels is None and np.array_equal(_np(corpus.tags), np.zeros(33))
    return corpus, utts, labels


def _epoch(sampler):
    return [tuple(None if t is None else _np(t) for t in b) for b in sampler.epoch()]


def _same(a, b):
    return len(a) == len(b) and all(
        (x is None and y is None) or np.array_equal(x, y) for ba, bb in zip(a, b) for x, y in zip(ba, bb))


def test_epochs_and_ranks(small):
    corpus, utts, labels = small
    n = len(utts)
    s = corpus.sampler(4, seed=SEED, Lcap=200, feat_len=1, hop=16)
    assert len(s) == n // 4
    e0, e1 = _epoch(s), _epoch(s)
    for e, ep in enumerate((e0, e1)):
        idx = np.concatenate([b[6] for b in ep])
        assert len(ep) == len(s) and len(set(idx.tolist())) == len(idx) == (n // 4) * 4
        assert np.array_equal(idx, co.permutation(0, n, SEED, e, 0)[:len(idx)])
        for b in ep:
            want = co.gather(b[6], utts, labels, np.zeros(n), None, 200, SEED, [e] * 4, 1, 16)
            assert all(np.array_equal(b[k], want[name]) for k, name in enumerate(
                ("pcm", "labels", "start", "lengths", "tags")))
    assert not np.array_equal(np.concatenate([b[6] for b in e0]), np.concatenate([b[6] for b in e1]))
    assert any(np.any(b[2] > 0) for b in e0)
    again = corpus.sampler(4, seed=SEED, Lcap=200, feat_len=1, hop=16)
    assert _same(_epoch(again), e0) and _same(_epoch(again), e1)
    assert not _same(_epoch(corpus.sampler(4, seed=SEED + 1, Lcap=200, feat_len=1, hop=16)), e0)
    # a state taken in the middle of an epoch resumes there
    s2 = corpus.sampler(4, seed=SEED, Lcap=200, feat_len=1, hop=16)
    _epoch(s2)
    it = s2.epoch()
    head = [tuple(None if t is None else _np(t) for t in next(it)) for _ in range(3)]
    s3 = corpus.sampler(4, seed=SEED, Lcap=200, feat_len=1, hop=16)
    s3.load_state_dict(s2.state_dict())
    tail = [tuple(None if t is None else _np(t) for t in b) for b in s3.resume()]
    assert _same(head + tail, e1)
    # two ranks in one process: disjoint, together the world = 1 batches of twice the size
    one = _epoch(corpus.sampler(8, seed=SEED, Lcap=200, feat_len=1, hop=16, rank=0, world=1))
    r0 = _epoch(corpus.sampler(4, seed=SEED, Lcap=200, feat_len=1, hop=16, rank=0, world=2))
    r1 = _epoch(corpus.sampler(4, seed=SEED, Lcap=200, feat_len=1, hop=16, rank=1, world=2))
    assert len(one) == len(r0) == len(r1) == n // 8
    for b, b0, b1 in zip(one, r0, r1):
        assert not set(b0[6].tolist()) & set(b1[6].tolist())
        for k in (0, 1, 2, 3, 4, 6):
            assert np.array_equal(b[k], np.concatenate([b0[k], b1[k]])), k


def test_two_flows(small):
    corpus, utts, labels = small
    ranges, B = [(0, 20), (20, 33)], 8
    s = corpus.sampler(B, seed=SEED, ranges=ranges, ratio=0.5, Lcap=200, feat_len=1, hop=16)
    assert len(s) == 5
    want = co.schedule(ranges, B, 3, ratio=0.5)
    cache, gens_seen = {}, []
    for e in range(3):
        got = _epoch(s)
        assert len(got) == 5
        for b, segs in zip(got, want[e]):
            rows, gens = co.step_rows(segs, ranges, SEED, cache=cache)
            assert np.all(b[6][:4] < 20) and np.all(b[6][4:] >= 20)
            w = co.gather(rows, utts, labels, np.zeros(33), None, 200, SEED, gens, 1, 16)
            assert all(np.array_equal(b[k], w[name]) for k, name in enumerate(("pcm", "labels", "start", "lengths", "tags")))
            assert np.array_equal(b[6], rows)
            gens_seen.append(segs[1][1])
    assert gens_seen[0] == 0 and gens_seen[-1] >= 3 and gens_seen == sorted(gens_seen)  # 13 rows last three steps


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


AUDIO_CAP = 32000  # the ragged shape of tests/test_flac_gpu.py: B = 4, 0.5 - 1.2 s rows in (4, 32000), feat_len 96


@pytest.fixture(scope="module")
def audio():
    from asvspoof2021_air_amd.corpus import DeviceCorpus
    lengths = [8000, 12345, 16000, 19200, 9000, 17000, 15360, 15519, 15520, 18000, 8001, 19999, 10000, 16400]
    wav = (synth_pcm(len(lengths), max(lengths), seed=55) * 32768.0).round().clamp(-32768, 32767).to(torch.int16).numpy()
    utts = [wav[i, :n].copy() for i, n in enumerate(lengths)]
    labels = np.array([0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 1, 1, 0, 1])
    corpus = DeviceCorpus(torch.int16).reserve(sum(lengths) + 8 * len(lengths), len(lengths))
    corpus.append(_ragged(utts, 20000, torch.int16, fill=0), lengths, labels)
    return corpus, utts, labels


def test_unshuffled_walk_feeds_evaluate(audio):
    corpus, utts, labels = audio
    s = corpus.sampler(4, shuffle=False, ranges=[(2, 12)], Lcap=AUDIO_CAP, feat_len=96)
    assert len(s) == 3
    got = _epoch(s)
    assert [len(b[6]) for b in got] == [4, 4, 2]
    assert np.array_equal(np.concatenate([b[6] for b in got]), np.arange(2, 12))
    for k, b in enumerate(got):
        rows = np.arange(2 + 4 * k, min(12, 6 + 4 * k))
        w = co.gather(rows, utts, labels, np.zeros(len(utts)), None, AUDIO_CAP, 688, [0] * len(rows), 96)
        assert all(np.array_equal(b[j], w[name]) for j, name in enumerate(("pcm", "labels", "start", "lengths", "tags")))
    _, tr = _trainer()
    res = tr.evaluate(s.epoch())
    assert res.scores.numel() == 10 and np.array_equal(_np(res.labels), labels[2:12])
    assert np.isfinite(res.loss) and 0.0 <= res.eer <= 1.0


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_trainer_steps_equal_host_collated_rows(audio, graph):
    """Three steps fed from sampler.epoch() against three steps fed the oracle's rows, collated on the host: the same
    loss bits and the same parameter arena."""
    corpus, utts, labels = audio
    n = len(utts)
    m1, tr1 = _trainer()
    m2, tr2 = _trainer()
    if graph:
        tr1.enable_graph()
        tr2.enable_graph()
    s = corpus.sampler(4, seed=SEED, Lcap=AUDIO_CAP, feat_len=96)
    assert len(s) == 3
    got = [tr1.step(b.pcm, b.labels, start=b.start, lengths=b.lengths)[0].clone() for b in s.epoch()]
    want_segs = co.schedule([(0, n)], 4, 1)[0]
    cropped = 0
    for k, segs in enumerate(want_segs):
        rows, gens = co.step_rows(segs, [(0, n)], SEED)
        w = co.gather(rows, utts, labels, np.zeros(n), None, AUDIO_CAP, SEED, gens, 96)
        cropped += int(np.count_nonzero(w["start"]))
        loss, _ = tr2.step(torch.from_numpy(w["pcm"]).cuda(), torch.from_numpy(w["labels"]).cuda(),
                           start=torch.from_numpy(w["start"]).cuda(), lengths=torch.from_numpy(w["lengths"]).cuda())
        assert torch.equal(loss, got[k]) and bool(torch.isfinite(loss)), k
    assert len(got) == 3 and cropped >= 1
    assert torch.equal(m1.arena().flat, m2.arena().flat)
    if graph:
        assert tr1._graph is not None and tr2._graph is not None


def test_train_epoch_log_and_copies(audio, tmp_path, monkeypatch):
    corpus, utts, labels = audio
    m1, tr1 = _trainer()
    m2, tr2 = _trainer()
    for tr, sub in ((tr1, "a"), (tr2, "b")):
        tr.set_out_fold(str(tmp_path / sub))
        b = next(corpus.sampler(4, seed=1, Lcap=AUDIO_CAP, feat_len=96).epoch())
        tr.features(b.pcm, b.start, b.lengths)  # (the front-end's plan is built on first use, from the host)
    s1 = corpus.sampler(4, seed=SEED, Lcap=AUDIO_CAP, feat_len=96)
    s2 = corpus.sampler(4, seed=SEED, Lcap=AUDIO_CAP, feat_len=96)
    copies, items = [], []
    real_cpu, real_item = torch.Tensor.cpu, torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **kw: (copies.append(t.numel()), real_cpu(t, *a, **kw))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda t, *a, **kw: (items.append(t.numel()), real_item(t, *a, **kw))[1])
    host = [tr1.train_epoch(s1.epoch(), e) for e in (0, 1)]
    assert copies == [3, 3] and items == []  # one device-to-host copy per epoch, no .item()
    monkeypatch.undo()
    want = []
    for e in (0, 1):
        tr2.set_epoch(e)
        for i, b in enumerate(s2.epoch()):
            loss, _ = tr2.step(b.pcm, b.labels, start=b.start, lengths=b.lengths)
            tr2.log_step(e, i, loss)
            want.append(loss.item())
    assert all(h.dtype == np.float32 and h.shape == (3,) for h in host)
    assert np.array_equal(np.concatenate(host), np.array(want, dtype=np.float32))
    a = (tmp_path / "a" / "train_loss.log").read_bytes()
    assert a == (tmp_path / "b" / "train_loss.log").read_bytes() and a.count(b"\n") == 6
    assert torch.equal(m1.arena().flat, m2.arena().flat)


# ---------------------------------------------------------------------------- from_dataset
def test_from_dataset(tmp_path):
    from asvspoof2021_air_amd import dataset as air_ds, raw_dataset
    from asvspoof2021_air_amd.corpus import DeviceCorpus
    lengths = [4096, 5000, 8192, 8193, 4500, 6000, 9001]
    wav = (synth_pcm(len(lengths), max(lengths), seed=21) * 32768.0).round().clamp(-32768, 32767).to(torch.int16).numpy()
    tags = ["-", "A03", "A06", "-", "A02", "A01", "-"]  # (in the tables of the 2019 set and of the *_aug sets)
    labels = ["bonafide" if t == "-" else "spoof" for t in tags]
    audio_dir = tmp_path / "db" / "LA" / "ASVspoof2019_LA_train" / "flac"
    audio_dir.mkdir(parents=True)
    (tmp_path / "proto").mkdir()
    specs = [dict(type="fixed", order=2), fc.lpc_spec(8, 9)]
    lines, items, decoded = [], [], []
    for i, n in enumerate(lengths):
        name = "LA_T_%07d" % (1000000 + i)
        buf = fo.encode(wav[i, :n], 4096, specs)
        (audio_dir / (name + ".flac")).write_bytes(buf)
        lines.append("LA_%04d %s - %s %s" % (i, name, tags[i], labels[i]))
        decoded.append(fo.decode(buf))
        items.append(("%05d_%s_%s_%s" % (i, name, tags[i], labels[i]), torch.from_numpy(decoded[-1])))
    (tmp_path / "proto" / "ASVspoof2019.LA.cm.train.trl.txt").write_text("\n".join(lines) + "\n")
    want_tags = np.array([air_ds.TAG_LA19[t] for t in tags])
    want_labels = np.array([air_ds.LABEL[v] for v in labels])

    raw = raw_dataset.ASVspoof2019Raw("LA", str(tmp_path / "db"), str(tmp_path / "proto"), "train")
    ref = air_ds.ASVspoof2019("LA", None, "train", source=air_ds.PCMSource(items), return_pcm="ragged")
    for ds in (raw, ref):
        corpus = DeviceCorpus.from_dataset(ds, batch_size=3)
        assert len(corpus) == len(lengths) and corpus.dtype == torch.int16 and corpus.channels is None
        for i, d in enumerate(decoded):
            assert np.array_equal(_np(corpus.row(i)), d), i
        assert np.array_equal(_np(corpus.labels), want_labels) and np.array_equal(_np(corpus.tags), want_tags)
        assert np.array_equal(_np(corpus.index), np.arange(len(lengths)))
    as_float = DeviceCorpus.from_dataset(raw, batch_size=4, dtype=torch.float32)
    for i, d in enumerate(decoded):
        assert np.array_equal(_np(as_float.row(i)), d.astype(np.float32) / np.float32(32768.0)), i
    with pytest.raises(ValueError):
        DeviceCorpus.from_dataset(ref, dtype=torch.float32)
    # an *_aug set: the channel ids become the channels table
    chans = ["g711[law=a]", "amr[br=5k9]", "silk[br=15k]"]
    aug_items = [("%05d_LA_T_%07d_%s_%s_%s" % (i, 2000000 + i, tags[i + 1], labels[i + 1], c), torch.from_numpy(decoded[i + 1]))
                 for i, c in enumerate(chans)]
    aug = air_ds.ASVspoof2021LA_aug(ori_source=air_ds.PCMSource(items[:4]), aug_source=air_ds.PCMSource(aug_items),
                                    return_pcm="ragged")
    corpus = DeviceCorpus.from_dataset(aug, batch_size=5)
    assert len(corpus) == 7 and tuple(corpus.channels.shape) == (7, 1)
    assert _np(corpus.channels)[:, 0].tolist() == [0] * 4 + [air_ds.CHANNELS_LA.index(c) for c in chans]
    for i, d in enumerate(decoded[:4] + decoded[1:4]):
        assert np.array_equal(_np(corpus.row(i)), d), i
