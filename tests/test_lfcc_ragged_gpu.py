"""GPU: the ragged front-end (``air_lfcc_fwd_ragged`` through ``LFCC.forward_ragged``), the replayed ragged train step and
the ``return_pcm='ragged'`` loader.

The yardstick is the fixed-length kernel, itself pinned to the reference in tests/test_lfcc_gpu.py: row b of a ragged batch
must be, BIT FOR BIT, what ``forward_padded`` gives for that utterance alone - the per-frame arithmetic is the same
instruction sequence and the vector and scalar staging paths round identically, so a differing bit is a bug."""
import numpy as np
import pytest
import torch

from oracle import lfcc as o_lfcc
from oracle import pad as o_pad
from oracle.filler import fill_module_, synth_pcm

pytestmark = pytest.mark.gpu

TOL = 3e-5  # the bound of tests/test_lfcc_gpu.py for this kernel against the oracle
FEAT_LEN = 40
# T = 1, 2, 28 (one full tile of 28 frames), 29 (first frame of a second tile), 40 (= feat_len), 41; + the capacity itself
SHORT = [159, 160, 28 * 160 - 1, 28 * 160, 39 * 160, 40 * 160]
# T = 101 both: rows of 16037 floats are not 16-byte aligned (scalar staging), rows of 16040 are (float4 staging)
CAPS = [100 * 160 + 37, 100 * 160 + 40]
STARTS = [0, 17, 61, 1000]  # of the last row: 61 = T - feat_len, 1000 is clamped like the fixed kernel clamps it


def _lfcc(with_emphasis=True, with_delta=True):
    from asvspoof2021_air_amd.feature_extraction import LFCC
    m = LFCC(320, 160, 512, 16000, 20, with_emphasis=with_emphasis, with_delta=with_delta).cuda()
    m.mutate_input = False
    return m


def _batch(cap, dtype, tail="zero"):
    """(x on the GPU, lengths): 7 rows of capacity ``cap``; beyond its length a row is zero, or the worst value of its type."""
    lengths = SHORT + [cap]
    x = synth_pcm(len(lengths), cap, seed=900 + cap)
    if dtype == torch.int16:
        x = (x * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
    fill = 0 if tail == "zero" else (float("nan") if dtype == torch.float32 else 32767)
    for b, n in enumerate(lengths):
        x[b, n:] = fill
    return x.cuda(), lengths


def _rows_alone(m, x, lengths, start, padding, feat_len=FEAT_LEN):
    rows = []
    for b, n in enumerate(lengths):
        st = None if start is None else start[b:b + 1]
        rows.append(m.forward_padded(x[b:b + 1, :n].contiguous(), feat_len, st, padding)[0])
    return torch.stack(rows)


@pytest.mark.parametrize("with_emphasis,with_delta", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("padding", ["repeat", "zero", "silence"])
def test_ragged_rows_equal_fixed_length_rows(padding, dtype, with_emphasis, with_delta):
    m = _lfcc(with_emphasis, with_delta)
    for cap in CAPS:
        x, lengths = _batch(cap, dtype)
        keep = x.clone()
        ld = torch.tensor(lengths, dtype=torch.int32).cuda()
        for s_last in STARTS:
            start = torch.tensor([0] * len(SHORT) + [s_last], dtype=torch.int32).cuda()
            got = m.forward_ragged(x, ld, FEAT_LEN, start, padding)
            assert got.shape == (len(lengths), m.out_dim, FEAT_LEN) and got.is_contiguous()
            want = _rows_alone(m, x, lengths, start, padding)
            for b in range(len(lengths)):
                assert torch.equal(got[b], want[b]), (cap, s_last, b, lengths[b], float((got[b] - want[b]).abs().max()))
        # no start at all == zeros
        assert torch.equal(m.forward_ragged(x, ld, FEAT_LEN, None, padding), _rows_alone(m, x, lengths, None, padding))
        assert torch.equal(x, keep)


def test_ragged_vs_oracle():
    m = _lfcc()
    cap = CAPS[0]
    x, lengths = _batch(cap, torch.float32)
    start = [0] * len(SHORT) + [17]
    sil_o = torch.from_numpy(o_lfcc.lfcc_forward(np.zeros((1, 3200), np.float32)))[:, 0, :]
    feats = [torch.from_numpy(o_lfcc.lfcc_forward(x[b:b + 1, :n].cpu().numpy().copy())) for b, n in enumerate(lengths)]
    for padding in ("repeat", "zero", "silence"):
        got = m.forward_ragged(x, lengths, FEAT_LEN, torch.tensor(start, dtype=torch.int32).cuda(), padding)
        rows = []
        for b, f in enumerate(feats):
            T = f.shape[1]
            if T > FEAT_LEN:
                f = f[:, start[b]:start[b] + FEAT_LEN]
            elif T < FEAT_LEN:
                f = {"zero": lambda: o_pad.zero_pad(f, FEAT_LEN), "repeat": lambda: o_pad.repeat_pad(f, FEAT_LEN),
                     "silence": lambda: o_pad.silence_pad(f, FEAT_LEN, sil_o)}[padding]()
            rows.append(f)
        want = o_pad.to_model_input(torch.stack(rows))[:, 0]
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), atol=TOL)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "i16"])
def test_ragged_tail_is_never_read(dtype):
    """What lies behind an utterance's length (NaN / full scale) reaches no output; the input is left as it was."""
    m = _lfcc()
    for cap in CAPS:
        clean, lengths = _batch(cap, dtype)
        dirty, _ = _batch(cap, dtype, tail="worst")
        assert not torch.equal(clean.float().nan_to_num(7.0), dirty.float().nan_to_num(7.0))
        keep = dirty.clone()
        ld = torch.tensor(lengths, dtype=torch.int32).cuda()
        start = torch.tensor([0] * len(SHORT) + [17], dtype=torch.int32).cuda()
        for padding in ("repeat", "zero", "silence"):
            a = m.forward_ragged(clean, ld, FEAT_LEN, start, padding)
            b = m.forward_ragged(dirty, ld, FEAT_LEN, start, padding)
            assert bool(torch.isfinite(b).all())
            assert torch.equal(a, b)
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        assert torch.equal(dirty.view(bits), keep.view(bits))


def test_ragged_input_validation():
    from asvspoof2021_air_amd import _hip
    m = _lfcc()
    cap = CAPS[0]
    x, lengths = _batch(cap, torch.float32)
    with pytest.raises(ValueError):
        m.forward_ragged(x, [0] + lengths[1:], FEAT_LEN)
    with pytest.raises(ValueError):
        m.forward_ragged(x, torch.tensor(lengths[:-1] + [cap + 1], dtype=torch.int32), FEAT_LEN)
    with pytest.raises(ValueError):
        m.forward_ragged(x, lengths[:-1], FEAT_LEN)
    with pytest.raises(ValueError, match="Padding should be zero or repeat!"):
        m.forward_ragged(x, lengths, FEAT_LEN, None, "reflect")
    with pytest.raises(_hip.AirError):
        m.forward_ragged(x.cpu(), lengths, FEAT_LEN)
    # a device tensor is used as is: the kernel clamps it into the row (memory safety, nothing more)
    over = torch.tensor(lengths[:-1] + [cap + 5], dtype=torch.int32).cuda()
    under = torch.tensor([-3] + lengths[1:], dtype=torch.int32).cuda()
    want = m.forward_ragged(x, lengths, FEAT_LEN)
    assert torch.equal(m.forward_ragged(x, over, FEAT_LEN), want)
    one = m.forward_ragged(x, [1] + lengths[1:], FEAT_LEN)
    assert torch.equal(m.forward_ragged(x, under, FEAT_LEN), one)
    # host lists, host tensors and device tensors agree
    assert torch.equal(m.forward_ragged(x, torch.tensor(lengths), FEAT_LEN), want)
    assert torch.equal(m.forward_ragged(x, torch.tensor(lengths, dtype=torch.int32).cuda(), FEAT_LEN), want)


# ---------------------------------------------------------------------------- trainer
def _trainer(graph, feat_len=96, seed=4242):
    """The model, head and seeds of the eager-vs-replay test of tests/test_resnet_gpu.py."""
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.resnet import ResNet
    from asvspoof2021_air_amd.train import Trainer
    m = ResNet(3, 256, resnet_type="18", nclasses=2)
    fill_module_(m)
    m = m.cuda()
    m._noise_seed = seed  # device noise ON: the replay has to draw what the eager step draws
    lossm = AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)
    fill_module_(lossm)
    tr = Trainer(m, loss_module=lossm, feat_len=feat_len)
    if graph:
        tr.enable_graph(segments=False)
    else:
        m.overlap_wgrad = False  # the capture is one chain; same launches eagerly
    return m, tr


def test_ragged_replay_equals_eager_and_serves_every_batch_from_one_capture():
    B, cap = 4, 32000  # T up to 201 > feat_len 96
    lens = [[32000, 159, 20000, 15359], [4480, 32000, 16000, 31999], [25000, 12000, 32000, 300]]
    starts = [[60, 0, 11, 0], [0, 105, 3, 1], [33, 0, 7, 0]]  # non-zero on every long row (T_b > 96)
    batches = []
    for i in range(3):
        pcm = synth_pcm(B, cap, seed=500 + i)
        for b, n in enumerate(lens[i]):
            pcm[b, n:] = 0
        batches.append((pcm.cuda(), ((torch.arange(B) + i) % 3 != 0).long().cuda(),
                        torch.tensor(starts[i], dtype=torch.int32).cuda(), torch.tensor(lens[i], dtype=torch.int32).cuda()))
    ends = []
    for graph in (False, True):
        m, tr = _trainer(graph)
        losses, capture = [], None
        for i in range(6):  # two eager warm-up steps, the capture on batch 2, then every batch again on replay
            pcm, lab, st, ln = batches[i % 3]
            losses.append(tr.step(pcm, lab, start=st, lengths=ln)[0].item())
            if graph and i == 2:
                capture = tr._graph
                assert capture is not None and "ragged" in capture["key"] and capture["lengths"].dtype == torch.int32
        torch.cuda.synchronize()
        if graph:
            # one capture, one graph object, served all three sets of lengths
            assert tr._graph is capture and len(capture["graphs"]) == 1
            assert capture["lengths"].tolist() == lens[2] and capture["start"].tolist() == starts[2]
        else:
            assert tr._graph is None
        ends.append((losses, m.arena().flat.clone(), tr.loss.center.detach().clone(), m.bn1.running_var.clone(),
                     int(m._noise_ctr.item())))
    (l0, w0, c0, rv0, k0), (l1, w1, c1, rv1, k1) = ends
    assert all(np.isfinite(l0)) and l0 == l1
    assert torch.equal(w0, w1) and torch.equal(c0, c1) and torch.equal(rv0, rv1) and k0 == k1 > 0


def test_ragged_replay_without_start_uses_zeros_and_fixed_batches_keep_their_rules():
    m, tr = _trainer(True)
    pcm = synth_pcm(4, 32000, seed=77).cuda()
    lab = torch.tensor([0, 1, 1, 0]).cuda()
    ln = torch.tensor([32000, 5000, 30000, 159], dtype=torch.int32).cuda()
    st = torch.tensor([9, 0, 4, 0], dtype=torch.int32).cuda()
    for _ in range(3):
        tr.step(pcm, lab, start=st, lengths=ln)
    g = tr._graph
    assert g is not None and g["start"].tolist() == [9, 0, 4, 0]
    tr.step(pcm, lab, lengths=ln)  # a missing start refreshes the capture's buffer to zeros
    assert tr._graph is g and g["start"].tolist() == [0, 0, 0, 0]
    tr.step(pcm, lab, start=st)  # lengths None: a start still forces the eager step, the capture is left alone
    assert tr._graph is g and g["start"].tolist() == [0, 0, 0, 0]
    tr.augment = lambda x: x  # ragged rows through the IR convolution are out of scope
    for call in (lambda: tr.step(pcm, lab, lengths=ln), lambda: tr.features(pcm, lengths=ln),
                 lambda: tr.eval_batch(pcm, lab, lengths=ln), lambda: tr.score(pcm, lengths=ln)):
        with pytest.raises(NotImplementedError):
            call()
    tr.augment = None
    m.set_attention_noise(None)  # (the per-call noise off: two calls on the same features give the same scores)
    loss, score = tr.eval_batch(pcm, lab, start=st, lengths=ln)
    assert bool(torch.isfinite(loss).all()) and score.shape == (4,)
    # eval_batch and score see the features of the same ragged launch: the utterances alone, not the rows' tails
    dirty = pcm.clone()
    for b, n in enumerate(ln.tolist()):
        dirty[b, n:] = float("nan")
    assert torch.equal(tr.score(dirty, start=st, lengths=ln), tr.score(pcm, start=st, lengths=ln))
    assert torch.equal(tr.eval_batch(dirty, lab, start=st, lengths=ln)[1], score)


# ---------------------------------------------------------------------------- dataset -> trainer
def _items(lengths, seed):
    wav = synth_pcm(len(lengths), max(lengths), seed=seed)
    return [("%05d_LA_T_%07d_%s_%s" % (i, 1000000 + i, "A%02d" % (1 + i % 6) if i % 2 else "-", "spoof" if i % 2 else "bonafide"),
             wav[i, :n].clone()) for i, n in enumerate(lengths)]


MIXED = SHORT + [CAPS[0], 77 * 160 + 3, 3000, 55 * 160, 12345, CAPS[1]]  # 12 utterances, five longer than feat_len 40


@pytest.mark.parametrize("padding", ["repeat", "zero", "silence"])
def test_ragged_collate_features_equal_the_grouped_collate(padding):
    from asvspoof2021_air_amd import dataset as air_ds
    items = _items(MIXED, 31)
    ragged = air_ds.ASVspoof2019("LA", None, "train", feat_len=FEAT_LEN, padding=padding, source=air_ds.PCMSource(items),
                                 return_pcm="ragged")
    grouped = air_ds.ASVspoof2019("LA", None, "train", feat_len=FEAT_LEN, padding=padding, source=air_ds.PCMSource(items),
                                  return_pcm=True)
    np.random.seed(5)
    want = grouped.collate_fn([grouped[i] for i in range(len(items))])
    np.random.seed(5)
    pcm, lengths, start, names, tags, labels = ragged.collate_fn([ragged[i] for i in range(len(items))])
    assert pcm.is_pinned() and pcm.shape == (12, 32000) and int(torch.count_nonzero(start)) >= 3
    got = ragged.lfcc.cuda().forward_ragged(pcm.cuda(), lengths.cuda(), FEAT_LEN, start.cuda(), padding)
    assert torch.equal(got, want[0].transpose(2, 3)[:, 0])
    assert list(names) == list(want[1]) and torch.equal(tags, want[2]) and torch.equal(labels, want[3])


def test_ragged_loader_feeds_the_trainer():
    from torch.utils.data import DataLoader
    from asvspoof2021_air_amd import dataset as air_ds
    m, tr = _trainer(False)
    ds = air_ds.ASVspoof2019("LA", None, "train", feat_len=96, source=air_ds.PCMSource(_items(MIXED[4:], 32)),
                             return_pcm="ragged")
    ds.ragged_samples = CAPS[1]
    dl = DataLoader(ds, batch_size=4, shuffle=False, collate_fn=ds.collate_fn, num_workers=0)
    np.random.seed(6)
    n = 0
    for pcm, lengths, start, audio_fn, tags, labels in air_ds.DevicePrefetcher(dl, "cuda"):
        assert pcm.is_cuda and pcm.shape == (4, CAPS[1]) and lengths.is_cuda and lengths.dtype == torch.int32
        assert lengths.tolist() == MIXED[4 + 4 * n:8 + 4 * n] and start.dtype == torch.int32 and len(audio_fn) == 4
        loss, neg = tr.step(pcm, labels, start=start, lengths=lengths)
        assert np.isfinite(loss.item()) and bool(torch.isfinite(neg).all())
        n += 1
    assert n == 2


def test_score_pcm_ragged_equals_each_utterance_alone():
    from asvspoof2021_air_amd.generate_score import batch_scores, score_pcm
    m, tr = _trainer(False)
    m.set_attention_noise(None)
    lengths = [159, 40 * 160, 12345, CAPS[1]]
    pcm = synth_pcm(4, CAPS[1], seed=41)
    for b, n in enumerate(lengths):
        pcm[b, n:] = float("nan")
    pcm = pcm.cuda()
    got = score_pcm(m, tr.loss, pcm, feat_len=96, lengths=lengths, lfcc=tr.lfcc)
    assert got.shape == (4,) and bool(torch.isfinite(got).all())
    # the same model batch on features made one utterance at a time: the front-end is the only difference - bit for bit
    feat = _rows_alone(tr.lfcc, pcm, lengths, None, "repeat", 96)
    assert torch.equal(got, -batch_scores(m, feat.unsqueeze(1), tr.loss, "ocsoftmax"))
    # each utterance alone through score_pcm: a batch of 1 may sum in another order than a batch of 4 (the convolution
    # routes depend on the batch size), so this is fp32 against fp32 on a cosine score in [-1, 1] - the 1e-4 that
    # smoke() allows the same scores against the CPU evaluation of the same network
    alone = torch.cat([score_pcm(m, tr.loss, pcm[b:b + 1, :n].contiguous(), feat_len=96, lfcc=tr.lfcc) for b, n in enumerate(lengths)])
    print("score_pcm ragged vs alone: max |diff| = %.3g" % float((got - alone).abs().max()))
    np.testing.assert_allclose(got.cpu().numpy(), alone.cpu().numpy(), atol=1e-4, rtol=0)
