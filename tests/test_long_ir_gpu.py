"""GPU: banks of impulse responses of different lengths (``air_ir_bank_convolve`` through ``augment.ir_convolve(pcm,
IRBank, ...)``): room-length responses by uniformly partitioned overlap-save beside device responses on the existing route.

Yardsticks.  tests/long_ir_oracle.py (oracle/channel.py per row, float64), to the bound tests/test_augment.py holds both
existing forms to: 2e-6 of the row's output scale, times sqrt(taps) / 8 behind 64 taps.  The existing ragged call, bit for
bit, for every row whose response has at most 1025 taps.  And the call itself: on one utterance alone, on a clean batch,
and eagerly, where the statement is that rows do not see each other, what lies outside them, or a graph replay."""
import functools

import numpy as np
import pytest
import torch

from oracle.filler import synth_pcm
from long_ir_oracle import bank_oracle, row_bound

pytestmark = pytest.mark.gpu

LCAP = 9300


def _dev(v):
    return torch.tensor(v, dtype=torch.int32).cuda()


def _responses(taps, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(t) * np.exp(-np.arange(t) / max(t / 6.0, 1.0))).astype(np.float32) for t in taps]


def _bank(taps, seed=5):
    from asvspoof2021_air_amd.augment import IRBank
    return IRBank(_responses(taps, seed)).to("cuda")


def _pcm(lengths, cap, dtype=torch.float32, tail="zero", seed=9):
    """(B, cap) on the GPU; beyond its length a row is zero, or the worst value of its type."""
    x = synth_pcm(len(lengths), cap, seed=seed)
    if dtype == torch.int16:
        x = (x * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
    fill = 0 if tail == "zero" else (float("nan") if dtype == torch.float32 else 32767)
    for b, n in enumerate(lengths):
        x[b, n:] = fill
    return x.cuda()


def _check_rows(got, x, lengths, bank, idx, normalize, what):
    """Every row of ``got`` (host) against the float64 helper, to the per-row bound; prints each figure first."""
    irs, taps = bank.irs.cpu().numpy(), bank.taps.cpu().numpy()
    want = bank_oracle(x.cpu().numpy(), lengths, irs, taps, idx, normalize)
    got = got.double().numpy()
    for b, n in enumerate(lengths):
        assert not got[b, n:].any(), (what, b, n)
        if idx[b] < 0:
            assert np.array_equal(got[b, :n], want[b, :n]), (what, b)  # pass-through: bit-exact
            continue
        t = int(taps[idx[b]])
        err, bound = np.abs(got[b, :n] - want[b, :n]).max(), row_bound(want[b, :n], t)
        print("%s normalize %d row %d L %d taps %d: max |err| %.3g, bound %.3g" % (what, normalize, b, n, t, err, bound))
        assert err <= bound, (what, normalize, b, n, t, err, bound)


# ------------------------------------------------------------------------------------------------------ 1. tap-count edges
TAP_EDGES = [1, 127, 1024, 1025, 1026, 2048, 2049, 3073, 4097, 16384, 20000]


def test_tap_count_edges_vs_oracle():
    """One row per response; both sides of the short / long switch (1025) and of the partition boundaries (2048 k)."""
    from asvspoof2021_air_amd.augment import ir_convolve
    bank = _bank(TAP_EDGES)
    B = len(TAP_EDGES)
    x = _pcm([LCAP] * B, LCAP)
    idx = list(range(B))
    for normalize in (False, True):
        got = ir_convolve(x, bank, _dev(idx), normalize)
        assert got.dtype == torch.float32 and got.shape == (B, LCAP)
        _check_rows(got.cpu(), x, [LCAP] * B, bank, idx, normalize, "taps")


# -------------------------------------------------------------------------------------------------------- 2. length edges
LENGTH_EDGES = [1, 777, 2048, 2049, 3072, 3073, 4096, 4097, 6144, 6145, LCAP]


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "i16"])
def test_length_edges_vs_oracle(dtype):
    """A 5000-tap response (three partitions) on rows that end around every block and pair boundary; rows of 1 and 777
    samples are shorter than the response."""
    from asvspoof2021_air_amd.augment import ir_convolve
    bank = _bank([5000])
    x = _pcm(LENGTH_EDGES, LCAP, dtype)
    idx = [0] * len(LENGTH_EDGES)
    for normalize in (False, True):
        got = ir_convolve(x, bank, _dev(idx), normalize, lengths=_dev(LENGTH_EDGES))
        _check_rows(got.cpu(), x, LENGTH_EDGES, bank, idx, normalize, "lengths")


# ---------------------------------------------------------------------------------------------------------- 3. mixed bank
def test_room_bank_mixed_batch_vs_oracle():
    from asvspoof2021_air_amd.augment import ir_convolve, synthetic_room_bank
    bank = synthetic_room_bank().to("cuda")
    lengths, idx = [64000, 40000, 12345, 64000, 5000, 30001], [3, 27, 28, 29, -1, 27]
    x = _pcm(lengths, 64000, seed=11)
    for normalize in (False, True):
        got = ir_convolve(x, bank, _dev(idx), normalize, lengths=_dev(lengths))
        _check_rows(got.cpu(), x, lengths, bank, idx, normalize, "room bank")


# ------------------------------------------------------------------------------------------- 4. short rows are the old rows
SHORT_TAPS = [128, 700, 1024, 1025]
SHORT_LENGTHS = [LCAP, 3073, 777, 6145, 2048, 1]
SHORT_IDX = [0, 1, 2, 3, -1, 2]


def test_short_rows_carry_the_bits_of_the_existing_call():
    from asvspoof2021_air_amd.augment import IRBank, ir_convolve
    short = _responses(SHORT_TAPS, 6)
    bank = IRBank(short).to("cuda")
    assert bank.irs.shape == (4, 1025)
    x = _pcm(SHORT_LENGTHS, LCAP)
    ld = _dev(SHORT_LENGTHS)
    # the same responses in a bank that also holds a 5000-tap one, drawn by an extra row in the middle of the batch
    mixed = IRBank(short + _responses([5000], 7)).to("cuda")
    assert torch.equal(mixed.irs[:4, :1025], bank.irs)
    lengths2 = SHORT_LENGTHS[:3] + [8000] + SHORT_LENGTHS[3:]
    idx2 = SHORT_IDX[:3] + [4] + SHORT_IDX[3:]
    x2 = torch.cat([x[:3], _pcm([8000], LCAP, seed=3), x[3:]]).contiguous()
    keep = [0, 1, 2, 4, 5, 6]
    for normalize in (False, True):
        old = ir_convolve(x, bank.irs, _dev(SHORT_IDX), normalize, lengths=ld)
        new = ir_convolve(x, bank, _dev(SHORT_IDX), normalize, lengths=ld)
        assert torch.equal(new, old), (normalize, float((new - old).abs().max()))
        got2 = ir_convolve(x2, mixed, _dev(idx2), normalize, lengths=_dev(lengths2))
        assert torch.equal(got2[keep], old), (normalize, float((got2[keep] - old).abs().max()))
        assert bool(torch.isfinite(got2[3]).all()) and float(got2[3, :8000].abs().max()) > 0 and not bool(got2[3, 8000:].any())


# ---------------------------------------------------------------------------------------------- 5. nothing outside is read
@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "i16"])
def test_nothing_outside_rows_responses_and_written_workspace_is_read(dtype):
    from asvspoof2021_air_amd import ops
    from asvspoof2021_air_amd.augment import IRBank, ir_convolve
    taps = [700, 5000, 2048, 1026]
    lengths, idx = [LCAP, 777, 4097, 6145, 3000, 1], [1, 1, 2, 0, -1, 3]
    clean = IRBank(_responses(taps, 8)).to("cuda")
    dirty = clean.to("cuda")
    dirty.irs = clean.irs.clone()
    for i, t in enumerate(taps):
        dirty.irs[i, t:] = float("nan")
    assert bool(torch.isnan(dirty.irs).any())
    xc, xd = _pcm(lengths, LCAP, dtype), _pcm(lengths, LCAP, dtype, tail="worst")
    ld = _dev(lengths)
    for normalize in (False, True):
        a = ir_convolve(xc, clean, _dev(idx), normalize, lengths=ld)
        torch.cuda.synchronize()
        for buf in list(ops._WS.values()):
            buf.fill_(255)  # NaN, as floats
        b = ir_convolve(xd, dirty, _dev(idx), normalize, lengths=ld)
        assert bool(torch.isfinite(b).all())
        assert torch.equal(a, b)
        for r, n in enumerate(lengths):
            assert int(torch.count_nonzero(b[r, n:])) == 0


# -------------------------------------------------------------------------------------------------------- 6. row independence
@pytest.mark.parametrize("taps", [5000, 2048, 700])
def test_a_row_carries_the_bits_of_the_call_on_that_utterance_alone(taps):
    from asvspoof2021_air_amd.augment import ir_convolve
    bank = _bank([300, taps, 9000, 1500], seed=12)
    n = 7001
    lengths, idx = [LCAP, 3000, n, 12000], [2, 0, 1, 3]
    x = _pcm(lengths, 12000, seed=13)
    for normalize in (False, True):
        alone = ir_convolve(x[2:3, :n].contiguous(), bank, _dev([1]), normalize)
        batch = ir_convolve(x, bank, _dev(idx), normalize, lengths=_dev(lengths))
        assert torch.equal(batch[2, :n], alone[0]), (taps, normalize, float((batch[2, :n] - alone[0]).abs().max()))


# ------------------------------------------------------------------------------------------------------------------ 7. replay
def test_graph_replay_with_changed_lengths_indices_and_pcm_equals_the_eager_call():
    from asvspoof2021_air_amd.augment import ir_convolve
    bank = _bank([700, 5000, 2049, 1025], seed=14)
    sets = [([LCAP, 100, 4097, 5001], [1, 2, -1, 0], 21), ([1, LCAP, 9297, 4096], [3, -1, 1, 2], 22),
            ([6145, 2048, 3, LCAP], [-1, 1, 2, 1], 23)]
    pcms = [_pcm([LCAP] * 4, LCAP, seed=s) for _, _, s in sets]
    eager = [ir_convolve(p, bank, _dev(ix), True, lengths=_dev(ln)).cpu() for (ln, ix, _), p in zip(sets, pcms)]
    x, ld, idx, out = pcms[0].clone(), _dev(sets[0][0]), _dev(sets[0][1]), torch.empty(4, LCAP, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the stream's workspace exists before the capture
        ir_convolve(x, bank, idx, True, out=out, lengths=ld)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ir_convolve(x, bank, idx, True, out=out, lengths=ld)
    for (ln, ix, _), p, want in list(zip(sets, pcms, eager))[::-1]:
        ld.copy_(_dev(ln))
        idx.copy_(_dev(ix))
        x.copy_(p)
        out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want), (ln, ix)


# --------------------------------------------------------------------------------------------------------------- 8. front-end
def test_room_bank_augment_in_the_ragged_front_end():
    """``ChannelAugment(irs=synthetic_room_bank())`` then ``LFCC.forward_ragged``, against the helper and the LFCC oracle
    of the helper's PCM, to the tolerances of tests/test_augment.py::test_channel_augment_in_front_end."""
    from asvspoof2021_air_amd.augment import ChannelAugment, IRBank, synthetic_room_bank
    from asvspoof2021_air_amd.feature_extraction import LFCC
    from oracle import lfcc as o_lfcc, pad as o_pad
    aug = ChannelAugment(irs=synthetic_room_bank(), p=0.5, seed=1)
    assert isinstance(aug.irs, IRBank) and aug.irs.irs.is_cuda and aug.irs.taps.is_cuda
    lengths = [16000, 12000, 9000, 16000, 15999, 8000, 16000, 10240]
    idx = aug.draw(8)
    idx[0], idx[1], idx[2] = 27, 28, 29  # every room response is drawn
    assert (idx < 0).any() and (idx[3:] >= 0).any() and idx.max() < 30
    x = _pcm(lengths, 16000, seed=2)
    ld = _dev(lengths)
    y = aug(x, idx, lengths=ld)
    want = bank_oracle(x.cpu().numpy(), lengths, aug.irs.irs.cpu().numpy(), aug.irs.taps.cpu().numpy(), idx, True)
    print("front-end: max |pcm err| %.3g" % np.abs(y.cpu().numpy() - want).max())
    np.testing.assert_allclose(y.cpu().numpy(), want, atol=2e-6)
    feat_len = 40  # <= every row's frame count: no padding
    lf = LFCC(320, 160, 512, 16000, 20, with_energy=False).cuda()
    got = lf.forward_ragged(y, ld, feat_len)
    rows = [torch.from_numpy(o_lfcc.lfcc_forward(want[b:b + 1, :n].astype(np.float32)))[:, :feat_len]
            for b, n in enumerate(lengths)]
    ref = o_pad.to_model_input(torch.stack(rows))[:, 0]
    print("front-end: max |feature err| %.3g" % float((got.cpu() - ref).abs().max()))
    np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), atol=2e-3)  # log10 of near-empty bins amplifies the PCM difference
