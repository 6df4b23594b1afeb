"""CPU: the device corpus's permutation rule (tests/corpus_oracle.py) and the host half of corpus.py - the batch
schedule and the capacity checks - which run without a GPU."""
import itertools

import numpy as np
import pytest

import corpus_oracle as co

SEED = 688


@pytest.mark.parametrize("n", [1, 2, 3, 257, 25380])
def test_permutation_is_a_bijection(n):
    for lo in (0, 1000):
        p = co.permutation(lo, n, SEED, 3, 0)
        assert p.dtype == np.int64 and np.array_equal(np.sort(p), np.arange(lo, lo + n))
    assert np.array_equal(co.permutation(0, n, SEED, 3, 0), co.permutation(0, n, SEED, 3, 0))
    if n >= 257:  # (shorter ones coincide by chance: 1 / n!)
        base = co.permutation(0, n, SEED, 3, 0)
        assert not np.array_equal(base, co.permutation(0, n, SEED, 4, 0))      # another generation
        assert not np.array_equal(base, co.permutation(0, n, SEED, 3, 1))      # the other flow
        assert not np.array_equal(base, co.permutation(0, n, SEED + 1, 3, 0))  # another seed


def test_every_order_of_four_occurs():
    seen = set(tuple(co.permutation(0, 4, SEED, g, 0)) for g in range(2000))
    assert seen == set(itertools.permutations(range(4)))


def test_stream_numbering_and_keys():
    assert [co.stream_id(0, 0), co.stream_id(0, 1), co.stream_id(0, 2), co.stream_id(5, 1)] == [0, 1, 2, 21]
    k = co.keys(100, SEED, co.stream_id(2, 1))
    assert k.dtype == np.uint64 and np.array_equal(k & np.uint64(0xFFFFFFFF), np.arange(100, dtype=np.uint64))
    assert np.array_equal((k >> np.uint64(32)).astype(np.uint32), co.words(np.arange(100), SEED, 9))
    assert int(k.max()) < 0xFFFFFFFFFFFFFFFF  # below the sort's sentinel


def test_crop_rule():
    hop, feat_len = 160, 10
    lens = np.array([1, 159, 160, 9 * 160 + 159, 10 * 160, 10 * 160 + 159, 11 * 160, 50 * 160 + 7, 208000])
    idx = np.arange(len(lens)) + 40
    s = co.crop_start(idx, lens, SEED, 1, feat_len, hop)
    T = 1 + lens // hop
    assert s.dtype == np.int32
    assert np.all(s[T <= feat_len + 1] == 0)  # T == feat_len + 1: randint(1) draws 0 only
    assert np.all((s >= 0) & (s < np.maximum(T - feat_len, 1)))
    big = co.crop_start(np.arange(4000), np.full(4000, 208000), SEED, 0, feat_len, hop)
    assert big.min() >= 0 and big.max() < 1301 - feat_len and big.max() > 1200 and len(set(big.tolist())) > 1000
    assert not np.array_equal(big, co.crop_start(np.arange(4000), np.full(4000, 208000), SEED, 1, feat_len, hop))


# ------------------------------------------------------------------------------------ corpus.Schedule (host code)
def _run(sched, n_epochs):
    out = []
    for _ in range(n_epochs):
        sched.begin_epoch()
        epoch = []
        while True:
            segs = sched.next_step()
            if segs is None:
                break
            epoch.append(segs)
        out.append(epoch)
    return out


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("n,B", [(100, 8), (64, 8), (7, 8), (25380, 64)])
def test_single_flow_schedule(n, B, world):
    from asvspoof2021_air_amd.corpus import Schedule
    per_rank = []
    for rank in range(world):
        s = Schedule([(5, 5 + n)], B, rank=rank, world=world)
        assert len(s) == n // (B * world)
        got = _run(s, 2)
        assert got == co.schedule([(5, 5 + n)], B, 2, world=world, rank=rank)
        per_rank.append(got)
    for e in range(2):
        perm = co.permutation(5, n, SEED, e, 0)
        taken = [np.concatenate([perm[f:f + c] for segs in per_rank[r][e] for _, _, f, c in segs] or [perm[:0]])
                 for r in range(world)]
        rows = np.concatenate(taken)
        # each index at most once, exactly len * b0 * world of them, the ranks disjoint
        assert len(rows) == len(set(rows.tolist())) == (n // (B * world)) * B * world
        # together the rows of the world = 1 schedule over the same permutation, step by step
        one = _run(Schedule([(5, 5 + n)], B * world), e + 1)[e]
        assert len(one) == len(per_rank[0][e])
        for s_i, segs in enumerate(one):
            _, g, f, c = segs[0]
            union = np.concatenate([perm[pf:pf + pc] for r in range(world) for _, _, pf, pc in per_rank[r][e][s_i]])
            assert g == e and np.array_equal(union, perm[f:f + c])


@pytest.mark.parametrize("world", [1, 2])
def test_two_flows_regenerate_exactly_when_short(world):
    from asvspoof2021_air_amd.corpus import Schedule
    ranges, B, ratio = [(0, 20), (20, 33)], 8, 0.5
    b1 = B - int(B * ratio)
    runs = [_run(Schedule(ranges, B, ratio=ratio, rank=r, world=world), 6) for r in range(world)]
    for r in range(world):
        assert runs[r] == co.schedule(ranges, B, 6, ratio=ratio, world=world, rank=r)
    remaining, gen, wraps = 13, 0, 0
    for e, epoch in enumerate(runs[0]):
        assert len(epoch) == 20 // (4 * world)
        for segs in epoch:
            (f0, g0, first0, c0), (f1, g1, first1, c1) = segs
            assert (f0, g0, c0, f1, c1) == (0, e, 4, 1, b1)
            if remaining < world * b1:  # fewer rows remain than a step needs: exactly then a new generation
                gen, remaining, wraps = gen + 1, 13, wraps + 1
            assert g1 == gen and first1 == 13 - remaining
            remaining -= world * b1
    assert wraps >= 2
    for r in range(1, world):  # the ranks' rows of the second flow are disjoint neighbours
        for ea, eb in zip(runs[0], runs[r]):
            for sa, sb in zip(ea, eb):
                assert sb[1][1] == sa[1][1] and sb[1][2] == sa[1][2] + r * b1


def test_unshuffled_keeps_the_short_batch():
    from asvspoof2021_air_amd.corpus import Schedule
    s = Schedule([(3, 30)], 8, shuffle=False)
    assert len(s) == 4
    got = _run(s, 1)[0]
    assert [(f, c) for segs in got for _, _, f, c in segs] == [(0, 8), (8, 8), (16, 8), (24, 3)]
    assert got == co.schedule([(3, 30)], 8, 1, shuffle=False)[0]
    assert len(Schedule([(3, 30)], 8, shuffle=False, drop_last=True)) == 3
    assert len(Schedule([(3, 30)], 8, drop_last=False)) == 4


def test_state_dict_round_trips_mid_epoch():
    from asvspoof2021_air_amd.corpus import Schedule
    ranges, B, ratio = [(0, 20), (20, 33)], 8, 0.5
    whole = [segs for epoch in _run(Schedule(ranges, B, ratio=ratio), 4) for segs in epoch]
    a = Schedule(ranges, B, ratio=ratio)
    head = []
    for _ in range(2):
        a.begin_epoch()
        head += [a.next_step() for _ in range(len(a))]
    a.begin_epoch()
    head.append(a.next_step())  # one step into the third epoch
    state = a.state_dict()
    assert set(state) == {"epochs", "step", "generation", "cursor"}
    assert all(isinstance(v, int) or all(isinstance(x, int) for x in v) for v in state.values())
    b = Schedule(ranges, B, ratio=ratio)
    b.load_state_dict(dict(state))
    tail = []
    while True:
        segs = b.next_step()
        if segs is None:
            break
        tail.append(segs)
    tail += _run(b, 1)[0]
    assert head + tail == whole
    with pytest.raises(ValueError):
        Schedule([(0, 20)], B).load_state_dict(state)


def test_refusals():
    from asvspoof2021_air_amd.corpus import MAX_PERMUTATION, Schedule, resolve_lcap
    lengths = np.array([100, 64000, 64001, 5])
    assert resolve_lcap(None, lengths, [(0, 2)]) == 64000
    assert resolve_lcap(None, lengths, [(0, 4)]) == 80000
    assert resolve_lcap(64008, lengths, [(0, 4)]) == 64008
    assert resolve_lcap(104, lengths, [(0, 1), (3, 4)]) == 104
    with pytest.raises(ValueError):
        resolve_lcap(64004, lengths, [(0, 4)])   # not a multiple of 8
    with pytest.raises(ValueError):
        resolve_lcap(64000, lengths, [(0, 4)])   # shorter than an utterance
    with pytest.raises(ValueError):
        resolve_lcap(96, lengths, [(0, 1), (3, 4)])
    assert MAX_PERMUTATION == 1 << 20
    Schedule([(0, MAX_PERMUTATION)], 64)
    with pytest.raises(ValueError):
        Schedule([(0, MAX_PERMUTATION + 1)], 64)
    Schedule([(0, MAX_PERMUTATION + 1)], 64, shuffle=False)  # nothing is permuted
    for bad in (dict(ranges=[(0, 20), (20, 33)]), dict(ranges=[(0, 20), (20, 33)], ratio=0.01),
                dict(ranges=[(0, 20), (20, 22)], ratio=0.5), dict(ranges=[(0, 20)], ratio=0.5),
                dict(ranges=[(4, 4)]), dict(ranges=[(0, 20)], rank=2, world=2),
                dict(ranges=[(0, 20), (20, 33)], ratio=0.5, shuffle=False)):
        with pytest.raises(ValueError):
            Schedule(bad.pop("ranges"), 8, **bad)
