"""Test infrastructure (numpy only): the device corpus's random words, permutation, crop rule, gather and batch schedule
(include/air_hip.h, "device corpus"), restated plainly over tests/philox_oracle.py.

    word(i, s)      word 0 of the Philox4x32-10 block at counter {i, s, 0, 0}, key {seed lo, seed hi}
    s               (generation << 2) | kind; kind 0 / 1: the permutation of the first / second flow, 2: the crops
    permutation     lo + (np.sort((word(i, s) << 32) | i) & 0xffffffff)
    crop            T = 1 + len // hop; 0 when T <= feat_len, else (word(index, s_crop) * (T - feat_len)) >> 32
"""
import numpy as np

import philox_oracle as po

KIND_CROP = 2
ALIGN = 8


def stream_id(generation, kind):
    return (int(generation) << 2) | int(kind)


def words(idx, seed, stream):
    """word(i, stream) for every i of ``idx``: (n,) uint32."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return po.philox4x32_10_full(np.asarray(idx, dtype=np.uint64), stream, 0, 0, seed & po.MASK32, seed >> 32)[:, 0]


def keys(n, seed, stream):
    i = np.arange(n, dtype=np.uint64)
    return (words(i, seed, stream).astype(np.uint64) << np.uint64(32)) | i


def permutation(lo, n, seed, generation, flow):
    """The permutation of [lo, lo + n) of (seed, generation, flow): (n,) int64."""
    k = np.sort(keys(n, seed, stream_id(generation, flow)))
    return int(lo) + (k & np.uint64(po.MASK32)).astype(np.int64)


def crop_start(index, lengths, seed, generation, feat_len, hop=160):
    """start of the utterances ``index`` (their corpus indices) of ``lengths`` samples: (n,) int32."""
    index = np.atleast_1d(np.asarray(index, dtype=np.int64))
    T = 1 + np.atleast_1d(np.asarray(lengths, dtype=np.int64)) // int(hop)
    w = words(index, seed, stream_id(generation, KIND_CROP)).astype(np.uint64)
    span = np.maximum(T - int(feat_len), 0).astype(np.uint64)
    return np.where(T > feat_len, (w * span) >> np.uint64(32), 0).astype(np.int32)


def store_offsets(lengths):
    """Element offsets of a store that holds utterances of ``lengths`` back to back, each at a multiple of 8: (N + 1,)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    return np.concatenate([[0], np.cumsum((lengths + ALIGN - 1) // ALIGN * ALIGN)])


def gather(rows, utterances, labels, tags, channels, Lcap, seed, generations, feat_len, hop=160):
    """One batch: ``rows`` the corpus indices drawn, ``generations`` their crop generation (one per row), ``utterances``
    the corpus as a list of 1-d arrays.  -> dict of pcm (B, Lcap), labels, start, lengths, tags, channels, index."""
    rows = np.asarray(rows, dtype=np.int64)
    pcm = np.zeros((len(rows), Lcap), dtype=utterances[0].dtype)
    lens = np.array([len(utterances[u]) for u in rows], dtype=np.int32)
    for b, u in enumerate(rows):
        pcm[b, :lens[b]] = utterances[u]
    start = np.array([crop_start(u, n, seed, g, feat_len, hop)[0] for u, n, g in zip(rows, lens, generations)], dtype=np.int32)
    return {"pcm": pcm, "labels": np.asarray(labels, dtype=np.int64)[rows], "start": start, "lengths": lens,
            "tags": np.asarray(tags, dtype=np.int64)[rows],
            "channels": None if channels is None else np.asarray(channels, dtype=np.int64)[rows], "index": rows}


def schedule(ranges, batch_size, n_epochs, ratio=None, world=1, rank=0, shuffle=True, drop_last=None):
    """The segments of every step of ``n_epochs`` epochs for one rank: a list (epochs) of lists (steps) of lists of
    ``(flow, generation, first, count)``: rows [first, first + count) of the flow's permutation of that generation
    (``shuffle=False``: of the range itself)."""
    drop_last = shuffle if drop_last is None else drop_last
    sizes = [hi - lo for lo, hi in ranges]
    rows = [batch_size]
    if len(ranges) == 2:
        rows = [int(batch_size * ratio), batch_size - int(batch_size * ratio)]
    per = world * rows[0]
    steps = sizes[0] // per if drop_last else -(-sizes[0] // per)
    gen1 = cur1 = 0
    out = []
    for e in range(n_epochs):
        epoch = []
        for s in range(steps):
            first = (s * world + rank) * rows[0]
            segs = [(0, e, first, max(0, min(rows[0], sizes[0] - first)))]
            if len(ranges) == 2:
                if sizes[1] - cur1 < world * rows[1]:  # fewer rows remain than a step needs: a new permutation
                    gen1, cur1 = gen1 + 1, 0
                segs.append((1, gen1, cur1 + rank * rows[1], rows[1]))
                cur1 += world * rows[1]
            epoch.append(segs)
        out.append(epoch)
    return out


def step_rows(segs, ranges, seed, shuffle=True, cache=None):
    """(corpus indices, crop generations) of one step's segments."""
    rows, gens = [], []
    for flow, generation, first, count in segs:
        lo, hi = ranges[flow]
        if shuffle:
            key = (flow, generation)
            if cache is None or key not in cache:
                perm = permutation(lo, hi - lo, seed, generation, flow)
                if cache is not None:
                    cache[key] = perm
            else:
                perm = cache[key]
        else:
            perm = np.arange(lo, hi, dtype=np.int64)
        rows.append(perm[first:first + count])
        gens += [generation] * count
    return np.concatenate(rows), gens
