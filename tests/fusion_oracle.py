"""The arithmetic of score fusion restated in numpy (no pandas): what the reference's score_fusion.py gets from
``pd.concat(frames).groupby(...)['score'].sum()`` / ``.mean()`` on float32 columns, pinned bit for bit to
tests/golden/fusion.npz by tests/test_score_fusion_cpu.py, and what csrc/score_fusion.hip is held to.

Per trial, over the systems k = 0 .. K-1 in that order (the order of the concatenation), skipping the systems that do
not have the trial:

    v = fl(score_k * weight_k)          only with weights: ONE float32 product, rounded before it is accumulated
    skip v if it is NaN                  (not summed, not counted)
    y = fl(v - c);  t = fl(s + y);  c = fl(fl(t - s) - y);  c = 0 if c is NaN;  s = t        (s = c = 0 at the start)

sum = s; mean = fl(s / float32(count)); a trial without any counted term is NaN with count 0.  ``fl`` is rounding to
float32: every array below is float32, so numpy rounds each operation once."""
import numpy as np


def fuse(scores, index=None, weights=None, mode="sum"):
    """scores: (K, L) float32.  index: None (trial n is column n) or (K, N) integers, the position of trial n in row k,
    negative = absent.  weights: None or K float32.  Returns (fused (N,) float32, counts (N,) uint32)."""
    scores = np.asarray(scores)
    assert scores.dtype == np.float32 and scores.ndim == 2 and mode in ("sum", "mean")
    K, L = scores.shape
    N = L if index is None else np.asarray(index).shape[1]
    s = np.zeros(N, dtype=np.float32)
    c = np.zeros(N, dtype=np.float32)
    count = np.zeros(N, dtype=np.uint32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(K):
            if index is None:
                present = np.ones(N, dtype=bool)
                v = scores[k].copy()
            else:
                pos = np.asarray(index)[k].astype(np.int64)
                present = (pos >= 0) & (pos < L)
                v = scores[k][np.where(present, pos, 0)] if L else np.zeros(N, dtype=np.float32)
            if weights is not None:
                v = v * np.float32(weights[k])
            assert v.dtype == np.float32
            use = present & ~np.isnan(v)
            y = v - c
            t = s + y
            cn = (t - s) - y
            cn[np.isnan(cn)] = np.float32(0.0)
            s = np.where(use, t, s)
            c = np.where(use, cn, c)
            count += use
        out = s / count.astype(np.float32) if mode == "mean" else s.copy()
    out[count == 0] = np.float32(np.nan)
    assert out.dtype == np.float32
    return out, count


# ------------------------------------------------------------------ the fixture (tests/golden/fusion.npz)
def fixture_inputs(g, folder):
    """Write the fixture's three input files into ``folder``; their paths in fusion order."""
    import os
    paths = []
    for name in g["names"].tolist():
        paths.append(os.path.join(str(folder), name))
        with open(paths[-1], "wb") as fh:
            fh.write(g["input_" + name[:4]].tobytes())
    return paths


def fixture_rows(g, method):
    """The reference's returned frame: [(fname, sysid, key)] in its order and the float32 scores' raw bits."""
    rows = list(zip(g[method + "_fname"].tolist(), g[method + "_sysid"].tolist(), g[method + "_key"].tolist()))
    return rows, g[method + "_bits"]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same_bits(got, want_bits):
    """Bit equality of float32 results with recorded bits, any NaN equal to any NaN."""
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(want_bits, dtype=np.uint32).view(np.float32)
    return got.shape == want.shape and bool(np.all((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))
