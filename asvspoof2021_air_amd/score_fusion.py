"""Fusion of the score files of several systems: the reference's score_fusion.py without pandas, and the same fusion on
the GPU in front of the device EER / min t-DCF chain.

The reference (score_fusion.py:13-120) reads K files ``fname sysid key score``, concatenates them, groups by
``(fname, sysid, key)`` and takes per group the SUM (``-m avg``: ``avg_fuse`` is a sum, not a mean) or, after each
file's scores were multiplied by its weight, the MEAN over the files that have the trial (``-m wght``); writes
``<output>avg_fuse_score`` (both methods write that name) and prints the lower EER of the two score polarities.
Everything below reproduces it bit for bit and byte for byte (tests/golden/fusion.npz), quirks included:

  - the join is an OUTER join: a trial missing from a file is fused from the others; a trial whose key or sysid differs
    between the files stays as separate rows; the rows come out sorted by (fname, sysid, key);
  - the float32 column is summed as pandas sums it: a compensated (Kahan) float32 accumulation in file order, NaN
    scores skipped and not counted (``_fuse_rows``; tests/fusion_oracle.py restates it, csrc/score_fusion.hip runs it);
  - the weight is applied as one float32 product before the accumulation (a float32 column times a Python float);
  - ``cal_weight`` returns the raw EERs when they are all equal (K = 1 included), replaces a zero weight by 1e-5,
    and normalises ``1 - entropy term`` to sum 1;
  - the output prints each float32 with its shortest representation (``-2.9228995``), a NaN as the empty string.

Beyond the reference: ``read_file`` also takes the three-column layout ``fname score key`` that the reference's own
shipped score files and generate_score.test_on_dataset write (sysid becomes ``-``); cal_weight's hard-coded path is an
argument (``cal_weight_from_file``); a trial listed twice in ONE file is refused (pandas would add both).

``fuse_device``: K score vectors that are already on the GPU (an ensemble pass, generate_score.test_on_dataset_ensemble)
are fused by ops.score_fuse and evaluated by eval_metrics.DeviceGroupedMinima without leaving the stream."""
import math
import os

import numpy as np

from . import eval_metrics as em

MERGE_COLS = ("fname", "sysid", "key")
OUTPUT_NAME = "avg_fuse_score"  # (score_fusion.py:25, :40: both methods)
LABELS = {"bonafide": 0, "spoof": 1}


class ScoreFrame:
    """The columns of a score file: ``fname``, ``sysid``, ``key`` (lists of str) and ``score`` (float32 array)."""

    def __init__(self, fname, sysid, key, score):
        self.fname, self.sysid, self.key = list(fname), list(sysid), list(key)
        self.score = np.asarray(score, dtype=np.float32)
        if not (len(self.fname) == len(self.sysid) == len(self.key) == self.score.size) or self.score.ndim != 1:
            raise ValueError("the columns of a score frame must be of one length")

    def __len__(self):
        return len(self.fname)

    def rows(self):
        """[(fname, sysid, key)] in the frame's order."""
        return list(zip(self.fname, self.sysid, self.key))


def read_file(fname):
    """score_fusion.py:13-18 for ``fname sysid key score`` lines, and ``fname score key`` lines (sysid ``-``) as well.
    The score is parsed as Python parses it and rounded to float32.  Blank lines are skipped; anything else raises a
    ValueError that names the file and the line."""
    cols = ([], [], [], [])
    with open(fname) as fh:
        for lineno, line in enumerate(fh, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) == 4:
                name, sysid, key, score = parts
            elif len(parts) == 3:
                (name, score, key), sysid = parts, "-"
            else:
                raise ValueError("%s:%d: expected 'fname sysid key score' or 'fname score key', got %d columns" % (
                    fname, lineno, len(parts)))
            try:
                score = float(score)
            except ValueError:
                raise ValueError("%s:%d: the score %r is not a number" % (fname, lineno, score)) from None
            for c, v in zip(cols, (name, sysid, key, score)):
                c.append(v)
    with np.errstate(over="ignore"):
        return ScoreFrame(cols[0], cols[1], cols[2], np.asarray(cols[3], dtype=np.float64).astype(np.float32))


def cal_weight(eers):
    """score_fusion.py:58-89 for a list of EERs, one per input.  All equal (K = 1 included: the reference never reaches
    its ``1 / log(1)``): the EERs themselves, unnormalised.  Otherwise w = (max - e) / (max - min) with 0 replaced by
    1e-5, then 1 - (-k p log p) with p = w / sum(w), k = 1 / log(K), normalised to sum 1.  ValueError for an empty list
    or a NaN."""
    weight = [float(e) for e in eers]
    if not weight:
        raise ValueError("cal_weight needs at least one EER")
    if any(math.isnan(w) for w in weight):
        raise ValueError("cal_weight: an EER is NaN: %r" % (weight,))
    max_w, min_w = max(weight), min(weight)
    if max_w == min_w:
        return weight
    for i in range(len(weight)):
        weight[i] = (max_w - weight[i]) / (max_w - min_w)
        if weight[i] == 0:
            weight[i] = 0.00001
    k = 1.0 / math.log(len(weight))
    for i in range(len(weight)):  # (sum(weight) changes as the loop overwrites the entries, as in the reference)
        if weight[i] == 0:
            lnfi = 0.0
        else:
            p = weight[i] / sum(weight)
            lnfi = math.log(p) * p * (-k)
        weight[i] = 1 - lnfi
    sum_w = sum(weight)
    return [w / sum_w for w in weight]


def cal_weight_from_file(inputs, eer_file):
    """score_fusion.py:45-58 with the path as an argument: ``eer_file`` holds ``feature eer`` lines; for each input, in
    order, every line whose feature name is a substring of the input's path contributes its EER."""
    with open(eer_file) as fh:
        table = [ln.split()[:2] for ln in fh if ln.split()]
    eers = [float(eer) for path in inputs for feat, eer in table if feat in path]
    return cal_weight(eers)


def align(frames):
    """The outer join of K frames on (fname, sysid, key), rows sorted by that key as the reference's groupby leaves them.
    Returns (matrix, index, keys, labels): ``matrix`` (K, N) float32, the score of trial n in system k (0 where absent);
    ``index`` (K, N) int32, the row of trial n in frame k or -1 where frame k does not have it; ``keys`` the N
    (fname, sysid, key) rows; ``labels`` (N,) int64, bonafide = 0, spoof = 1, any other key -1."""
    frames = list(frames)
    if not frames:
        raise ValueError("align needs at least one frame")
    tables = []
    for k, f in enumerate(frames):
        rows = f.rows()
        table = dict(zip(rows, range(len(rows))))
        if len(table) != len(rows):
            seen = set()
            dup = next(r for r in rows if r in seen or seen.add(r))
            raise ValueError("input %d lists %r twice" % (k, dup))
        tables.append(table)
    keys = sorted(set().union(*tables))
    K, N = len(frames), len(keys)
    index = np.full((K, N), -1, dtype=np.int32)
    matrix = np.zeros((K, N), dtype=np.float32)
    for k, (f, table) in enumerate(zip(frames, tables)):
        index[k] = [table.get(r, -1) for r in keys]
        have = index[k] >= 0
        matrix[k, have] = f.score[index[k, have]]
    labels = np.array([LABELS.get(r[2], -1) for r in keys], dtype=np.int64)
    return matrix, index, keys, labels


def _fuse_rows(matrix, present, weights=None, mean=False):
    """pandas' group sum / group mean of a float32 column, per column of ``matrix`` over the rows where ``present``:
    a compensated float32 accumulation in row order, NaN skipped and not counted (module docstring)."""
    K, N = matrix.shape
    s, c = np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.float32)
    count = np.zeros(N, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(K):
            v = matrix[k] if weights is None else matrix[k] * np.float32(weights[k])
            use = present[k] & ~np.isnan(v)
            y = v - c
            t = s + y
            comp = (t - s) - y
            comp[np.isnan(comp)] = 0.0
            s, c = np.where(use, t, s), np.where(use, comp, c)
            count += use
        out = s / count if mean else s
    out = out.astype(np.float32)
    out[count == 0] = np.nan
    return out


def write_fused(path, keys, scores):
    """The text of ``result_df.to_csv(path, sep=' ', header=False, index=False)``: ``fname sysid key score`` with the
    shortest representation of the float32 score; a NaN prints as nothing."""
    scores = np.asarray(scores, dtype=np.float32)
    text = scores.astype(str)
    text[np.isnan(scores)] = ""
    with open(path, "w") as fh:
        fh.write("".join("%s %s %s %s\n" % (r[0], r[1], r[2], t) for r, t in zip(keys, text)))


def _frames(inputs):
    return [f if isinstance(f, ScoreFrame) else read_file(f) for f in inputs]


def _finish(keys, scores, output):
    if output is not None:
        if os.path.dirname(output):
            os.makedirs(os.path.dirname(output), exist_ok=True)
        write_fused(output + OUTPUT_NAME, keys, scores)
    return ScoreFrame([r[0] for r in keys], [r[1] for r in keys], [r[2] for r in keys], scores)


def avg_fuse(inputs, output=None):
    """score_fusion.py:21-28: per (fname, sysid, key) the SUM of the scores of the inputs (paths or ScoreFrames) that
    have it.  With ``output`` the file ``output + 'avg_fuse_score'`` is written.  Returns the fused ScoreFrame."""
    matrix, index, keys, _ = align(_frames(inputs))
    return _finish(keys, _fuse_rows(matrix, index >= 0), output)


def weighted_fuse(inputs, eers, output=None):
    """score_fusion.py:31-43: every input's scores times its weight ``cal_weight(eers)[k]``, then per key the MEAN over
    the inputs that have it.  Writes the same file name as avg_fuse."""
    frames = _frames(inputs)
    weights = cal_weight(eers)
    if len(weights) != len(frames):
        raise ValueError("%d EERs for %d inputs" % (len(weights), len(frames)))
    matrix, index, keys, _ = align(frames)
    return _finish(keys, _fuse_rows(matrix, index >= 0, weights, mean=True), output)


def fused_eer(keys, scores):
    """What the reference's main block prints (score_fusion.py:111-120): the lower EER of the two score polarities over
    the bonafide / spoof rows.  ``keys``: the (fname, sysid, key) rows or the key column."""
    labels = np.array([LABELS.get(k if isinstance(k, str) else k[2], -1) for k in keys], dtype=np.int64)
    return em.eer_both_polarities(np.asarray(scores, dtype=np.float32).astype(np.float64), labels)


# ------------------------------------------------------------------ on the device
class FusionResult:
    """fuse_device's result: ``scores`` the fused (N,) device tensor, ``weights`` the weights used (None for "avg"),
    ``system_eers`` per system the pair (EER, EER of the negated scores), ``eer`` the lower of the fused scores' two,
    ``eers`` that pair, ``min_tdcf`` (None without ``tdcf``) of the polarity with the lower EER, ``by_group`` (None
    without ``n_groups``) per group a dict(eers, eer, min_tdcf) or None where the group lacks a class."""

    def __init__(self, scores, weights, system_eers, eers, min_tdcf=None, by_group=None):
        self.scores, self.weights, self.system_eers = scores, weights, system_eers
        self.eers, self.eer, self.min_tdcf, self.by_group = eers, min(eers), min_tdcf, by_group


def fuse_device(scores, labels, method="avg", eers=None, index=None, tdcf=None, groups=None, n_groups=None):
    """avg_fuse (``method="avg"``) / weighted_fuse (``"wght"``) of K systems' scores that live on the GPU, and the
    figures of the fused scores from the device metric chain.

    ``scores``: fp32 (K, L) GPU tensor.  ``index`` None: trial n is column n of every row (N = L).  ``index`` (K, N)
    integers on the HOST (what ``align`` returns): the position of trial n in row k, -1 = system k lacks it; every row k
    must then be exactly its own trials (positions 0 .. count - 1 used once) so that a system's EER is taken over its
    L_k = count leading scores.  ``labels`` (N,) integers on the GPU, 0 = bona fide, anything else = spoof;
    ``groups`` / ``n_groups`` and ``tdcf = (Pfa_asv, Pmiss_asv, Pmiss_spoof_asv, cost_model[, rates per group])`` as
    train.Trainer.evaluate takes them, for the FUSED scores.

    ``"avg"``, or ``"wght"`` with ``eers``: the kernel fuses, the chain writes the K systems' records and the fused
    records into one packed buffer, and ONE device-to-host copy fetches them.  ``"wght"`` with ``eers=None``: the weights
    come from the systems' own EERs, which have to reach the host first - one copy for the K systems' records, then the
    fusion and a SECOND copy for the fused records.  The reference takes "the figure in the file" for a system's EER;
    here it is the lower of the system's two polarities.  The weights reach the kernel as device data.

    Every EER equals eval_metrics' host functions on the same scores bit for bit (the chain guarantees it or raises).
    Up to 2^20 trials (ValueError beyond); CPU tensors raise AirError; a trial that no system has raises ValueError
    before anything is evaluated (its fused score is NaN, which the chain refuses)."""
    import torch
    from . import _hip, ops
    from .eval_metrics import DeviceCurveMinima, DeviceGroupedMinima, _rates_of_group, tdcf_weights
    if method not in ("avg", "wght"):
        raise ValueError("method must be 'avg' or 'wght', got %r" % (method,))
    if not (torch.is_tensor(scores) and scores.is_cuda and torch.is_tensor(labels) and labels.is_cuda) or (
            groups is not None and not (torch.is_tensor(groups) and groups.is_cuda)):
        raise _hip.AirError("fuse_device takes GPU tensors (avg_fuse / weighted_fuse are the host path)")
    if scores.dim() != 2 or scores.dtype != torch.float32:
        raise ValueError("scores must be fp32 of shape (K, L), got %s %s" % (scores.dtype, tuple(scores.shape)))
    K, L = scores.shape
    N = L
    rows = [(scores[k], labels) for k in range(K)]
    dev_index = None
    if index is not None:
        if torch.is_tensor(index) and index.is_cuda:
            raise ValueError("index must be a host array (align's): its absent trials are checked without a synchronisation")
        index = np.asarray(index)
        if index.ndim != 2 or index.shape[0] != K or not np.issubdtype(index.dtype, np.integer):
            raise ValueError("index must be (%d, N) integers" % K)
        N = index.shape[1]
        lost = int(np.count_nonzero(~(index >= 0).any(axis=0)))
        if lost:
            raise ValueError("%d trials are absent from every system" % lost)
        rows = []
        for k in range(K):
            have = np.flatnonzero(index[k] >= 0)
            trial_at = np.empty(have.size, dtype=np.int64)
            pos = index[k, have].astype(np.int64)
            if have.size > L or not np.array_equal(np.sort(pos), np.arange(have.size)):
                raise ValueError("row %d must hold exactly its %d trials at positions 0 .. %d" % (k, have.size, have.size - 1))
            trial_at[pos] = have
            rows.append((scores[k, :have.size], labels.reshape(-1).index_select(0, torch.from_numpy(trial_at).to(labels.device))))
        dev_index = torch.from_numpy(np.ascontiguousarray(index, dtype=np.int32)).to(scores.device)
    if labels.numel() != N:
        raise ValueError("%d labels for %d trials" % (labels.numel(), N))
    if N < 1 or N > ops.EVAL_MAX_TRIALS:
        raise ValueError("fuse_device takes 1 .. %d trials, got %d" % (ops.EVAL_MAX_TRIALS, N))
    if K > ops.score_fuse_max_systems():
        raise ValueError("score fusion takes 1 .. %d systems, got %d" % (ops.score_fuse_max_systems(), K))
    if eers is not None and (method != "wght" or len(eers) != K):
        raise ValueError("eers: %d EERs for method 'wght', one per system" % K)
    grouped = n_groups is not None
    if grouped != (groups is not None):
        raise ValueError("groups and n_groups go together")
    weights = tdcf_weights(*tdcf[:4]) if tdcf is not None else None
    if not grouped and tdcf is not None and len(tdcf) > 4:
        raise ValueError("per-group t-DCF rates need n_groups")
    if grouped:
        n_groups = int(n_groups)
        if weights is not None:
            rates = _rates_of_group(tdcf[4] if len(tdcf) > 4 else tdcf[:3], n_groups)
            weights = [weights] + [tdcf_weights(*r, tdcf[3]) for r in rates]

    W = ops.EVAL_RECORD_WORDS
    sys_words, fused_words = K * 2 * W, 2 * ((n_groups or 0) + 1) * W
    pack = torch.empty(sys_words + fused_words, dtype=torch.int32, device=scores.device)  # [K systems | fused]
    per_system = [DeviceCurveMinima(s, lab, (False, True), out=pack[k * 2 * W:(k + 1) * 2 * W]) for k, (s, lab) in enumerate(rows)]

    def system_eers(host):
        out = []
        for k, m in enumerate(per_system):
            m.fetch(host[k * 2 * W:(k + 1) * 2 * W])
            out.append((m.eer(0)[0], m.eer(1)[0]))
        return out

    fuse_weights = dev_weights = sys_eers = None
    if method == "wght":
        if eers is None:  # the first of the two copies: the systems' records
            sys_eers = system_eers(pack[:sys_words].cpu().numpy())
            eers = [min(e) for e in sys_eers]
        fuse_weights = cal_weight(eers)
        dev_weights = torch.tensor(fuse_weights, dtype=torch.float64).to(torch.float32).to(scores.device)
    fused = ops.score_fuse(scores, dev_index, dev_weights, "mean" if method == "wght" else "sum")
    minima = DeviceGroupedMinima(fused, labels, groups if grouped else None, n_groups or 0, (False, True), weights,
                                 out=pack[sys_words:])
    host = pack.cpu().numpy() if sys_eers is None else pack[sys_words:].cpu().numpy()
    if sys_eers is None:
        sys_eers = system_eers(host)
        host = host[sys_words:]
    minima.fetch(host)
    pair = (minima.eer(0)[0], minima.eer(1)[0])
    win = 0 if pair[0] < pair[1] else 1
    out = FusionResult(fused, fuse_weights, sys_eers, pair, minima.min_tdcf(win)[0] if weights is not None else None)
    if grouped:
        out.by_group = []
        for g in range(n_groups):
            p = (minima.eer(0, g), minima.eer(1, g))
            out.by_group.append(None if p[0] is None else dict(
                eers=(p[0][0], p[1][0]), eer=min(p[0][0], p[1][0]),
                min_tdcf=minima.min_tdcf(win, g)[0] if weights is not None else None))
    return out
