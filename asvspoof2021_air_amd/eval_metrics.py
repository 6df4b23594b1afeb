"""Equal error rate as the trainer computes it (main_train.py:662-664 calls eval_metrics.compute_eer on
both score polarities).  Host numpy, like the reference: a few hundred to a few ten thousand scores.

Formulation: sort all trials by (score, class) with bona fide trials first among equal scores, then walk the
thresholds once - a threshold at the k-th sorted trial rejects the k lowest trials, so the false-rejection
rate is the share of targets among them and the false-acceptance rate the share of non-targets above them.
Equals the reference's curve (eval_metrics.py:19-46) point for point, ties included
(tests/golden/eer.npz, 1e-12).

Beside it: host ports of the reference's t-DCF (eval_metrics.py:4-16, :49-193, evaluate_tDCF_asvspoof19.py) and the
same minima of the curve found on the GPU for whole dev / eval passes (``*_device``: csrc/eval_metrics.hip sorts one
integer key per trial, scans the class bit and reduces to the first minimum; the host finishes from integer counts,
so every result is bit-equal to the host functions here or a ValueError).  DESIGN.md, "Evaluation on the device".

``*_by_group``: the same figures per spoofing attack or per channel condition, from a group id per trial (-1 = member of
every group) - on the host as a loop over the subsets, on the device from the one sort (``*_by_group_device``)."""
import numpy as np


def compute_det_curve(target_scores, nontarget_scores):
    """(frr, far, thresholds), each of length n_trials + 1; entry 0 = nothing rejected."""
    tar = np.asarray(target_scores, dtype=np.float64).ravel()
    non = np.asarray(nontarget_scores, dtype=np.float64).ravel()
    scores = np.concatenate((tar, non))
    is_non = np.zeros(scores.size, dtype=bool)
    is_non[tar.size:] = True
    order = np.lexsort((is_non, scores))  # by score; among ties targets first
    rejected_non = np.cumsum(is_non[order])
    rejected_tar = np.arange(1, scores.size + 1) - rejected_non
    frr = np.empty(scores.size + 1)
    far = np.empty(scores.size + 1)
    frr[0], far[0] = 0.0, 1.0
    frr[1:] = rejected_tar / tar.size
    far[1:] = (non.size - rejected_non) / non.size
    thresholds = np.empty(scores.size + 1)
    thresholds[1:] = scores[order]
    thresholds[0] = thresholds[1] - 0.001
    return frr, far, thresholds


def compute_eer(target_scores, nontarget_scores):
    """(eer, threshold) at the curve point where |FRR - FAR| is smallest (first such point)."""
    frr, far, thresholds = compute_det_curve(target_scores, nontarget_scores)
    k = int(np.argmin(np.abs(frr - far)))
    return float((frr[k] + far[k]) / 2.0), float(thresholds[k])


def eer_both_polarities(scores, labels):
    """min over both score polarities with label 0 = bona fide (main_train.py:662-664)."""
    scores = np.asarray(scores, dtype=np.float64)
    labels = np.asarray(labels)
    return min(compute_eer(scores[labels == 0], scores[labels == 1])[0],
               compute_eer(-scores[labels == 0], -scores[labels == 1])[0])


# ------------------------------------------------------------------ t-DCF (host ports)
def _asarray(x):
    return np.asarray(x, dtype=np.float64).ravel()


def obtain_asv_error_rates(tar_asv, non_asv, spoof_asv, asv_threshold):
    """(Pfa_asv, Pmiss_asv, Pmiss_spoof_asv) of the ASV system at ``asv_threshold`` (eval_metrics.py:4-16);
    Pmiss_spoof_asv is None when there are no spoof trials."""
    tar_asv, non_asv, spoof_asv = _asarray(tar_asv), _asarray(non_asv), _asarray(spoof_asv)
    Pfa_asv = np.sum(non_asv >= asv_threshold) / non_asv.size
    Pmiss_asv = np.sum(tar_asv < asv_threshold) / tar_asv.size
    Pmiss_spoof_asv = None if spoof_asv.size == 0 else np.sum(spoof_asv < asv_threshold) / spoof_asv.size
    return Pfa_asv, Pmiss_asv, Pmiss_spoof_asv


def asvspoof19_cost_model():
    """The t-DCF parameters of the ASVspoof 2019 evaluation plan (evaluate_tDCF_asvspoof19.py:10-19)."""
    Pspoof = 0.05
    return {"Pspoof": Pspoof, "Ptar": (1 - Pspoof) * 0.99, "Pnon": (1 - Pspoof) * 0.01,
            "Cmiss_asv": 1, "Cfa_asv": 10, "Cmiss_cm": 1, "Cfa_cm": 10}


def tdcf_weights(Pfa_asv, Pmiss_asv, Pmiss_spoof_asv, cost_model):
    """The weights (C1, C2) of the t-DCF curve with the reference's checks (eval_metrics.py:134-166); what it ends
    the process for raises ValueError."""
    cm = cost_model
    if cm["Ptar"] < 0 or cm["Pnon"] < 0 or cm["Pspoof"] < 0 or np.abs(cm["Ptar"] + cm["Pnon"] + cm["Pspoof"] - 1) > 1e-10:
        raise ValueError("the prior probabilities should be positive and sum up to one")
    if Pmiss_spoof_asv is None:
        raise ValueError("the miss rate of spoof tests against the ASV system is needed")
    C1 = cm["Ptar"] * (cm["Cmiss_cm"] - cm["Cmiss_asv"] * Pmiss_asv) - cm["Pnon"] * cm["Cfa_asv"] * Pfa_asv
    C2 = cm["Cfa_cm"] * cm["Pspoof"] * (1 - Pmiss_spoof_asv)
    if C1 < 0 or C2 < 0 or np.isnan(C1) or np.isnan(C2):
        raise ValueError("t-DCF cannot be evaluated with negative weights (C1 = %r, C2 = %r): check the ASV error rates" % (C1, C2))
    return C1, C2


def compute_tDCF(bonafide_score_cm, spoof_score_cm, Pfa_asv, Pmiss_asv, Pmiss_spoof_asv, cost_model, print_cost=False):
    """(tDCF_norm, CM_thresholds) over the n + 1 operating points of the countermeasure (eval_metrics.py:49-193);
    higher scores support the bona fide hypothesis."""
    C1, C2 = tdcf_weights(Pfa_asv, Pmiss_asv, Pmiss_spoof_asv, cost_model)
    bona, spoof = _asarray(bonafide_score_cm), _asarray(spoof_score_cm)
    combined = np.concatenate((bona, spoof))
    if np.isnan(combined).any() or np.isinf(combined).any():
        raise ValueError("the scores contain nan or inf")
    if np.unique(combined).size < 3:
        raise ValueError("soft CM scores are needed, not binary decisions")
    Pmiss_cm, Pfa_cm, CM_thresholds = compute_det_curve(bona, spoof)
    tDCF = C1 * Pmiss_cm + C2 * Pfa_cm
    tDCF_norm = tDCF / np.minimum(C1, C2)
    if print_cost:
        print("t-DCF evaluation from [Nbona={}, Nspoof={}] trials\n".format(bona.size, spoof.size))
        if C2 == np.minimum(C1, C2):
            print("   tDCF_norm(s) = {:8.5f} x Pmiss_cm(s) + Pfa_cm(s)\n".format(C1 / C2))
        else:
            print("   tDCF_norm(s) = Pmiss_cm(s) + {:8.5f} x Pfa_cm(s)\n".format(C2 / C1))
    return tDCF_norm, CM_thresholds


def compute_eer_and_tdcf(cm_score_file, asv_score_file):
    """(min EER over both polarities, min t-DCF of the polarity with the lower EER) of a CM score file
    ``utt source key score`` against the organisers' ASV score file ``source key score``
    (evaluate_tDCF_asvspoof19.py:6-67, :120, without the plots)."""
    asv = np.genfromtxt(asv_score_file, dtype=str)
    asv_keys, asv_scores = asv[:, 1], asv[:, 2].astype(np.float64)
    cm = np.genfromtxt(cm_score_file, dtype=str)
    cm_keys, cm_scores = cm[:, 2], cm[:, 3].astype(np.float64)
    tar_asv, non_asv, spoof_asv = (asv_scores[asv_keys == k] for k in ("target", "nontarget", "spoof"))
    bona_cm, spoof_cm = cm_scores[cm_keys == "bonafide"], cm_scores[cm_keys == "spoof"]
    _, asv_threshold = compute_eer(tar_asv, non_asv)
    eer_cm = compute_eer(bona_cm, spoof_cm)[0]
    other_eer_cm = compute_eer(-bona_cm, -spoof_cm)[0]
    rates = obtain_asv_error_rates(tar_asv, non_asv, spoof_asv, asv_threshold)
    if eer_cm < other_eer_cm:
        curve, _ = compute_tDCF(bona_cm, spoof_cm, *rates, asvspoof19_cost_model())
    else:
        curve, _ = compute_tDCF(-bona_cm, -spoof_cm, *rates, asvspoof19_cost_model())
    return min(eer_cm, other_eer_cm), float(curve[np.argmin(curve)])


# ------------------------------------------------------------------ breakdown by attack / by channel condition
# Every trial carries an integer group id: g in 0 .. n_groups - 1 puts it into group g, -1 into EVERY group.  Per-attack
# table: bona fide trials -1, spoof trials their attack index.  Per-channel table: every trial its condition.  Group g's
# result is BY DEFINITION what the pooled functions above return for the subset {i : g_i == g or g_i == -1}; a group
# without bona fide or without spoof trials (a dev set that lacks the attack) gives None.
def _checked_groups(groups, n_groups, n):
    groups = np.asarray(groups).ravel()
    n_groups = int(n_groups)
    if n_groups < 1:
        raise ValueError("n_groups must be at least 1, got %d" % n_groups)
    if groups.size != n or not np.issubdtype(groups.dtype, np.integer):
        raise ValueError("groups must be %d integers" % n)
    bad = int(np.count_nonzero((groups < -1) | (groups >= n_groups)))
    if bad:
        raise ValueError("%d group ids lie outside -1 .. %d" % (bad, n_groups - 1))
    return groups, n_groups


def _subsets(scores, labels, groups, n_groups):
    """Per group the (bona fide scores, spoof scores) of its subset; label 0 = bona fide, anything else = spoof."""
    scores = _asarray(scores)
    labels = np.asarray(labels).ravel()
    groups, n_groups = _checked_groups(groups, n_groups, scores.size)
    for g in range(n_groups):
        member = (groups == g) | (groups == -1)
        yield scores[member & (labels == 0)], scores[member & (labels != 0)]


def _rates_of_group(rates_by_group, n_groups):
    """n_groups triples (Pfa_asv, Pmiss_asv, Pmiss_spoof_asv) from one triple for all groups or one per group."""
    rates = list(rates_by_group)
    if len(rates) == 3 and not any(isinstance(r, (tuple, list, np.ndarray)) for r in rates):
        return [tuple(rates)] * n_groups
    if len(rates) != n_groups or any(len(r) != 3 for r in rates):
        raise ValueError("rates_by_group must be one (Pfa_asv, Pmiss_asv, Pmiss_spoof_asv) or one per group (%d)" % n_groups)
    return [tuple(r) for r in rates]


def compute_eer_by_group(scores, labels, groups, n_groups):
    """[compute_eer of group g's subset, or None where it lacks a class] for g in 0 .. n_groups - 1."""
    return [compute_eer(tar, non) if tar.size and non.size else None for tar, non in _subsets(scores, labels, groups, n_groups)]


def eer_both_polarities_by_group(scores, labels, groups, n_groups):
    """Per group the lower of the two polarities' EERs (eer_both_polarities of its subset), or None."""
    scores = _asarray(scores)
    pos = compute_eer_by_group(scores, labels, groups, n_groups)
    neg = compute_eer_by_group(-scores, labels, groups, n_groups)
    return [None if p is None else min(p[0], q[0]) for p, q in zip(pos, neg)]


def min_tdcf_by_group(scores, labels, groups, n_groups, rates_by_group, cost_model):
    """Per group (min, argmin) of compute_tDCF over its subset's curve, or None where the subset lacks a class.
    ``rates_by_group``: one (Pfa_asv, Pmiss_asv, Pmiss_spoof_asv) for all groups or one per group (a per-attack table
    takes Pmiss_spoof_asv from that attack's ASV trials).  What compute_tDCF refuses raises here too."""
    rates = _rates_of_group(rates_by_group, int(n_groups))
    for r in rates:
        tdcf_weights(*r, cost_model)  # (refused before any curve is walked)
    out = []
    for (tar, non), r in zip(_subsets(scores, labels, groups, n_groups), rates):
        if not (tar.size and non.size):
            out.append(None)
            continue
        curve, _ = compute_tDCF(tar, non, *r, cost_model)
        k = int(np.argmin(curve))
        out.append((float(curve[k]), k))
    return out


def compute_eer_and_tdcf_by_source(cm_score_file, asv_score_file):
    """compute_eer_and_tdcf broken down by the ``source`` column of the CM score file ``utt source key score``:
    ({source: (eer, min_tdcf)}, (pooled eer, pooled min_tdcf)).  A source is an attack: its subset is every bona fide
    trial plus its own spoof trials.  The ASV threshold, Pfa_asv and Pmiss_asv are the pooled ones, Pmiss_spoof_asv is
    taken over the ASV rows of that source, and every entry uses the ONE polarity that wins the pooled EER."""
    asv = np.genfromtxt(asv_score_file, dtype=str)
    asv_src, asv_keys, asv_scores = asv[:, 0], asv[:, 1], asv[:, 2].astype(np.float64)
    cm = np.genfromtxt(cm_score_file, dtype=str)
    cm = cm[(cm[:, 2] == "bonafide") | (cm[:, 2] == "spoof")]
    cm_src, cm_keys, cm_scores = cm[:, 1], cm[:, 2], cm[:, 3].astype(np.float64)
    tar_asv, non_asv, spoof_asv = (asv_scores[asv_keys == k] for k in ("target", "nontarget", "spoof"))
    bona_cm, spoof_cm = cm_scores[cm_keys == "bonafide"], cm_scores[cm_keys == "spoof"]
    _, asv_threshold = compute_eer(tar_asv, non_asv)
    eer_cm = compute_eer(bona_cm, spoof_cm)[0]
    other_eer_cm = compute_eer(-bona_cm, -spoof_cm)[0]
    Pfa_asv, Pmiss_asv, Pmiss_spoof_asv = obtain_asv_error_rates(tar_asv, non_asv, spoof_asv, asv_threshold)
    sign = 1.0 if eer_cm < other_eer_cm else -1.0
    curve, _ = compute_tDCF(sign * bona_cm, sign * spoof_cm, Pfa_asv, Pmiss_asv, Pmiss_spoof_asv, asvspoof19_cost_model())
    pooled = (min(eer_cm, other_eer_cm), float(curve[np.argmin(curve)]))
    sources = sorted(set(cm_src[cm_keys == "spoof"].tolist()))
    if not sources:
        return {}, pooled
    labels = (cm_keys == "spoof").astype(np.int64)
    groups = np.full(cm_scores.size, -1, dtype=np.int64)
    rates = []
    for g, src in enumerate(sources):
        groups[(labels == 1) & (cm_src == src)] = g
        of_src = asv_scores[(asv_keys == "spoof") & (asv_src == src)]
        rates.append((Pfa_asv, Pmiss_asv, obtain_asv_error_rates(tar_asv, non_asv, of_src, asv_threshold)[2]))
    eers = compute_eer_by_group(sign * cm_scores, labels, groups, len(sources))
    tdcfs = min_tdcf_by_group(sign * cm_scores, labels, groups, len(sources), rates, asvspoof19_cost_model())
    return {src: (eers[g][0], tdcfs[g][0]) for g, src in enumerate(sources)}, pooled


# ------------------------------------------------------------------ on the device (csrc/eval_metrics.hip)
_RECORD = np.dtype([("n_tar", "<u4"), ("n_non", "<u4"), ("n_nan", "<u4"), ("n_inf", "<u4"), ("n_distinct", "<u4"),
                    ("has_dcf", "<u4"), ("eer_idx", "<u4"), ("eer_rej_non", "<u4"), ("eer_score_first", "<f4"),
                    ("eer_score_at", "<f4"), ("dcf_idx", "<u4"), ("dcf_rej_non", "<u4"), ("dcf_score_first", "<f4"),
                    ("dcf_score_at", "<f4"), ("reserved", "<u4", (2,))])  # air_eval_record (include/air_hip.h)


def _rates(rec, which):
    """(frr, far, threshold, k) at the record's EER / t-DCF point, from its integer counts as compute_det_curve has them."""
    k, rn = int(rec[which + "_idx"]), int(rec[which + "_rej_non"])
    n_tar, n_non = int(rec["n_tar"]), int(rec["n_non"])
    frr = np.float64(k - rn) / np.float64(n_tar)
    far = np.float64(n_non - rn) / np.float64(n_non)
    thr = np.float64(rec[which + "_score_at"]) if k > 0 else np.float64(rec[which + "_score_first"]) - 0.001
    return frr, far, float(thr), k


def _check_record(rec, tdcf=False):
    if int(rec["n_nan"]) > 0:
        raise ValueError("%d scores are NaN" % int(rec["n_nan"]))
    if int(rec["n_tar"]) == 0 or int(rec["n_non"]) == 0:
        raise ValueError("both classes need trials (bona fide: %d, spoof: %d)" % (int(rec["n_tar"]), int(rec["n_non"])))
    if tdcf:
        if int(rec["n_inf"]) > 0:
            raise ValueError("the scores contain nan or inf")
        if int(rec["n_distinct"]) < 3:
            raise ValueError("soft CM scores are needed, not binary decisions")


class DeviceGroupedMinima:
    """The enqueued device metrics of one score set, for the pooled trials and every group from one sort per polarity
    (ops.eval_det_min_grouped): ``records`` is (P, n_groups + 1, 16) int32 on the GPU (``out`` when the caller packs it
    with other results of a pass), row 0 of a polarity the pooled air_eval_record, row 1 + g group g's - what the chain
    writes for that subset alone.  ``weights``: None or (n_groups + 1, 2) t-DCF weights (C1, C2) per record.  Without
    groups (``groups`` None, ``n_groups`` 0: ops.eval_det_min, nothing uploaded) the axis of the groups is left out:
    ``records`` (P, 16), ``fetch()`` (P,).  Nothing has been copied back or synchronised until ``fetch()`` /
    ``result()``; ids outside -1 .. n_groups - 1 raise ValueError there."""

    def __init__(self, scores, labels, groups, n_groups, negates, weights=None, out=None):
        import torch
        from . import ops
        given = (scores, labels) if groups is None else (scores, labels, groups)
        if not all(torch.is_tensor(t) and t.is_cuda for t in given):
            raise ValueError("the device metrics take GPU tensors (compute_eer / compute_eer_by_group are the host path)")
        if scores.dtype != torch.float32:
            raise ValueError("scores must be fp32, got %s" % scores.dtype)
        given = [t.reshape(-1).contiguous() for t in given]
        self.n_groups = int(n_groups)
        self.negates = tuple(bool(n) for n in negates)
        self.weights = None if weights is None else np.asarray(weights, dtype=np.float64).reshape(self.n_groups + 1, 2)
        if groups is None:
            self._shape = (len(self.negates),)
            nbytes = ops.eval_workspace_bytes(given[0].numel())
            c1, c2 = (None, None) if weights is None else (float(self.weights[0, 0]), float(self.weights[0, 1]))
            run = lambda rows, neg: ops.eval_det_min(*given, rows, ws, negate=neg, c1=c1, c2=c2)
        else:
            self._shape = (len(self.negates), self.n_groups + 1)
            nbytes = ops.eval_workspace_bytes_grouped(given[0].numel(), self.n_groups)
            c12 = None if weights is None else torch.from_numpy(self.weights).to(scores.device)
            run = lambda rows, neg: ops.eval_det_min_grouped(*given, self.n_groups, rows, ws, negate=neg, c12=c12)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=scores.device)
        shape = self._shape + (ops.EVAL_RECORD_WORDS,)
        self.records = out.view(shape) if out is not None else torch.empty(shape, dtype=torch.int32, device=scores.device)
        for rows, neg in zip(self.records, self.negates):  # back to back on the stream, sharing the scratch
            run(rows, neg)
        self._host = None

    def fetch(self, host_words=None):
        """The single device-to-host copy (or the caller's copy of the packed ``out``, as int32 words)."""
        if self._host is None:
            words = self.records.cpu().numpy() if host_words is None else np.asarray(host_words)
            host = np.ascontiguousarray(words, dtype=np.int32).reshape(-1).view(_RECORD).reshape(self._shape)
            bad = int(host[0, 0]["reserved"][0]) if host.ndim == 2 else 0
            if bad:
                raise ValueError("%d group ids lie outside -1 .. %d" % (bad, self.n_groups - 1))
            self._host = host
        return self._host

    def _record(self, i, g, tdcf=False):
        """Polarity i's record of group g (None: pooled), checked; None for a group that lacks a class."""
        rec = self.fetch()[i] if len(self._shape) == 1 else self.fetch()[i, 0 if g is None else 1 + g]
        if g is not None and int(rec["n_nan"]) == 0 and (int(rec["n_tar"]) == 0 or int(rec["n_non"]) == 0):
            return None
        _check_record(rec, tdcf)
        return rec

    def eer(self, i=0, g=None):
        """(eer, threshold) of polarity i (of its group g), finished on the host as compute_eer does."""
        rec = self._record(i, g)
        if rec is None:
            return None
        frr, far, thr, _ = _rates(rec, "eer")
        return float((frr + far) / 2.0), thr

    def min_tdcf(self, i=0, g=None):
        """(min t-DCF, index of the operating point) of polarity i (of its group g): the device's argmin, the value
        recomputed from the counts with the host formula of compute_tDCF."""
        rec = self._record(i, g, tdcf=True)
        if rec is None:
            return None
        C1, C2 = self.weights[0 if g is None else 1 + g]
        frr, far, _, k = _rates(rec, "dcf")
        return float((C1 * frr + C2 * far) / np.minimum(C1, C2)), k


class DeviceCurveMinima(DeviceGroupedMinima):
    """DeviceGroupedMinima without groups: one air_eval_record per polarity; ``weights``: None or the pair (C1, C2)."""

    def __init__(self, scores, labels, negates, weights=None, out=None):
        super().__init__(scores, labels, None, 0, negates, weights, out)


class _Pending:
    def __init__(self, minima, finish):
        self.minima, self._finish = minima, finish

    def result(self, refresh=False):
        """``refresh``: copy the records again (the enqueued work was captured in a graph and replayed since)."""
        if refresh:
            self.minima._host = None
        return self._finish(self.minima)


def compute_eer_device(scores, labels, negate=False):
    """compute_eer(scores[labels == 0], scores[labels != 0]) (of -scores with ``negate``) for fp32 scores and integer
    labels on the GPU, up to 2^20 trials: enqueued on the current stream; ``.result()`` makes the one device-to-host
    copy and returns (eer, threshold), bit-equal to compute_eer's.  ValueError for NaN scores or an empty class."""
    return _Pending(DeviceCurveMinima(scores, labels, (negate,)), lambda m: m.eer(0))


def eer_both_polarities_device(scores, labels):
    """eer_both_polarities on the GPU: both polarities enqueued back to back, one host copy in ``.result()``."""
    return _Pending(DeviceCurveMinima(scores, labels, (False, True)), lambda m: min(m.eer(0)[0], m.eer(1)[0]))


def min_tdcf_device(scores, labels, Pfa_asv, Pmiss_asv, Pmiss_spoof_asv, cost_model, negate=False):
    """min and argmin of compute_tDCF(scores[labels == 0], scores[labels != 0], ...)[0] on the GPU: the host computes
    and checks the weights, the device finds the first minimum of the curve; ``.result()`` -> (min t-DCF, index).
    NaN / inf scores, fewer than three distinct scores or an empty class raise ValueError there."""
    weights = tdcf_weights(Pfa_asv, Pmiss_asv, Pmiss_spoof_asv, cost_model)
    return _Pending(DeviceCurveMinima(scores, labels, (negate,), weights), lambda m: m.min_tdcf(0))


# ------------------------------------------------------------------ the breakdown on the device
def eer_by_group_device(scores, labels, groups, n_groups, negate=False):
    """compute_eer_by_group (of -scores with ``negate``) for fp32 scores and integer labels / groups on the GPU, up to
    2^20 trials and ops.EVAL_MAX_GROUPS groups: one sort for all groups, enqueued on the current stream; ``.result()``
    makes the one device-to-host copy and returns the list, bit-equal to the host's."""
    m = DeviceGroupedMinima(scores, labels, groups, n_groups, (negate,))
    return _Pending(m, lambda m: [m.eer(0, g) for g in range(m.n_groups)])


def eer_both_polarities_by_group_device(scores, labels, groups, n_groups):
    """eer_both_polarities_by_group on the GPU: both polarities enqueued back to back, one host copy in ``.result()``."""
    def finish(m):
        pairs = [(m.eer(0, g), m.eer(1, g)) for g in range(m.n_groups)]
        return [None if p is None else min(p[0], q[0]) for p, q in pairs]
    return _Pending(DeviceGroupedMinima(scores, labels, groups, n_groups, (False, True)), finish)


def min_tdcf_by_group_device(scores, labels, groups, n_groups, rates_by_group, cost_model, negate=False):
    """min_tdcf_by_group on the GPU: the host computes and checks each group's weights, the device finds the first
    minimum of every group's curve; ``.result()`` -> [(min t-DCF, index) or None]."""
    rates = _rates_of_group(rates_by_group, int(n_groups))
    weights = [(1.0, 1.0)] + [tdcf_weights(*r, cost_model) for r in rates]  # (row 0: the pooled record, not read here)
    m = DeviceGroupedMinima(scores, labels, groups, n_groups, (negate,), weights)
    return _Pending(m, lambda m: [m.min_tdcf(0, g) for g in range(m.n_groups)])
