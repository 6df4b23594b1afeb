"""Test infrastructure (numpy): the device's formulation of the DET-curve minima (csrc/eval_metrics.hip: one sort of keys
that carry the group below the class bit, a masked walk per record) as a model that writes air_eval_record words, and the
inputs on which the GPU test holds the kernels to it.  test_eval_groups_cpu.py pins the model to the host functions."""
import numpy as np

from asvspoof2021_air_amd import eval_metrics as em

WALK_SIZES = [1, 2, 3, 4095, 4096, 4097, 8193]  # one block of the sort and of the walk, its edges, three blocks
WALK_GROUPS = [0, 1, 13]  # 0: the call without groups
WALK_KINDS = ("normal", "ties")
WALK_ASV = (0.05, 0.03)  # Pfa_asv, Pmiss_asv; Pmiss_spoof_asv differs by record


def walk_case(n, n_groups, kind, seed):
    """(fp32 scores, labels, groups), NaN- and inf-free.  Both classes wherever n >= 2.  n_groups == 0: every id -1.
    Else ids 0 .. n_groups - 1 with every seventh trial -1 (member of every group) and, from n = 4095 on, three ids
    out of range."""
    rng = np.random.default_rng(seed)
    lab = (rng.random(n) < 0.7).astype(np.int64) * rng.integers(1, 4, n)  # any nonzero label is a spoof
    if n >= 2:
        lab[0], lab[n - 1] = 0, 2
    x = rng.normal(0.0, 1.0, n) + np.where(lab == 0, 1.0, -1.0)
    s = (np.round(2.0 * x) if kind == "ties" else x).astype(np.float32)
    grp = np.full(n, -1, dtype=np.int64)
    if n_groups:
        grp = rng.integers(0, n_groups, n).astype(np.int64)
        grp[::7] = -1
        if n >= 4095:
            grp[[5, 4094, n - 2]] = (-2, n_groups, 1 << 33)
    return s, lab, grp


def walk_rates(n_groups):
    """(Pfa_asv, Pmiss_asv, Pmiss_spoof_asv) per record: row 0 pooled, row 1 + g group g."""
    return [WALK_ASV + (0.1 + 0.8 * r / (n_groups + 1),) for r in range(n_groups + 1)]


def walk_weights(n_groups):
    """The t-DCF weights (C1, C2) per record that go with walk_rates."""
    return [em.tdcf_weights(*r, em.asvspoof19_cost_model()) for r in walk_rates(n_groups)]


def walk_model(s, lab, grp, n_groups, negate=False, weights=None):
    """The device's formulation in numpy: records[1 + g] of air_eval_det_min_grouped (record 0: pooled)."""
    v = (-s if negate else s) + np.float32(0.0)  # -0.0 -> +0.0
    u = v.view(np.uint32).astype(np.uint64)
    img = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    code = np.where((grp >= -1) & (grp < n_groups), grp + 1, 255).astype(np.uint64)
    keys = np.sort((img << np.uint64(9)) | ((lab != 0).astype(np.uint64) << np.uint64(8)) | code)
    k_img, k_spoof, k_code = keys >> np.uint64(9), ((keys >> np.uint64(8)) & np.uint64(1)).astype(np.int64), keys & np.uint64(255)
    bits = np.where(k_img & 0x80000000, k_img ^ 0x80000000, ~k_img & 0xFFFFFFFF).astype(np.uint32)
    sorted_scores = bits.view(np.float32)
    recs = np.zeros(n_groups + 1, dtype=em._RECORD)
    recs[0]["reserved"][0] = int((code == 255).sum())
    for r in range(n_groups + 1):
        member = np.ones(keys.size, bool) if r == 0 else (k_code == 0) | (k_code == r)
        at = np.flatnonzero(member)  # sorted position of the subset's k-th member, k = 1 ..
        rn = np.cumsum(k_spoof[at])
        rt = np.arange(1, at.size + 1) - rn
        rec = recs[r]
        rec["n_non"], rec["n_tar"] = int(k_spoof[at].sum()), int(at.size - k_spoof[at].sum())
        rec["n_inf"] = int(np.isinf(sorted_scores[at]).sum())
        rec["n_distinct"] = int(np.unique(k_img[at]).size)
        if at.size == 0 or rec["n_tar"] == 0 or rec["n_non"] == 0:
            continue
        n_tar, n_non = np.float64(rec["n_tar"]), np.float64(rec["n_non"])
        frr = np.concatenate(([0.0], rt / n_tar))
        far = np.concatenate(([1.0], (int(rec["n_non"]) - rn) / n_non))
        for which, curve in (("eer", np.abs(frr - far)),
                             ("dcf", None if weights is None else (weights[r][0] * frr + weights[r][1] * far) / min(weights[r]))):
            if curve is None:
                continue
            k = int(np.argmin(curve))  # the first minimum
            rec[which + "_idx"], rec[which + "_rej_non"] = k, 0 if k == 0 else int(rn[k - 1])
            rec[which + "_score_first"] = sorted_scores[at[0]]
            rec[which + "_score_at"] = sorted_scores[at[max(k, 1) - 1]]
        rec["has_dcf"] = 0 if weights is None else 1
    return recs


def finish_eer(rec):
    if int(rec["n_tar"]) == 0 or int(rec["n_non"]) == 0:
        return None
    frr, far, thr, _ = em._rates(rec, "eer")
    return float((frr + far) / 2.0), thr
