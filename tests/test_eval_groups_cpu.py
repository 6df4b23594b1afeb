"""CPU: the breakdown of EER / min t-DCF by group (eval_metrics.compute_eer_by_group and friends) against a brute-force
loop over the subsets, and a numpy model of the device's walk (one sort of keys that carry the group below the class
bit, a masked scan per group: eval_walk_oracle.walk_model) pinned to the same subset functions with ``==``."""
import numpy as np
import pytest

from asvspoof2021_air_amd import eval_metrics as em
from eval_walk_oracle import (WALK_ASV, WALK_GROUPS, WALK_KINDS, WALK_SIZES, finish_eer, walk_case, walk_model, walk_rates,
                              walk_weights)

RATES = (0.05, 0.03, 0.4)


def make_case(kind, n, n_groups, mode, seed):
    """(fp32 scores, labels, groups).  mode "partition": every trial one group; "attack": bona fide -1, spoof its group."""
    rng = np.random.default_rng(seed)
    lab = (rng.random(n) < 0.7).astype(np.int64) * rng.integers(1, 4, n)  # any nonzero label is a spoof
    x = rng.normal(0.0, 1.0, n) + np.where(lab == 0, 1.0, -1.0)
    if kind == "tied":
        s = rng.integers(0, 3, n).astype(np.float64)  # three distinct values shared by groups and classes
    elif kind == "half":
        s = np.round(2.0 * x) / 2.0
        s[s == 0.0] = np.where(rng.random(int((s == 0.0).sum())) < 0.5, -0.0, 0.0)
    else:
        s = x
    grp = rng.integers(0, n_groups, n)
    if mode == "attack":
        grp[lab == 0] = -1
    return s.astype(np.float32), lab, grp.astype(np.int64)


def brute_force(s, lab, grp, n_groups, rates=None, only=None):
    """The definition, written out: per group (``only``: those groups) the pooled function on the subset's bona fide and
    spoof scores."""
    out = []
    for g in (range(n_groups) if only is None else only):
        idx = [i for i in range(s.size) if grp[i] == g or grp[i] == -1]
        tar = np.array([s[i] for i in idx if lab[i] == 0], dtype=np.float64)
        non = np.array([s[i] for i in idx if lab[i] != 0], dtype=np.float64)
        if tar.size == 0 or non.size == 0:
            out.append(None)
        elif rates is None:
            out.append(em.compute_eer(tar, non))
        else:
            curve, _ = em.compute_tDCF(tar, non, *rates[g], em.asvspoof19_cost_model())
            out.append((float(curve[np.argmin(curve)]), int(np.argmin(curve))))
    return out


@pytest.mark.parametrize("mode", ["partition", "attack"])
@pytest.mark.parametrize("kind", ["random", "tied", "half"])
def test_by_group_equals_the_loop_over_subsets(kind, mode):
    cost = em.asvspoof19_cost_model()
    for n, G in ((1, 1), (2, 1), (3, 2), (40, 3), (257, 13), (600, 40)):
        s, lab, grp = make_case(kind, n, G, mode, 17 * n + G)
        rates = [(RATES[0], RATES[1], 0.1 + 0.8 * g / G) for g in range(G)]  # a C2 per group
        for sign in (1.0, -1.0):
            h = sign * s.astype(np.float64)
            want = brute_force(h, lab, grp, G)
            assert em.compute_eer_by_group(h, lab, grp, G) == want
            few = [g for g in range(G) if want[g] is not None and np.unique(h[(grp == g) | (grp == -1)]).size < 3]
            if few:  # compute_tDCF refuses fewer than three distinct scores; so does the breakdown
                with pytest.raises(ValueError):
                    em.min_tdcf_by_group(h, lab, grp, G, rates, cost)
            else:
                assert em.min_tdcf_by_group(h, lab, grp, G, rates, cost) == brute_force(h, lab, grp, G, rates)
        both = em.eer_both_polarities_by_group(s, lab, grp, G)
        pos, neg = brute_force(s.astype(np.float64), lab, grp, G), brute_force(-s.astype(np.float64), lab, grp, G)
        assert both == [None if p is None else min(p[0], q[0]) for p, q in zip(pos, neg)]


def test_one_rate_triple_serves_every_group():
    s, lab, grp = make_case("random", 300, 4, "attack", 3)
    cost = em.asvspoof19_cost_model()
    assert em.min_tdcf_by_group(s, lab, grp, 4, RATES, cost) == em.min_tdcf_by_group(s, lab, grp, 4, [RATES] * 4, cost)
    with pytest.raises(ValueError):
        em.min_tdcf_by_group(s, lab, grp, 4, [RATES] * 3, cost)
    with pytest.raises(ValueError):  # a miss rate is missing: refused before any curve
        em.min_tdcf_by_group(s, lab, grp, 4, [RATES] * 3 + [(0.05, 0.03, None)], cost)


def test_a_group_that_lacks_a_class_gives_none():
    s = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6], dtype=np.float32)
    lab = np.array([0, 1, 0, 1, 1, 0])
    grp = np.array([0, 0, 1, 2, 0, 1])  # group 1: bona fide only, group 2: spoof only, group 3: nobody
    got = em.compute_eer_by_group(s, lab, grp, 4)
    assert got[0] == em.compute_eer(s[[0]], s[[1, 4]]) and got[1:] == [None, None, None]
    assert em.min_tdcf_by_group(s, lab, grp, 4, RATES, em.asvspoof19_cost_model())[1:] == [None, None, None]
    assert em.eer_both_polarities_by_group(s, lab, grp, 4)[1:] == [None, None, None]


@pytest.mark.parametrize("bad", [-2, 3, 1 << 40])
def test_ids_out_of_range_raise(bad):
    s, lab, grp = make_case("random", 50, 3, "partition", 1)
    grp[7] = bad
    for fn in (em.compute_eer_by_group, em.eer_both_polarities_by_group):
        with pytest.raises(ValueError):
            fn(s, lab, grp, 3)
    with pytest.raises(ValueError):
        em.min_tdcf_by_group(s, lab, grp, 3, RATES, em.asvspoof19_cost_model())
    with pytest.raises(ValueError):
        em.compute_eer_by_group(s, lab, grp[:-1], 3)
    with pytest.raises(ValueError):
        em.compute_eer_by_group(s, lab, np.zeros(50), 3)  # floating-point ids
    with pytest.raises(ValueError):
        em.compute_eer_by_group(s, lab, np.zeros(50, np.int64), 0)


def test_one_group_of_everybody_is_the_pooled_result():
    for kind in ("random", "tied", "half"):
        s, lab, _ = make_case(kind, 500, 1, "partition", 9)
        every = np.full(500, -1)
        h = s.astype(np.float64)
        assert em.compute_eer_by_group(h, lab, every, 1) == [em.compute_eer(h[lab == 0], h[lab != 0])]
        assert em.eer_both_polarities_by_group(h, lab, every, 1) == [em.eer_both_polarities(h, np.minimum(lab, 1))]
        if kind != "tied" or np.unique(h).size >= 3:
            curve, _ = em.compute_tDCF(h[lab == 0], h[lab != 0], *RATES, em.asvspoof19_cost_model())
            assert em.min_tdcf_by_group(h, lab, every, 1, RATES, em.asvspoof19_cost_model()) == [
                (float(curve[np.argmin(curve)]), int(np.argmin(curve)))]


@pytest.mark.parametrize("mode", ["partition", "attack"])
@pytest.mark.parametrize("kind", ["random", "tied", "half"])
def test_the_walk_model_equals_the_subset_functions(kind, mode):
    """What the kernel computes, modelled in numpy: sort once, walk per group.  EER, threshold, min t-DCF and its index
    equal the subset functions bit for bit, in both polarities, with shared bona fide trials and tied scores."""
    cost = em.asvspoof19_cost_model()
    for n, G in ((1, 1), (5, 2), (64, 3), (300, 13), (700, 128)):
        s, lab, grp = make_case(kind, n, G, mode, 5 * n + G)
        rates = [(RATES[0], RATES[1], 0.1 + 0.8 * g / G) for g in range(G)]
        weights = [(1.0, 1.0)] + [em.tdcf_weights(*r, cost) for r in rates]
        for negate in (False, True):
            h = (-s if negate else s).astype(np.float64)
            recs = walk_model(s, lab, grp, G, negate, weights)
            assert int(recs[0]["reserved"][0]) == 0
            assert finish_eer(recs[0]) == (em.compute_eer(h[lab == 0], h[lab != 0]) if (lab == 0).any() and (lab != 0).any() else None)
            assert [finish_eer(r) for r in recs[1:]] == em.compute_eer_by_group(h, lab, grp, G), (kind, mode, n, G, negate)
            for g in range(G):
                sub = h[(grp == g) | (grp == -1)]
                rec = recs[1 + g]
                assert int(rec["n_distinct"]) == np.unique(sub).size and int(rec["n_tar"]) + int(rec["n_non"]) == sub.size
                if finish_eer(rec) is None or np.unique(sub).size < 3:
                    continue
                frr, far, _, k = em._rates(rec, "dcf")
                got = (float((weights[1 + g][0] * frr + weights[1 + g][1] * far) / np.minimum(*weights[1 + g])), k)
                assert got == brute_force(h, lab, grp, G, rates, only=[g])[0], (kind, mode, n, G, negate, g)


def test_the_walk_model_counts_ids_out_of_range():
    s, lab, grp = make_case("random", 90, 4, "partition", 2)
    grp[[3, 50, 51]] = (-2, 4, 1 << 33)
    assert int(walk_model(s, lab, grp, 4)[0]["reserved"][0]) == 3


@pytest.mark.parametrize("n", WALK_SIZES)
def test_the_walk_model_without_groups_equals_the_pooled_host_functions(n):
    """The numpy side of test_eval_walk_gpu.py on that test's own inputs: at n_groups = 0 the model's one record finishes
    to compute_eer's pair, and its t-DCF point is the first minimum of compute_tDCF's curve at the same weights (where
    compute_tDCF takes the scores: three distinct ones)."""
    cost = em.asvspoof19_cost_model()
    assert WALK_GROUPS[0] == 0
    (c1, c2), = walk_weights(0)
    for j, kind in enumerate(WALK_KINDS):
        s, lab, grp = walk_case(n, 0, kind, 10 * n + j)
        assert (grp == -1).all() and not np.isnan(s).any() and not np.isinf(s).any()
        for negate in (False, True):
            h = (-s if negate else s).astype(np.float64)
            rec, = walk_model(s, lab, grp, 0, negate, walk_weights(0))
            both = (lab == 0).any() and (lab != 0).any()
            assert both == (n >= 2)
            assert finish_eer(rec) == (em.compute_eer(h[lab == 0], h[lab != 0]) if both else None), (n, kind, negate)
            assert int(rec["n_distinct"]) == np.unique(h).size and int(rec["reserved"][0]) == 0
            if both and np.unique(h).size >= 3:
                curve, _ = em.compute_tDCF(h[lab == 0], h[lab != 0], *WALK_ASV, walk_rates(0)[0][2], cost)
                frr, far, _, k = em._rates(rec, "dcf")
                assert (float((c1 * frr + c2 * far) / np.minimum(c1, c2)), k) == (float(curve[np.argmin(curve)]), int(np.argmin(curve)))


# ------------------------------------------------------------------ score files
def write_scores(tmp_path, flip=False):
    rng = np.random.default_rng(4)
    attacks = ["A07", "A08", "A19"]
    cm, asv = [], []
    for i in range(400):
        src = "-" if i % 4 == 0 else attacks[i % 3]
        key = "bonafide" if src == "-" else "spoof"
        mean = {"-": 2.0, "A07": -2.0, "A08": -0.5, "A19": 1.0}[src]
        score = rng.normal(mean, 1.0) * (-1.0 if flip else 1.0)
        cm.append("LA_E_%07d %s %s %.6f" % (i, src, key, score))
    for i in range(600):
        kind = ("target", "nontarget", "spoof")[i % 3]
        src = attacks[(i // 3) % 3] if kind == "spoof" else "-"
        mean = {"target": 3.0, "nontarget": -3.0}.get(kind, {"A07": 2.5, "A08": 0.0, "A19": -2.0}.get(src))
        asv.append("%s %s %.6f" % (src, kind, rng.normal(mean, 1.0)))
    cm_file, asv_file = tmp_path / ("cm%d.txt" % flip), tmp_path / "asv.txt"
    cm_file.write_text("\n".join(cm) + "\n")
    asv_file.write_text("\n".join(asv) + "\n")
    return str(cm_file), str(asv_file), attacks


@pytest.mark.parametrize("flip", [False, True])
def test_eer_and_tdcf_by_source(tmp_path, flip):
    cm_file, asv_file, attacks = write_scores(tmp_path, flip)
    table, pooled = em.compute_eer_and_tdcf_by_source(cm_file, asv_file)
    assert pooled == em.compute_eer_and_tdcf(cm_file, asv_file)
    assert sorted(table) == attacks
    # written out from the files: pooled ASV threshold, the attack's own ASV spoof trials, the pooled polarity
    cm = np.genfromtxt(cm_file, dtype=str)
    asv = np.genfromtxt(asv_file, dtype=str)
    sc, asc = cm[:, 3].astype(np.float64), asv[:, 2].astype(np.float64)
    tar, non = asc[asv[:, 1] == "target"], asc[asv[:, 1] == "nontarget"]
    thr = em.compute_eer(tar, non)[1]
    bona, spoof = sc[cm[:, 2] == "bonafide"], sc[cm[:, 2] == "spoof"]
    sign = 1.0 if em.compute_eer(bona, spoof)[0] < em.compute_eer(-bona, -spoof)[0] else -1.0
    assert sign == (-1.0 if flip else 1.0)
    for a in attacks:
        sp = sc[(cm[:, 2] == "spoof") & (cm[:, 1] == a)]
        rates = em.obtain_asv_error_rates(tar, non, asc[(asv[:, 1] == "spoof") & (asv[:, 0] == a)], thr)
        curve, _ = em.compute_tDCF(sign * bona, sign * sp, *rates, em.asvspoof19_cost_model())
        assert table[a] == (em.compute_eer(sign * bona, sign * sp)[0], float(curve[np.argmin(curve)]))
    assert table["A07"][0] < table["A08"][0] < table["A19"][0]  # the attacks were drawn closer and closer to bona fide
