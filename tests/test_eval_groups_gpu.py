"""GPU: the breakdown of the device EER / min t-DCF by group (air_eval_det_min_grouped, eval_metrics.*_by_group_device,
Trainer.evaluate(n_groups=...)).  The oracle is the ungrouped kernel and the host functions: group g's record must be,
field for field, the record ``ops.eval_det_min`` writes for the subset {i : g_i == g or g_i == -1} compacted on the host,
and ``.result()`` must equal compute_eer_by_group / min_tdcf_by_group with ``==`` (this file's contract is bit equality).

Sizes: 1, 2, 3 trials; 4095, 4096, 4097 (the sort block and the walk's block of 4096 curve points), 8193 (three
blocks), 71,237 (the ASVspoof 2019 LA evaluation set), 2^20 (the limit).  Groups: 1, 2, 13 (the attacks of an
evaluation set) and the most the library takes."""
import numpy as np
import pytest
import torch

from oracle.filler import fill_module_, synth_pcm

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 4095, 4096, 4097, 8193, 71237]
KINDS = ("normal", "ties", "zeros", "half")
COUNT_FIELDS = ("n_tar", "n_non", "n_nan", "n_inf")
FIELDS = COUNT_FIELDS + ("n_distinct", "has_dcf", "eer_idx", "eer_rej_non", "eer_score_first", "eer_score_at", "dcf_idx",
                         "dcf_rej_non", "dcf_score_first", "dcf_score_at")
ASV = (0.05, 0.03)  # Pfa_asv, Pmiss_asv; Pmiss_spoof_asv differs by group


def max_groups():
    from asvspoof2021_air_amd import _hip, ops
    g = _hip.lib().air_eval_max_groups()
    assert g == ops.EVAL_MAX_GROUPS >= 128  # 7 codecs x 13 attacks = 91 must fit
    return g


def make_case(n, G, mode, kind, mix, seed):
    """(fp32 scores, labels, groups).  mode "partition": every trial in one group; "attack": bona fide trials -1, spoof
    trials their group.  With G >= 13 and n >= 4095: group 0 holds the 700 lowest scores alone (its members sit in one
    sort block) while the others are spread over all blocks, group G - 1 has one member, group G - 2 only spoof trials."""
    rng = np.random.default_rng(seed)
    lab = np.ones(n, dtype=np.int64)
    n_tar = max(1, n // 10) if mix == "1:9" else (1 if mix == "1:rest" else n - 1)
    lab[:max(1, min(n_tar, n - 1)) if n > 1 else 0] = 0
    rng.shuffle(lab)
    lab = lab * rng.integers(1, 5, n)  # any nonzero label is a spoof
    x = rng.normal(0.0, 1.0, n) + np.where(lab == 0, 1.0, -1.0)
    if kind == "ties":
        s = np.round(2.0 * x)
    elif kind == "zeros":
        s = rng.choice(np.array([-0.0, 0.0, -0.0, 0.0, -1.0, 1.0]), n)
    elif kind == "half":
        s = np.round(2.0 * x) / 2.0
        s[::5] = -0.0
    else:
        s = x
    s = s.astype(np.float32)
    grp = rng.integers(0, G, n).astype(np.int64)
    if G >= 13 and n >= 4095:
        grp[grp == 0] = 1
        grp[grp >= G - 2] = 2
        grp[np.argsort(s, kind="stable")[:700]] = 0
        spoof = np.flatnonzero((lab != 0) & (grp > 0))
        if spoof.size > 50:
            grp[spoof[:50]] = G - 2
            grp[spoof[50]] = G - 1
    if mode == "attack":
        grp[lab == 0] = -1
    return s, lab, grp


def rates_of(G):
    return [ASV + (0.1 + 0.8 * g / G,) for g in range(G)]


def parent_records(s, lab, grp, G, negate, weights):
    """Per record (0: pooled) what the ungrouped kernel writes for the subset compacted on the host, or None for a
    group without members."""
    from asvspoof2021_air_amd import eval_metrics as em, ops
    out, pend = [], []
    ws = torch.empty(ops.eval_workspace_bytes(s.size), dtype=torch.uint8, device="cuda")
    for r in range(G + 1):
        m = np.ones(s.size, bool) if r == 0 else (grp == r - 1) | (grp == -1)
        if not m.any():
            pend.append(None)
            continue
        rec = torch.empty(ops.EVAL_RECORD_WORDS, dtype=torch.int32, device="cuda")
        c1, c2 = (None, None) if weights is None else weights[r]
        ops.eval_det_min(torch.from_numpy(s[m]).cuda(), torch.from_numpy(lab[m]).cuda(), rec, ws, negate=negate, c1=c1, c2=c2)
        pend.append(rec)
    for rec in pend:
        out.append(None if rec is None else rec.cpu().numpy().view(em._RECORD)[0])
    return out


def check_records(s, lab, grp, G, weights, negates, tag, gdtype=torch.int64):
    """Every record of the grouped call against the ungrouped kernel on the compacted subset, field by field (the count
    fields alone where the subset holds a NaN: the parent's other fields mean nothing then)."""
    from asvspoof2021_air_amd import eval_metrics as em
    ds, dl, dg = torch.from_numpy(s).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(grp).cuda().to(gdtype)
    minima = em.DeviceGroupedMinima(ds, dl, dg, G, negates, weights)
    got = minima.fetch()
    for i, negate in enumerate(negates):
        want = parent_records(s, lab, grp, G, negate, weights)
        for r in range(G + 1):
            if want[r] is None:
                assert all(int(got[i, r][f]) == 0 for f in COUNT_FIELDS + ("n_distinct",)), (tag, negate, r)
                continue
            for f in (COUNT_FIELDS if int(want[r]["n_nan"]) > 0 else FIELDS):
                a, b = got[i, r][f], want[r][f]
                assert a.tobytes() == b.tobytes(), (tag, negate, r, f, a, b)
    return minima, (ds, dl, dg)


def check_case(s, lab, grp, G, with_tdcf=True, negates=(False, True), tag=None, gdtype=torch.int64):
    from asvspoof2021_air_amd import eval_metrics as em
    cost = em.asvspoof19_cost_model()
    rates = rates_of(G)
    weights = [em.tdcf_weights(*(ASV + (0.5,)), cost)] + [em.tdcf_weights(*r, cost) for r in rates] if with_tdcf else None
    minima, (ds, dl, dg) = check_records(s, lab, grp, G, weights, negates, tag, gdtype)
    host_eers = []
    for i, negate in enumerate(negates):
        h = (-s if negate else s).astype(np.float64)
        host_eers.append(em.compute_eer_by_group(h, lab, grp, G))
        assert em.eer_by_group_device(ds, dl, dg, G, negate=negate).result() == host_eers[i], (tag, negate)
        assert [minima.eer(i, g) for g in range(G)] == host_eers[i], (tag, negate)
        if with_tdcf:
            pending = em.min_tdcf_by_group_device(ds, dl, dg, G, rates, cost, negate=negate)
            try:
                host = em.min_tdcf_by_group(h, lab, grp, G, rates, cost)
            except ValueError:  # fewer than three distinct scores, or inf, in some group: refused on both sides
                with pytest.raises(ValueError):
                    pending.result()
            else:
                assert pending.result() == host, (tag, negate)
    if tuple(negates) == (False, True):
        want = [None if p is None else min(p[0], q[0]) for p, q in zip(*host_eers)]
        assert em.eer_both_polarities_by_group_device(ds, dl, dg, G).result() == want, tag


@pytest.mark.parametrize("n", SIZES)
def test_grouped_records_equal_the_ungrouped_kernel_on_each_subset(n):
    combos = [(G, mode) for G in (1, 2, 13, max_groups()) for mode in ("partition", "attack")]
    for j, (G, mode) in enumerate(combos):
        kind, mix = KINDS[(j + n) % len(KINDS)], ("1:9", "1:rest", "rest:1")[(j // 2 + n) % 3]
        s, lab, grp = make_case(n, G, mode, kind, mix, 100 * n + j)
        check_case(s, lab, grp, G, tag=(n, G, mode, kind, mix), gdtype=torch.int32 if j % 2 else torch.int64)


def test_special_groups_are_where_the_case_puts_them():
    """What make_case promises: one group inside one sort block, the others over all blocks, a one-member group and a
    group that lacks a class."""
    from asvspoof2021_air_amd import _hip
    block = _hip.lib().air_eval_sort_block()
    s, lab, grp = make_case(8193, 13, "partition", "normal", "1:9", 1)
    pos = np.empty(s.size, np.int64)
    pos[np.lexsort((grp, lab != 0, s + np.float32(0.0)))] = np.arange(s.size)
    assert pos[grp == 0].max() < block and (grp == 0).sum() == 700
    assert {int(p) // block for p in pos[grp == 3]} >= {0, 1}
    assert (grp == 12).sum() == 1 and (lab[grp == 11] != 0).all() and (grp == 11).sum() == 50
    assert {block - 1, block, block + 1} <= set(SIZES)


@pytest.mark.parametrize("G", [1, 5])
def test_every_trial_in_every_group(G):
    """All ids -1: every group's record is the pooled record (also without t-DCF weights: has_dcf = 0)."""
    from asvspoof2021_air_amd import eval_metrics as em
    for kind, with_tdcf in (("normal", True), ("ties", False), ("zeros", False)):
        s, lab, _ = make_case(5000, G, "partition", kind, "1:9", 7)
        grp = np.full(s.size, -1, dtype=np.int64)
        check_case(s, lab, grp, G, with_tdcf=with_tdcf, tag=(kind, G))
        h = s.astype(np.float64)
        got = em.eer_by_group_device(*(torch.from_numpy(a).cuda() for a in (s, lab, grp)), G).result()
        assert got == [em.compute_eer(h[lab == 0], h[lab != 0])] * G


def test_nan_and_inf_are_counted_per_group():
    from asvspoof2021_air_amd import eval_metrics as em
    s, lab, grp = make_case(6000, 3, "partition", "normal", "1:9", 11)
    s[np.flatnonzero(grp == 0)[:4]] = np.inf
    s[np.flatnonzero(grp == 1)[:2]] = -np.inf
    s[np.flatnonzero(grp == 1)[5]] = np.nan
    m, _ = check_records(s, lab, grp, 3, [(1.0, 2.0)] * 4, (False, True), "nan")
    assert [int(m.fetch()[0, r]["n_inf"]) for r in range(4)] == [6, 4, 2, 0]
    assert [int(m.fetch()[0, r]["n_nan"]) for r in range(4)] == [1, 0, 1, 0]
    assert m.eer(0, 0) is not None and m.min_tdcf(0, 2) is not None
    for bad in (lambda: m.eer(0, 1), lambda: m.eer(0), lambda: m.min_tdcf(0, 0)):  # NaN; NaN; inf
        with pytest.raises(ValueError):
            bad()


def test_errors():
    from asvspoof2021_air_amd import _hip, eval_metrics as em, ops
    s, lab, grp = make_case(5000, 4, "partition", "normal", "1:9", 3)
    ds, dl, dg = (torch.from_numpy(a).cuda() for a in (s, lab, grp))
    for bad in (-2, 4, 1 << 40):  # counted on the device, refused on the host
        g = grp.copy()
        g[[17, 4500]] = bad
        pending = em.eer_by_group_device(ds, dl, torch.from_numpy(g).cuda(), 4)
        with pytest.raises(ValueError):
            pending.result()
        assert int(pending.minima.records.cpu().numpy().view(em._RECORD)[0, 0, 0]["reserved"][0]) == 2
    G = max_groups()
    for n_groups in (0, G + 1):
        with pytest.raises(ValueError):
            em.eer_by_group_device(ds, dl, dg, n_groups)
        assert _hip.lib().air_eval_workspace_bytes_grouped(_hip.ci(5000), _hip.ci(n_groups)) == 0
    # the C entry point itself: AIR_EUNSUPPORTED for n_groups out of range, AIR_EWORKSPACE for a short workspace
    ws = torch.empty(ops.eval_workspace_bytes_grouped(5000, 4), dtype=torch.uint8, device="cuda")
    recs = torch.empty((G + 2) * ops.EVAL_RECORD_WORDS, dtype=torch.int32, device="cuda")

    def call(n_groups, ws_bytes):
        return _hip.lib().air_eval_det_min_grouped(
            _hip.dptr(ds), _hip.dptr(dl, torch.int64), _hip.ci(8), _hip.dptr(dg, torch.int64), _hip.ci(8), _hip.ci(5000),
            _hip.ci(n_groups), _hip.ci(0), _hip.ci(0), None, _hip.dptr(recs, torch.int32), _hip.dptr(ws, torch.uint8),
            _hip.csz(ws_bytes), _hip.stream())
    assert call(G + 1, ws.numel()) == -2 and call(0, ws.numel()) == -2
    assert call(4, ws.numel() - 1) == -4 and call(4, ws.numel()) == 0
    with pytest.raises(ValueError):
        ops.eval_det_min_grouped(ds, dl, dg, 4, recs[:5 * ops.EVAL_RECORD_WORDS], ws[:-1])
    with pytest.raises(ValueError):
        ops.eval_det_min_grouped(ds, dl, dg[:-1], 4, recs[:5 * ops.EVAL_RECORD_WORDS], ws)
    with pytest.raises(ValueError):
        ops.eval_det_min_grouped(ds, dl, dg, 4, recs[:4 * ops.EVAL_RECORD_WORDS], ws)
    with pytest.raises(_hip.AirError):
        ops.eval_det_min_grouped(ds, dl, dg.to(torch.int16), 4, recs[:5 * ops.EVAL_RECORD_WORDS], ws)
    with pytest.raises(ValueError):
        em.eer_by_group_device(ds, dl, torch.from_numpy(grp), 4)  # host tensor: compute_eer_by_group is the host path
    with pytest.raises(ValueError):  # a missing miss rate is refused before anything is enqueued
        em.min_tdcf_by_group_device(ds, dl, dg, 4, [ASV + (None,)] * 4, em.asvspoof19_cost_model())
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", ["partition", "attack"])
def test_at_the_limit(mode):
    """2^20 trials: partition mode with the most groups the library takes, attack mode with 13."""
    n = 1 << 20
    G = max_groups() if mode == "partition" else 13
    s, lab, grp = make_case(n, G, mode, "normal" if mode == "partition" else "half", "1:9", 20)
    check_case(s, lab, grp, G, negates=(mode == "attack",), tag=(n, G, mode))


def test_both_polarities_by_group_replay_in_a_graph():
    """As test_both_polarities_replay_in_a_graph: one warm-up call, then the grouped both-polarities metric captured in a
    single-stream graph and replayed on three sets copied into its static inputs."""
    from asvspoof2021_air_amd import eval_metrics as em
    n, G = 10007, 13
    sets = [make_case(n, G, mode, kind, mix, 40 + i) for i, (mode, kind, mix) in enumerate(
        (("attack", "normal", "1:9"), ("partition", "ties", "rest:1"), ("attack", "half", "1:9")))]
    ss, sl, sg = (torch.from_numpy(a).cuda() for a in sets[0])
    want0 = em.eer_both_polarities_by_group(sets[0][0].astype(np.float64), sets[0][1], sets[0][2], G)
    assert em.eer_both_polarities_by_group_device(ss, sl, sg, G).result() == want0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pending = em.eer_both_polarities_by_group_device(ss, sl, sg, G)
    for s, lab, grp in reversed(sets):
        ss.copy_(torch.from_numpy(s))
        sl.copy_(torch.from_numpy(lab))
        sg.copy_(torch.from_numpy(grp))
        graph.replay()
        assert pending.result(refresh=True) == em.eer_both_polarities_by_group(s.astype(np.float64), lab, grp, G)


def test_the_groups_share_one_sort():
    """A grouped call at G = 13 launches as many sort kernels as an ungrouped call of the same n."""
    from torch.profiler import ProfilerActivity, profile
    from asvspoof2021_air_amd import eval_metrics as em
    n, G = 71237, 13
    s, lab, grp = make_case(n, G, "attack", "normal", "1:9", 5)
    ds, dl, dg = (torch.from_numpy(a).cuda() for a in (s, lab, grp))

    def sort_launches(fn):
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA]
        return sum("ev_sort_block_kernel" in k or "ev_merge_global_kernel" in k for k in names), names

    plain, _ = sort_launches(lambda: em.compute_eer_device(ds, dl))
    grouped, names = sort_launches(lambda: em.eer_by_group_device(ds, dl, dg, G))
    assert plain > 0 and grouped == plain, (plain, grouped)
    assert any("ev_curve_kernel" in k for k in names)


# ------------------------------------------------------------------ Trainer.evaluate(n_groups=...)
def _model(kind):
    if kind == "resnet":
        from asvspoof2021_air_amd.resnet import ResNet
        m = ResNet(3, 256, resnet_type="18", nclasses=2)
        fill_module_(m)
        m.set_attention_noise(None)  # two passes see the same arithmetic
        return m
    from asvspoof2021_air_amd.ecapa_tdnn import Bottle2neck, Res2Net2
    m = Res2Net2(Bottle2neck, C=512, model_scale=8, nOut=2, n_mels=60)
    fill_module_(m)
    return m


@pytest.mark.parametrize("kind", ["ecapa", "resnet"])
def test_evaluate_breaks_the_pass_down_by_group(kind):
    from asvspoof2021_air_amd import eval_metrics as em
    from asvspoof2021_air_amd.train import Trainer
    tr = Trainer(_model(kind), feat_len=128, ecapa=(kind == "ecapa"))
    fill_module_(tr.loss)
    B, G = 4, 4
    cost = em.asvspoof19_cost_model()
    rates = (0.05, 0.03, 0.4)
    per_group = [(0.05, 0.03, 0.2 + 0.1 * g) for g in range(G)]
    plain, attack, channel = [], [], []
    for i in range(6):
        pcm = synth_pcm(B, 16000, seed=700 + i).cuda()
        lab = ((torch.arange(B) + i) % 3 != 0).long()
        att = torch.where(lab == 0, torch.full_like(lab, -1), (torch.arange(B) + 2 * i) % 3)  # attack 3: no trial
        cond = (torch.arange(B) * 3 + i) % G
        plain.append((pcm, lab.cuda()))
        attack.append((pcm, lab.cuda(), None, None, att.cuda()))
        channel.append((pcm, lab.cuda(), None, None, cond.to(torch.int32)))  # host groups are uploaded like labels
    base = tr.evaluate(plain, tdcf=rates + (cost,))
    assert base.by_group is None
    names = ["A07", "A08", "A09", "A10"]
    for batches, groups, tdcf, by in ((attack, [b[4] for b in attack], rates + (cost, per_group), per_group),
                                      (iter(channel), [b[4] for b in channel], rates + (cost,), [rates] * G),
                                      (attack, [b[4] for b in attack], None, None)):
        out = tr.evaluate(batches, tdcf=tdcf, n_groups=G, group_names=names)
        loss, eer, min_tdcf, scores, labels = out  # still five fields
        assert loss == base.loss and eer == base.eer and min_tdcf == (base.min_tdcf if tdcf is not None else None)
        assert torch.equal(scores, base.scores) and torch.equal(labels, base.labels)
        s, lab = scores.cpu().numpy().astype(np.float64), labels.cpu().numpy()
        grp = torch.cat([g.cpu().long() for g in groups]).numpy()
        pos, neg = em.compute_eer_by_group(s, lab, grp, G), em.compute_eer_by_group(-s, lab, grp, G)
        pooled = (em.compute_eer(s[lab == 0], s[lab != 0])[0], em.compute_eer(-s[lab == 0], -s[lab != 0])[0])
        win = 0 if pooled[0] < pooled[1] else 1
        dcf = em.min_tdcf_by_group(-s if win else s, lab, grp, G, by, cost) if by is not None else [None] * G
        assert len(out.by_group) == G and any(e is not None for e in out.by_group)
        for g, entry in enumerate(out.by_group):
            if pos[g] is None:
                assert entry is None
                continue
            assert entry.name == names[g] and entry.eers == (pos[g][0], neg[g][0])
            assert entry.eer == entry.eers[win]  # the pooled polarity, never a per-group minimum
            assert entry.min_tdcf == (dcf[g][0] if by is not None else None)
        if batches is attack:
            assert out.by_group[3] is None
    assert tr.evaluate(attack, n_groups=G).by_group[0].name == 0
    with pytest.raises(ValueError):
        tr.evaluate(plain, n_groups=G)  # batches without groups
    with pytest.raises(ValueError):
        tr.evaluate(attack, n_groups=G, group_names=names[:2])
    with pytest.raises(ValueError):
        tr.evaluate(plain, group_names=names)
    with pytest.raises(ValueError):
        tr.evaluate(attack, n_groups=2)  # attack ids 2 lie outside 2 groups
