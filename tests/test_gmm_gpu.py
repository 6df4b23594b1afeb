"""GPU: csrc/gmm.hip and gmm.py (DiagGMM, GMMBackend) against the numpy fp64 oracle tests/gmm_oracle.py, within the
bounds derived there; exact integer data for the f64 MFMA operand and result maps."""
import functools

import numpy as np
import pytest
import torch

import gmm_oracle as go

pytestmark = pytest.mark.gpu
REG = 1e-6
LAYOUTS = ("nd", "bdt")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _model(w, mu, var, reg=REG):
    from asvspoof2021_air_amd.gmm import DiagGMM
    return DiagGMM(mu.shape[0], mu.shape[1], reg).set_params(w, mu, var)


def _feats(x, layout, B=1):
    """(N, D) host frames as one device batch of B equal rows in ``layout``."""
    N, D = x.shape
    if layout == "nd":
        assert B == 1
        return _dev(x), None
    rows = x.reshape(B, N // B, D)
    return (_dev(rows), "btd") if layout == "btd" else (_dev(rows.transpose(0, 2, 1)), "bdt")


def _stats(m):
    return [_np(s) for s in m.statistics()]


def _accumulated(m, x, layout, B=1, n_frames=None):
    f, lay = _feats(x, layout, B)
    return m.begin().accumulate(f, n_frames, lay)


def _check_stats(got, x, w, mu, var, n_terms=None):
    want = go.statistics(x, w, mu, var)
    bound = go.statistics_bound(x, w, mu, var, n_terms)
    for g, e, b, what in zip(got[:4], want[:4], bound, ("S0", "S1", "S2", "LL")):
        err = np.abs(g - e)
        print(what, "max err / allowance", float(np.max(err / (go.BOTH * b + 1e-300))), "max err", float(np.max(err)))
        assert np.all(np.isfinite(g)) and np.all(err <= go.BOTH * b), what
    assert int(got[4]) == want[4]


def _init(x, K, seed):
    """go.init_from_data, and for K > N (the 512-component model on one tile + 1 frames) frames drawn with
    replacement and moved by a fraction of the global deviation."""
    if K <= x.shape[0]:
        return go.init_from_data(x, K, seed, REG)
    rng = np.random.default_rng(seed)
    x64 = x.astype(np.float64)
    sd = x64.std(axis=0)
    return np.full(K, 1.0 / K), x64[rng.integers(0, len(x), K)] + 0.5 * sd * rng.normal(size=(K, x.shape[1])), \
        np.tile(x64.var(axis=0) + REG, (K, 1))


# ------------------------------------------------------------------------------------------- 1. exact operand maps
LIVE70 = [int(6.9 * i) for i in range(11)]  # 0, 6, 13, .. 62, 69: every 16-component tile and both 64-component chunks


def _far_apart(K, D):
    """Components keyed on coordinate 0 (variance 1e-4: neighbouring integers differ by 5000 nats, far beyond the
    745 at which exp underflows to exactly 0), every other coordinate shared.  K = 5: means -2 .. 2; K = 70: the
    eleven values -5 .. 5 at the components LIVE70, the rest out of reach."""
    mu = np.zeros((K, D))
    var = np.full((K, D), 1.0e6)
    var[:, 0] = 1.0e-4
    if K == 5:
        mu[:, 0] = np.arange(5) - 2.0
        owner = lambda v: int(np.clip(v, -2, 2)) + 2
    else:
        mu[:, 0] = 1000.0 + np.arange(K)
        mu[LIVE70, 0] = np.arange(11) - 5.0
        owner = lambda v: LIVE70[int(v) + 5]
    return np.full(K, 1.0 / K), mu, var, owner


@pytest.mark.parametrize("layout", ("btd", "bdt"))
@pytest.mark.parametrize("D", (1, 7, 60))
@pytest.mark.parametrize("K", (1, 5, 70))
def test_integer_frames_give_the_integer_sums_bit_for_bit(K, D, layout):
    N = 150  # three rows of 50 frames: two full 64-frame tiles and a short one, tiles across row boundaries
    x = go.integer_frames(N, D)
    if K == 1:
        w, mu, var, owner = np.ones(1), np.full((1, D), 0.5), np.ones((1, D)), (lambda v: 0)
    else:
        w, mu, var, owner = _far_apart(K, D)
    own = np.array([owner(v) for v in x[:, 0]])
    x64 = x.astype(np.float64)
    S0, S1, S2 = np.zeros(K), np.zeros((K, D)), np.zeros((K, D))
    for k in range(K):
        S0[k], S1[k], S2[k] = np.sum(own == k), x64[own == k].sum(axis=0), (x64[own == k] ** 2).sum(axis=0)
    got = _stats(_accumulated(_model(w, mu, var), x, layout, B=3))
    assert np.array_equal(got[0], S0) and np.array_equal(got[1], S1) and np.array_equal(got[2], S2)
    assert int(got[4]) == N and np.isfinite(got[3])


# -------------------------------------------------------------------------------- 2. one EM step against the oracle
def _tile():
    from asvspoof2021_air_amd import gmm
    return gmm.frame_tile()


STEP_CASES = ((1, 1, 1), (15, 7, 3), (17, 60, 37), ("tile+1", 60, 512), (4099, 128, 1024))


@functools.lru_cache(maxsize=None)
def _step_case(N, D, K):
    x = go.lfcc_like(N, D, seed=N + D)
    return x, _init(x, K, seed=K)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: "%s-%s-%s" % c)
def test_one_em_step_within_the_fp64_bound(case, layout):
    """LFCC-like frames (offset 25, variances down to 1e-4): an fp32 accumulation misses these bounds by six orders."""
    N, D, K = case
    N = _tile() + 1 if N == "tile+1" else N
    x, init = _step_case(N, D, K)
    m = _accumulated(_model(*init), x, layout)
    _check_stats(_stats(m), x, *init)
    f, lay = _feats(x, layout)
    ll = _np(m.score_samples(f, None, lay)).reshape(-1)
    assert np.all(np.abs(ll - go.score_samples(x, *init)) <= go.BOTH * go.lse_bound(x, *init))
    lb = m.m_step()
    w, mu, var, lower = go.m_step(*go.statistics(x, *init), REG)
    dw, dmu, dvar, dlb = go.params_bound(x, *init, REG)
    for g, e, b, what in ((m.weights_, w, dw, "w"), (m.means_, mu, dmu, "mu"), (m.covariances_, var, dvar, "var")):
        err = np.abs(_np(g) - e)
        print(what, "max err / allowance", float(np.max(err / (go.BOTH * b))), "max relative", float(np.max(err / (np.abs(e) + 1e-300))))
        assert np.all(err <= go.BOTH * b), what
    assert abs(lb.item() - lower) <= go.BOTH * dlb


# ------------------------------------------------------------------------------------------------ 3. ragged batches
N_FRAMES = [0, 1, 16, 33, 40]  # the last is clamped to Tcap


def _ragged(layout, D=7, Tcap=33, seed=9):
    B = len(N_FRAMES)
    x = go.lfcc_like(B * Tcap, D, seed).reshape(B, Tcap, D)
    valid = [min(n, Tcap) for n in N_FRAMES]
    rows = [x[b, :valid[b]].copy() for b in range(B)]
    for b in range(B):
        x[b, valid[b]:] = np.nan  # the tails: nothing may read them into the arithmetic
    host = x if layout == "btd" else x.transpose(0, 2, 1)
    # the batch is the middle of a larger buffer of NaN: a read before or behind it poisons the result
    big = torch.full((3 * host.size,), float("nan"), dtype=torch.float32, device="cuda")
    feats = big[host.size:2 * host.size].view(host.shape)
    feats.copy_(_dev(host))
    return feats, rows, big


GUARD = 256  # canary elements in front of and behind every buffer the kernels write


def _guarded(numel, dtype, fill):
    """(the buffer, the tensor it is the middle of): a write before or past the buffer lands in the canaries."""
    big = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return big[GUARD:GUARD + numel], big


def _canaries_intact(big, fill):
    return bool((big[:GUARD] == fill).all()) and bool((big[-GUARD:] == fill).all())


@pytest.mark.parametrize("layout", ("btd", "bdt"))
def test_ragged_batch_equals_the_dense_call_on_its_valid_frames(layout):
    from asvspoof2021_air_amd import gmm
    feats, rows, big = _ragged(layout)
    dense = np.concatenate(rows)
    init = go.init_from_data(dense, 3, seed=4, reg_covar=REG)
    nf = _dev(np.array(N_FRAMES, dtype=np.int32))
    m = _model(*init)
    # every buffer the kernels write is the middle of a larger one: statistics, workspace (exactly the size the
    # library asks for), frame and row scores
    m._stats, stats_big = _guarded(3 + 2 * 3 * 7 + 2, torch.float64, 7.25)
    m._ws, ws_big = _guarded(gmm.ws_bytes(5 * 33, 3, 7), torch.uint8, 0xA5)
    ll_out, ll_big = _guarded(5 * 33, torch.float64, 7.25)
    rs_out, rs_big = _guarded(5, torch.float64, 7.25)
    m.begin().accumulate(feats, nf, layout)
    got = _stats(m)
    _check_stats(got, dense, *init)
    ref = _stats(_accumulated(_model(*init), dense, "nd"))
    bound = go.statistics_bound(dense, *init)
    for g, r, b in zip(got[:4], ref[:4], bound):
        assert np.all(np.abs(g - r) <= go.BOTH * b)
    assert int(got[4]) == int(ref[4]) == len(dense)
    # scores: the frames of each row, zeros behind them; the row means; NaN for the row without frames
    ll = _np(m.score_samples(feats, nf, layout, out=ll_out))
    rs = _np(m.score_rows(feats, nf, layout, out=rs_out))
    assert ll.shape == (5, 33) and np.isnan(rs[0])
    for b, r in enumerate(rows):
        want, bnd = go.score_samples(r, *init) if len(r) else np.zeros(0), go.lse_bound(r, *init) if len(r) else np.zeros(0)
        assert np.all(np.abs(ll[b, :len(r)] - want) <= go.BOTH * bnd) and np.all(ll[b, len(r):] == 0.0)
        if len(r):
            assert abs(rs[b] - want.mean()) <= go.BOTH * (bnd.mean() + (len(r) + 2) * go.U * np.abs(want).mean())
    # an all-empty batch leaves the statistics as they are, bit for bit
    before = m._stats.clone()
    m.accumulate(feats, torch.zeros(5, dtype=torch.int32, device="cuda"), layout)
    assert torch.equal(before, m._stats)
    # the input and its surroundings were only read
    n = feats.numel()
    assert bool(torch.isnan(big[:n]).all()) and bool(torch.isnan(big[2 * n:]).all())
    # nothing was written in front of or behind the outputs, and the calls used the guarded buffers
    assert m._stats.data_ptr() == stats_big.data_ptr() + 8 * GUARD and m._ws.data_ptr() == ws_big.data_ptr() + GUARD
    assert _canaries_intact(stats_big, 7.25) and _canaries_intact(ws_big, 0xA5)
    assert _canaries_intact(ll_big, 7.25) and _canaries_intact(rs_big, 7.25)


# --------------------------------------------------------------------------------- 4. accumulation and determinism
def test_split_calls_accumulate_and_equal_calls_give_equal_bits():
    feats, rows, _ = _ragged("bdt", D=60, seed=10)
    dense = np.concatenate(rows)
    init = go.init_from_data(dense, 37, seed=6, reg_covar=REG)
    nf = _dev(np.array(N_FRAMES, dtype=np.int32))
    one = _model(*init).begin().accumulate(feats, nf, "bdt")
    again = _model(*init).begin().accumulate(feats, nf, "bdt")
    assert torch.equal(one._stats, again._stats)
    two = _model(*init).begin().accumulate(feats[:3].contiguous(), nf[:3], "bdt").accumulate(feats[3:].contiguous(), nf[3:], "bdt")
    bound = go.statistics_bound(dense, *init)
    for g, r, b in zip(_stats(one)[:4], _stats(two)[:4], bound):
        assert np.all(np.abs(g - r) <= go.BOTH * b)
    assert int(_stats(two)[4]) == len(dense)
    _check_stats(_stats(two), dense, *init)


def test_m_step_alone_matches_to_a_few_ulps():
    x = go.lfcc_like(500, 60, seed=12)
    init = go.init_from_data(x, 6, seed=2, reg_covar=REG)
    S0, S1, S2, LL, Nf = go.statistics(x, *init)
    S0[4], S1[4], S2[4] = 0.0, 0.0, 0.0  # an empty component
    m = _model(*init).begin()
    K, D = 6, 60
    m._stats[:K + 2 * K * D + 1].copy_(_dev(np.concatenate([S0, S1.ravel(), S2.ravel(), [LL]])))
    m._stats[K + 2 * K * D + 1:].view(torch.int64).fill_(Nf)
    lb = m.m_step().item()
    w, mu, var, lower = go.m_step(S0, S1, S2, LL, Nf, REG)
    bw, bmu, bvar = go.m_step_bound(S0, S1, S2, REG)
    gw, gmu, gvar = _np(m.weights_), _np(m.means_), _np(m.covariances_)
    assert np.all(np.isfinite(gw)) and np.all(np.isfinite(gmu)) and np.all(np.isfinite(gvar))
    assert np.all(np.abs(gw - w) <= bw) and np.all(np.abs(gmu - mu) <= bmu) and np.all(np.abs(gvar - var) <= bvar)
    assert np.all(gmu[4] == 0.0) and np.all(gvar[4] == REG)
    assert abs(lb - lower) <= 2 * go.U * abs(lower)


# ----------------------------------------------------------------------------------------------------- 5. extremes
def test_far_frames_and_vanishing_weights_stay_finite():
    x = go.lfcc_like(64, 4, seed=1)
    w, mu, var = go.init_from_data(x, 3, seed=1, reg_covar=REG)
    far = (mu[0] + 1.0e3 * np.sqrt(var[0]) * np.array([1.0, -1.0, 1.0, -1.0])).astype(np.float32)[None, :]
    m = _accumulated(_model(w, mu, var), far, "nd")
    S0, S1, S2, LL, Nf = _stats(m)
    assert np.isfinite(LL) and LL < -1.0e5 and int(Nf) == 1
    assert abs(S0.sum() - 1.0) <= 16 * go.U and np.all(np.isfinite(S1)) and np.all(np.isfinite(S2))
    _check_stats([S0, S1, S2, LL, Nf], far, w, mu, var)
    w2 = np.array([1.0e-300, 0.5, 0.5])
    m = _accumulated(_model(w2, mu, var), x, "nd")
    got = _stats(m)
    assert all(np.all(np.isfinite(g)) for g in got[:4])
    _check_stats(got, x, w2, mu, var)
    m.m_step()
    assert all(bool(torch.isfinite(t).all()) for t in (m.weights_, m.means_, m.covariances_))


# ---------------------------------------------------------------------------------------------------------- 6. fit
# The drift ten data-dependent iterations allow cannot be derived; it is measured: the oracle's own largest drift over
# 8 random frame permutations (w, var and the lower bound relative, mu relative to |mu| + sqrt(var)), times 16 because
# a tree of partial sums differs from a permutation by more than a permutation differs from itself.  Measured on the
# CPU: 5.7e-13 for (2053, 3, 4) and 1.5e-10 for (4099, 60, 16) - recorded in profiles/gmm_backend.md.
FIT_CASES = {"2053-3-4": (2053, 3, 4, 0.0, 9.1e-12), "4099-60-16": (4099, 60, 16, 25.0, 2.4e-9)}


@pytest.mark.parametrize("name", sorted(FIT_CASES))
def test_fit_follows_the_oracle(name):
    N, D, K, offset, drift = FIT_CASES[name]
    x = go.separable(N, D, K, seed=1, offset=offset)
    init = go.init_from_data(x, K, seed=11, reg_covar=REG)
    o = go.fit(x, *init, reg_covar=REG, max_iter=10, tol=1e-3)
    change = np.abs(np.diff([-np.inf] + o["bounds"]))
    assert np.all(np.abs(change - 1e-3) > 1e-6)  # n_iter_ / converged_ cannot hinge on rounding
    xd = _dev(x)
    cut = N // 3
    m = _model(*init).fit(lambda: [(xd[:cut], None), (xd[cut:], None)], max_iter=10, tol=1e-3)
    assert (m.n_iter_, m.converged_) == (o["n_iter"], o["converged"])
    gw, gmu, gvar = _np(m.weights_), _np(m.means_), _np(m.covariances_)
    errs = (np.max(np.abs(gw - o["w"]) / o["w"]), np.max(np.abs(gmu - o["mu"]) / (np.abs(o["mu"]) + np.sqrt(o["var"]))),
            np.max(np.abs(gvar - o["var"]) / o["var"]), abs(m.lower_bound_ - o["lower_bound"]) / abs(o["lower_bound"]))
    print(name, "drift (w, mu, var, lower bound)", errs, "allowed", drift)
    assert max(errs) <= drift


def test_init_from_frames():
    feats, rows, _ = _ragged("bdt", D=7, seed=13)
    dense = np.concatenate(rows).astype(np.float64)
    from asvspoof2021_air_amd.gmm import DiagGMM
    m = DiagGMM(5, 7, REG).init_from_frames(feats, _dev(np.array(N_FRAMES, dtype=np.int32)), "bdt", seed=3)
    mu = _np(m.means_)
    assert all(np.any(np.all(dense == mu[k], axis=1)) for k in range(5)) and len(np.unique(mu, axis=0)) == 5
    assert np.array_equal(_np(m.weights_), np.full(5, 0.2))
    var = dense.var(axis=0) + REG
    assert np.allclose(_np(m.covariances_), np.tile(var, (5, 1)), rtol=1e-9, atol=0)
    with pytest.raises(ValueError):
        DiagGMM(84, 7, REG).init_from_frames(feats, _dev(np.array(N_FRAMES, dtype=np.int32)), "bdt")


# ----------------------------------------------------------------------------------- 7. the back-end on a corpus
@pytest.fixture(scope="module")
def corpus():
    from asvspoof2021_air_amd import synth
    from asvspoof2021_air_amd.corpus import DeviceCorpus
    lengths = [8000 + 331 * ((7 * i) % 19) for i in range(24)]  # 0.5 .. 0.9 s
    utts, labels = [], []
    for i, n in enumerate(lengths):
        pcm, lab = synth.utterance(21, i, length=n)
        utts.append(pcm)
        labels.append(lab)
    cap = max(lengths) + 8 - max(lengths) % 8
    host = np.zeros((len(utts), cap), dtype=np.float32)
    for b, r in enumerate(utts):
        host[b, :len(r)] = r
    c = DeviceCorpus(torch.float32).reserve(sum(lengths) + 8 * len(lengths), len(lengths))
    c.append(_dev(host), lengths, np.array(labels))
    return c, np.array(labels), lengths, cap


def test_backend_fit_score_evaluate_and_score_file(corpus, tmp_path):
    from asvspoof2021_air_amd import eval_metrics, score_fusion
    from asvspoof2021_air_amd.generate_score import format_score_line, test_on_dataset_gmm
    from asvspoof2021_air_amd.gmm import GMMBackend
    c, labels, lengths, cap = corpus
    assert 4 <= labels.sum() <= 20
    walk = lambda: c.sampler(8, shuffle=False, Lcap=cap).epoch()
    be = GMMBackend(n_components=4)
    # the frames on the host, per utterance, as the back-end computes them
    rows = []
    for b in walk():
        feats, nf = be.frames(b.pcm, b.lengths)
        f, n = _np(feats), _np(nf)
        assert np.array_equal(n, np.minimum(1 + _np(b.lengths) // 160, feats.shape[2]))
        rows.extend(f[j, :, :n[j]].T.copy() for j in range(len(n)))
    assert len(rows) == 24 and all(len(r) == 1 + lengths[i] // 160 for i, r in enumerate(rows))
    inits, fitted = [], []
    for cls, m in ((0, be.bona), (1, be.spoof)):
        x = np.concatenate([r for r, lab in zip(rows, labels) if lab == cls])
        inits.append(go.init_from_data(x, 4, seed=cls, reg_covar=REG))
        m.set_params(*inits[-1])
        fitted.append((x, go.fit(x, *inits[-1], reg_covar=REG, max_iter=3, tol=1e-3)))
    be.fit(walk, max_iter=3, tol=1e-3)
    for m, (x, o) in zip((be.bona, be.spoof), fitted):
        assert (m.n_iter_, m.converged_) == (o["n_iter"], o["converged"])
    # the LLR: each model's row mean carries its lse bound, and the three EM steps a parameter drift of at most the
    # recorded 60-feature allowance of the fit test (2.4e-9 relative), which moves a logit by at most 3 delta times
    # the logit's magnitude sum (mu p, p and c_k each move by delta)
    want = go.llr(rows, *[(o["w"], o["mu"], o["var"]) for _, o in fitted])
    tol = np.zeros(len(rows))
    for _, o in fitted:
        p = (o["w"], o["mu"], o["var"])
        for i, r in enumerate(rows):
            mag = go.logit_bound(r, *p).max(axis=1) / ((2 * 60 + 3) * go.U)
            tol[i] += go.BOTH * go.lse_bound(r, *p).mean() + 3 * 2.4e-9 * mag.mean()
    got = torch.cat([be.score(b.pcm, b.lengths) for b in walk()])
    assert got.dtype == torch.float32 and got.shape == (24,)
    err = np.abs(_np(got).astype(np.float64) - want)
    print("LLR max err", err.max(), "allowance", tol.min(), "LLR range", want.min(), want.max())
    assert np.all(err <= tol + 2.0 ** -24 * np.abs(want))  # (+ the fp32 rounding of the returned score)
    # evaluate: the device chain's EER equals the host function on its own scores
    res = be.evaluate(walk)
    assert np.array_equal(_np(res.labels), labels) and torch.equal(res.scores, got)
    assert res.eer == eval_metrics.eer_both_polarities(_np(res.scores), labels) and res.min_tdcf is None
    assert res.eer < 0.5
    # the score file
    names = ["LA_E_%07d" % i for i in range(24)]
    lab_t = torch.from_numpy(labels)
    loader = [(b.pcm, names[8 * k:8 * k + 8], None, lab_t[8 * k:8 * k + 8], None, b.lengths) for k, b in enumerate(walk())]
    host_scores = _np(got).tolist()
    for sync in ("end", "batch"):
        path = str(tmp_path / ("scores_%s.txt" % sync))
        assert test_on_dataset_gmm(be, loader, path, task="19eval", keep_dataset_labels=True, sync=sync) == 24
        assert open(path).read() == "".join(format_score_line(n, v, "spoof" if lab else "bonafide")
                                            for n, v, lab in zip(names, host_scores, labels))
    path = str(tmp_path / "scores_21.txt")
    assert test_on_dataset_gmm(be, [(b[0], b[1], b[5]) for b in loader], path, task="21LA") == 24  # (pcm, names, lengths)
    assert open(path).read() == "".join(format_score_line(n, v) for n, v in zip(names, host_scores))
    # fusion beside a network's scores (a stand-in vector: the fusion reads fp32 (K, N) device scores)
    other = _dev(np.random.default_rng(0).normal(size=24).astype(np.float32) - labels.astype(np.float32))
    fused = score_fusion.fuse_device(torch.stack([res.scores, other]), res.labels, "avg")
    assert fused.scores.shape == (24,) and fused.system_eers[0][0] == eval_metrics.compute_eer(
        _np(res.scores)[labels == 0].astype(np.float64), _np(res.scores)[labels == 1].astype(np.float64))[0]
