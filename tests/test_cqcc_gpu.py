"""The CQCC front-end on the GPU (csrc/cqcc.hip through feature_extraction.CQCC) against the numpy fp64 oracle of
tests/cqcc_oracle.py, and its conformance as a front-end: layouts, ragged rows, replay, the GMM back-end.

The bounds are the oracle's (``power_bounds`` / ``cqcc_bounds``): derived from fp32 roundoff along the kernels' sums,
never from what the kernels return."""
import functools

import numpy as np
import pytest
import torch

import cqcc_oracle as co
from oracle.filler import fill_module_, synth_pcm

pytestmark = pytest.mark.gpu

RAGGED = [1, 159, 160, 161, 4001, 16000]  # one frame, the frame-count edge, shorter than every atom / the lowest atoms


def _fe(n_octaves=9, **kw):
    from asvspoof2021_air_amd.feature_extraction import CQCC
    return CQCC(n_octaves=n_octaves, **kw)


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _ragged_batch(dtype="f32"):
    """(6, 16000) rows of noise plus tones, NaN (fp32) / full scale (int16) behind each row's own samples: reading
    past a row's length poisons what is compared."""
    x = torch.from_numpy(co.make_signal(len(RAGGED), 16000, 31))
    if dtype == "i16":
        x = (x * 32767).round().to(torch.int16)
    for b, n in enumerate(RAGGED):
        x[b, n:] = float("nan") if dtype == "f32" else 32767
    return x.cuda(), torch.tensor(RAGGED, dtype=torch.int32).cuda()


# ---------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("n_octaves", [2, 3, 9])
def test_spectrum_matches_the_oracle(n_octaves):
    ref = co.reference(n_octaves)
    fe = _fe(n_octaves)
    S = _np(fe.forward_spectrum(torch.from_numpy(ref["x"]).cuda())).astype(np.float64)
    assert S.shape == ref["S"].shape and np.isfinite(S).all()
    err = np.abs(np.exp(S) - ref["P"])
    print("n_octaves %d: max |exp(S) - P| / bound = %.3g, max relative error %.3g, median bound / P %.3g" % (
        n_octaves, (err / ref["tolP"]).max(), (err / ref["P"]).max(), np.median(ref["tolP"] / ref["P"])))
    assert np.all(err <= ref["tolP"])


@pytest.mark.parametrize("n_octaves", [2, 3, 9])
def test_forward_matches_the_oracle(n_octaves):
    ref = co.reference(n_octaves)
    fe = _fe(n_octaves)
    out = _np(fe(torch.from_numpy(ref["x"]).cuda())).astype(np.float64)
    assert out.shape == ref["feats"].shape == (ref["x"].shape[0], 1 + ref["x"].shape[1] // 160, 60)
    err = np.abs(out - ref["feats"])
    print("n_octaves %d: max error / bound = %.3g; max error static %.3g delta %.3g delta-delta %.3g; max bound %.3g" % (
        n_octaves, (err / ref["bounds"]).max(), err[..., :20].max(), err[..., 20:40].max(), err[..., 40:].max(),
        ref["bounds"].max()))
    assert np.all(err <= ref["bounds"])


def test_other_hop_and_coefficient_count_match_the_oracle():
    x = co.make_signal(1, 3001, 41, n_octaves=3)
    fe = _fe(3, hop=128, n_coef=12, d=8)
    out = _np(fe(torch.from_numpy(x).cuda()))[0].astype(np.float64)
    X, R, G, E = co.transform(x[0].astype(np.float64), 3, hop=128, with_envelope=True)
    tolP = co.power_bounds(X, R, G, E)
    proj = co.projection(3, n_coef=12, d=8)
    S = co.log_power(X)
    assert (tolP / np.exp(S)).max() < 0.5
    want = co.cqcc(x[0].astype(np.float64), 3, hop=128, n_coef=12, d=8)
    assert out.shape == want.shape == (1 + 3001 // 128, 36)
    assert np.all(np.abs(out - want) <= co.cqcc_bounds(S, tolP, proj))


# ---------------------------------------------------------------------------- bits
def test_int16_equals_fp32_on_the_scaled_samples():
    x16, ln = _ragged_batch("i16")
    fe = _fe()
    xf = x16.float() / 32768.0
    assert torch.equal(fe.forward_ragged(x16, ln, 101), fe.forward_ragged(xf, ln, 101))
    assert torch.equal(fe(x16[5:]), fe(xf[5:]))
    assert torch.equal(fe.forward_spectrum(x16[4:, :4001]), fe.forward_spectrum(xf[4:, :4001]))


@pytest.mark.parametrize("n_octaves", [3, 9])
def test_each_ragged_row_equals_the_dense_call_on_it_alone(n_octaves):
    x, ln = _ragged_batch()
    fe = _fe(n_octaves)
    got = fe.forward_ragged(x, ln, 101, padding="zero")
    spec = fe.forward_spectrum(x, ln)
    assert not torch.isnan(got).any() and not torch.isnan(spec).any()
    for b, n in enumerate(RAGGED):
        row = x[b:b + 1, :n].contiguous()
        assert torch.equal(got[b:b + 1], fe.forward_padded(row, 101, padding="zero")), n
        T = 1 + n // 160
        assert torch.equal(got[b, :, :T].t(), fe(row)[0]), n
        assert torch.equal(spec[b, :T], fe.forward_spectrum(row)[0]) and not spec[b, T:].any(), n


def test_ragged_rows_follow_the_oracle_where_atoms_outrun_the_row():
    """Rows shorter than every atom (160, 161 samples), shorter than the lowest atoms only (4001), and the full row:
    101 frames, i.e. the second 64-frame tile of every decimated level against the oracle."""
    x, ln = _ragged_batch()
    fe = _fe()
    spec = _np(fe.forward_spectrum(x, ln)).astype(np.float64)
    for b in (2, 3, 4, 5):
        n = RAGGED[b]
        X, R, G, E = co.transform(_np(x[b, :n]).astype(np.float64), with_envelope=True)
        err = np.abs(np.exp(spec[b, :1 + n // 160]) - (np.abs(X) ** 2 + co.EPS))
        assert np.all(err <= co.power_bounds(X, R, G, E)), n


def test_a_second_call_repeats_the_bits():
    x, ln = _ragged_batch()
    fe = _fe()
    a = fe.forward_ragged(x, ln, 64).clone()
    s = fe.forward_spectrum(x[5:]).clone()
    torch.zeros(1 << 22, device="cuda").add_(1.0)  # other work in between
    assert torch.equal(a, fe.forward_ragged(x, ln, 64)) and torch.equal(s, fe.forward_spectrum(x[5:]))
    assert torch.equal(a, _fe().forward_ragged(x, ln, 64))  # and so does a second plan


# ---------------------------------------------------------------------------- layouts
def _pad_chop(feat, feat_len, start, mode):
    """dataset.py:62-79 on one (T, D) array -> (D, feat_len)."""
    T = feat.shape[0]
    if T >= feat_len:
        st = min(max(start, 0), T - feat_len)
        out = feat[st:st + feat_len]
    elif mode == "repeat":
        out = np.tile(feat, (feat_len // T + 1, 1))[:feat_len]
    else:
        out = np.concatenate([feat, np.zeros((feat_len - T, feat.shape[1]), feat.dtype)])
    return out.T


@pytest.mark.parametrize("mode", ["repeat", "zero"])
def test_padded_layout_is_pad_or_chop_of_the_frames(mode):
    x = torch.from_numpy(co.make_signal(3, 4000, 51, n_octaves=3)).cuda()  # T = 26
    fe = _fe(3)
    frames = _np(fe(x))
    for feat_len, starts in ((10, [0, 7, 999]), (26, [3, 0, 0]), (61, [0, 5, -4])):  # chop; exact; pad
        st = torch.tensor(starts, dtype=torch.int32).cuda()
        got = _np(fe.forward_padded(x, feat_len, st, mode))
        assert got.shape == (3, 60, feat_len)
        for b in range(3):
            assert np.array_equal(got[b], _pad_chop(frames[b], feat_len, starts[b], mode)), (feat_len, b)
    assert np.array_equal(_np(fe.forward_padded(x, 10, None, mode))[1], _pad_chop(frames[1], 10, 0, mode))
    ln = torch.tensor([4000, 1700, 161], dtype=torch.int32).cuda()  # T = 26, 11, 2 in one batch: chop, pad, pad
    st = torch.tensor([9, 4, 1], dtype=torch.int32).cuda()
    got = _np(fe.forward_ragged(x, ln, 16, st, mode))
    for b, n in enumerate([4000, 1700, 161]):
        own = _np(fe(x[b:b + 1, :n].contiguous()))[0]
        assert np.array_equal(got[b], _pad_chop(own, 16, [9, 4, 1][b], mode)), n


def test_silence_padding_is_refused():
    x = torch.zeros(1, 800).cuda()
    fe = _fe(2)
    with pytest.raises(ValueError, match="silence"):
        fe.forward_padded(x, 8, padding="silence")
    with pytest.raises(ValueError, match="silence"):
        fe.forward_ragged(x, [800], 8, padding="silence")
    # and the C entry point itself says AIR_EUNSUPPORTED
    from asvspoof2021_air_amd import _hip
    lib = _hip.lib()
    out = torch.empty(1, 60, 8).cuda()
    ws = torch.empty(lib.air_cqcc_ws_bytes(1, 800, 2, 160, 20), dtype=torch.uint8).cuda()
    rc = lib.air_cqcc_fwd_ragged(_hip.dptr(x), None, 1, 800, None, _hip.dptr(out), 8, None,
                                 _hip.dptr(fe.plan(x.device), torch.uint8), 2, 160, 20, 2,
                                 _hip.dptr(ws, torch.uint8), _hip.csz(ws.numel()), _hip.stream())
    assert rc == -2
    rc = lib.air_cqcc_fwd_ragged(_hip.dptr(x), None, 1, 800, None, _hip.dptr(out), 8, None,
                                 _hip.dptr(fe.plan(x.device), torch.uint8), 2, 160, 20, 0,
                                 _hip.dptr(ws, torch.uint8), _hip.csz(16), _hip.stream())
    assert rc == -4  # a workspace smaller than air_cqcc_ws_bytes says


# ---------------------------------------------------------------------------- consumers
def test_trainer_steps_replay_bit_for_bit_on_cqcc():
    """Trainer(model, frontend=CQCC()) unchanged: four steps (two eager, the capture, one replay) under enable_graph
    equal four eager steps bit for bit."""
    from asvspoof2021_air_amd.resnet import ResNet
    from asvspoof2021_air_amd.train import Trainer
    pcm = synth_pcm(2, 8000, seed=883).cuda()
    labels = torch.tensor([1, 0]).cuda()
    runs = []
    for graph in (False, True):
        model = fill_module_(ResNet(3, 256, resnet_type="18", nclasses=2))
        model.set_attention_noise(None)
        tr = Trainer(model, add_loss=None, frontend=_fe(), feat_len=64)
        if graph:
            tr.enable_graph(True)
        losses = [float(tr.step(pcm, labels)[0]) for _ in range(4)]
        torch.cuda.synchronize()
        if graph:
            assert tr._graph is not None and "CQCC" in tr._graph["key"]
        runs.append((losses, tr.model.arena().flat.clone()))
    assert all(np.isfinite(runs[0][0])) and runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(tr.features(pcm)[:, 0], tr.lfcc.forward_padded(pcm, 64))


def test_gmm_backend_fits_and_scores_on_cqcc():
    from asvspoof2021_air_amd import GMMBackend
    pcm = torch.from_numpy(co.make_signal(4, 8000, 61)).cuda()
    labels = torch.tensor([0, 1, 0, 1])
    be = GMMBackend(n_components=4, frontend=_fe())
    be.fit([(pcm, labels)], max_iter=3)
    llr = be.score(pcm)
    ragged = be.score(pcm, torch.tensor([8000, 8000, 3000, 500], dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    assert llr.shape == (4,) and torch.isfinite(llr).all() and torch.isfinite(ragged).all()
