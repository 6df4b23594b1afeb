"""CPU: the host ports of the reference's t-DCF (eval_metrics.py:4-16, :49-193, evaluate_tDCF_asvspoof19.py) against
tests/golden/tdcf.npz, which tests/golden/make_golden_tdcf.py wrote from the reference itself.  Bit for bit: the
ports do the reference's fp64 operations in its order."""
import numpy as np
import pytest

from asvspoof2021_air_amd import eval_metrics as em


@pytest.fixture(scope="module")
def g(golden):
    return golden("tdcf.npz")


def cost_model(g):
    return {str(k): float(v) for k, v in zip(g["cost_names"], g["cost_values"])}


def rates(g):
    return tuple(g["asv_rates"])


def test_cost_model_is_the_reference_one(g):
    assert em.asvspoof19_cost_model() == cost_model(g)


def test_asv_error_rates_equal_the_reference(g):
    eer, thr = em.compute_eer(g["tar_asv"], g["non_asv"])
    assert eer == g["eer_asv"] and thr == g["asv_threshold"]
    got = em.obtain_asv_error_rates(g["tar_asv"], g["non_asv"], g["spoof_asv"], thr)
    assert np.array_equal(np.array(got, dtype=np.float64), g["asv_rates"])
    assert em.obtain_asv_error_rates(g["tar_asv"], g["non_asv"], np.array([]), thr)[2] is None


@pytest.mark.parametrize("tag, sign", [("pos", 1.0), ("neg", -1.0)])
def test_tdcf_curve_equals_the_reference(g, tag, sign):
    curve, thr = em.compute_tDCF(sign * g["bona_cm"], sign * g["spoof_cm"], *rates(g), cost_model(g), False)
    assert curve.dtype == np.float64 and curve.shape == (g["bona_cm"].size + g["spoof_cm"].size + 1,)
    assert np.array_equal(curve, g["curve_" + tag])
    assert np.array_equal(thr, g["thr_" + tag])
    k = int(np.argmin(curve))
    assert k == int(g["argmin_" + tag]) and curve[k] == g["min_" + tag]
    assert np.array_equal(np.array(em.compute_eer(sign * g["bona_cm"], sign * g["spoof_cm"])), g["eer_" + tag])


def write_scores(path, g, sign):
    """Score files in the layouts evaluate_tDCF_asvspoof19.py:21-32 reads; repr() round-trips the float64 values."""
    cm = path / "cm.txt"
    with open(cm, "w") as fh:
        for key, arr in (("bonafide", g["bona_cm"]), ("spoof", g["spoof_cm"])):
            for i, s in enumerate(arr):
                fh.write("LA_E_%s%05d A%02d %s %r\n" % (key[0], i, i % 19, key, float(sign * s)))
    asv = path / "asv.txt"
    with open(asv, "w") as fh:
        for key, arr in (("target", g["tar_asv"]), ("nontarget", g["non_asv"]), ("spoof", g["spoof_asv"])):
            for s in arr:
                fh.write("LA_0001 %s %r\n" % (key, float(s)))
    return str(cm), str(asv)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_eer_and_tdcf_of_score_files(g, tmp_path, sign):
    """The composition of the pinned pieces: the polarity with the lower EER gives the t-DCF
    (evaluate_tDCF_asvspoof19.py:53-67), whichever polarity the file was written in."""
    assert g["eer_pos"][0] < g["eer_neg"][0]
    cm, asv = write_scores(tmp_path, g, sign)
    eer, tdcf = em.compute_eer_and_tdcf(cm, asv)
    assert eer == g["eer_pos"][0]
    assert tdcf == g["min_pos"]


def test_error_paths(g):
    cmod, (pfa, pmiss, pms) = cost_model(g), rates(g)
    bona, spoof = g["bona_cm"], g["spoof_cm"]
    with pytest.raises(ValueError):  # priors that do not sum to one
        em.compute_tDCF(bona, spoof, pfa, pmiss, pms, dict(cmod, Ptar=0.5), False)
    with pytest.raises(ValueError):  # a negative prior
        em.compute_tDCF(bona, spoof, pfa, pmiss, pms, dict(cmod, Pnon=-0.01, Ptar=cmod["Ptar"] + cmod["Pnon"] + 0.01), False)
    with pytest.raises(ValueError):  # binary decisions
        em.compute_tDCF(np.array([1.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0]), pfa, pmiss, pms, cmod, False)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            em.compute_tDCF(np.append(bona, bad), spoof, pfa, pmiss, pms, cmod, False)
    with pytest.raises(ValueError):  # no spoof trials against the ASV system
        em.compute_tDCF(bona, spoof, pfa, pmiss, None, cmod, False)
    with pytest.raises(ValueError):  # ASV error rates that make a weight negative
        em.compute_tDCF(bona, spoof, 1.0, 1.0, pms, dict(cmod, Ptar=0.0, Pnon=0.95), False)
