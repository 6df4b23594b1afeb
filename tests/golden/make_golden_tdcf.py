#!/usr/bin/env python3
"""Golden fixture tdcf.npz from the REAL reference: the t-DCF of eval_metrics.py:4-16, :49-193 as
evaluate_tDCF_asvspoof19.py:10-67 drives it, on seeded scores.

About 2,000 countermeasure scores (bona fide N(1, 1), spoof N(-1, 1), every eighth rounded to one decimal so that
the curve has plateaus and the two classes tie) and about 3,000 ASV scores (target / nontarget / spoof), all exactly
representable in fp32.  Stored: the inputs, the ASV operating point and error rates, and for both polarities of the CM
scores the full normalised curve, its thresholds, the minimum and its index, and compute_eer's pair.

Build container only (needs the reference checkout beside the repository).  Usage: python tests/golden/make_golden_tdcf.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("AIR_REFERENCE", "/root/reference"))

import numpy as np

SEED = 2019


def main():
    import eval_metrics as ref_em  # noqa: E402
    rng = np.random.default_rng(SEED)

    def draw(n, mean):
        s = rng.normal(mean, 1.0, n).astype(np.float32)
        s[::8] = np.round(s[::8], 1)
        return s.astype(np.float64)

    bona_cm, spoof_cm = draw(611, 1.0), draw(1403, -1.0)
    tar_asv, non_asv, spoof_asv = draw(1009, 2.0), draw(997, -2.0), draw(1013, 0.5)
    cost_model = {"Pspoof": 0.05, "Ptar": (1 - 0.05) * 0.99, "Pnon": (1 - 0.05) * 0.01, "Cmiss_asv": 1, "Cfa_asv": 10,
                  "Cmiss_cm": 1, "Cfa_cm": 10}  # evaluate_tDCF_asvspoof19.py:10-19
    eer_asv, asv_threshold = ref_em.compute_eer(tar_asv, non_asv)
    Pfa_asv, Pmiss_asv, Pmiss_spoof_asv = ref_em.obtain_asv_error_rates(tar_asv, non_asv, spoof_asv, asv_threshold)
    out = dict(bona_cm=bona_cm, spoof_cm=spoof_cm, tar_asv=tar_asv, non_asv=non_asv, spoof_asv=spoof_asv,
               eer_asv=np.float64(eer_asv), asv_threshold=np.float64(asv_threshold),
               asv_rates=np.array([Pfa_asv, Pmiss_asv, Pmiss_spoof_asv], dtype=np.float64),
               cost_names=np.array(sorted(cost_model)), cost_values=np.array([cost_model[k] for k in sorted(cost_model)],
                                                                            dtype=np.float64))
    for tag, sign in (("pos", 1.0), ("neg", -1.0)):
        curve, thr = ref_em.compute_tDCF(sign * bona_cm, sign * spoof_cm, Pfa_asv, Pmiss_asv, Pmiss_spoof_asv, cost_model,
                                         False)
        k = int(np.argmin(curve))
        eer, eer_thr = ref_em.compute_eer(sign * bona_cm, sign * spoof_cm)
        out.update({"curve_" + tag: curve, "thr_" + tag: thr, "argmin_" + tag: np.int64(k), "min_" + tag: np.float64(curve[k]),
                    "eer_" + tag: np.array([eer, eer_thr], dtype=np.float64)})
    path = os.path.join(HERE, "tdcf.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
