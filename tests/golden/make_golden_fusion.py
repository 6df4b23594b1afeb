#!/usr/bin/env python3
"""Golden fixture fusion.npz from the REAL reference: score_fusion.py's avg_fuse / weighted_fuse / cal_weight (pandas)
on every 6th trial of the three ``19dev`` score files the reference ships (scores/lfcc_ecapa512c{f,t}s{t,f}_ocs_19dev_score.txt).

The shipped files have three columns ``fname score key``; the reference's reader wants four, ``fname sysid key score``,
so the generator writes K = 3 four-column inputs (sysid ``-``; the score text is kept as shipped) and makes them awkward:

  - three different row orders (as shipped, reversed, a seeded permutation);
  - trials absent from one file, trials present in one file only;
  - one trial whose key disagrees between the files (two rows in the result);
  - N_CANCEL appended ``ZZ_CANCEL_*`` trials whose scores have mixed sign and widely different magnitude (a third of them
    in two files only), so that the order and the compensation of the float32 sum show in the result: half of them are
    big, small, nearly -big (an fp64 sum rounded once differs), half are drawn until a plain and a compensated float32
    sum of the row differ; the generator asserts that, on these rows, a plain float32 sum, an fp64 sum rounded once and
    pandas' result do not all agree (and prints how many rows each candidate matches);
  - one trial with ``inf`` in one file and one with ``nan`` in one file (pandas skips the NaN and does not count it).

Stored: the three input files' bytes and their names; per method (``avg``, ``wght``) the returned frame (fname, sysid, key
in its order, the float32 scores as raw bits), the bytes of the file the reference wrote and the EER its main block prints;
the weights weighted_fuse used; cal_weight's result for the EER lists [three distinct], [two equal and one different],
[all equal], [K = 2], [K = 1].  cal_weight opens a hard-coded path: ``open`` is patched inside this generator only.

Build container only (needs the reference checkout beside the repository and pandas).
Usage: python tests/golden/make_golden_fusion.py
"""
import argparse
import io
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("AIR_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

import numpy as np

SEED = 2021
STRIDE = 6
N_CANCEL = 48
SHIPPED = ["lfcc_ecapa512cfst_ocs_19dev_score.txt", "lfcc_ecapa512ctsf_ocs_19dev_score.txt",
           "lfcc_ecapa512ctst_ocs_19dev_score.txt"]
NAMES = ["sysA_score.txt", "sysB_score.txt", "sysC_score.txt"]  # cal_weight matches "sysA" ... as substrings of the path
EERS = [0.228, 0.237, 0.197]
WEIGHT_CASES = {"distinct": [0.228, 0.237, 0.197], "two_equal": [0.21, 0.21, 0.35], "all_equal": [0.2, 0.2, 0.2],
                "k2": [0.3, 0.1], "k1": [0.25]}


def f32_text(x):
    return repr(float(np.float32(x)))


def plain_sum(vals):
    acc = np.float32(0.0)
    for v in vals:
        acc = np.float32(acc + v)
    return acc


def compensated_sum(vals):
    """The float32 sum tests/fusion_oracle.py states."""
    acc = c = np.float32(0.0)
    for v in vals:
        y = np.float32(v - c)
        t = np.float32(acc + y)
        c = np.float32(np.float32(t - acc) - y)
        acc = t
    return acc


def build_inputs():
    """Three lists of rows (fname, sysid, key, score text)."""
    rng = np.random.default_rng(SEED)
    shipped = []
    for f in SHIPPED:
        rows = [ln.split() for ln in open(os.path.join(REF, "scores", f)) if ln.strip()]
        shipped.append({r[0]: (r[1], r[2]) for r in rows})
        if len(shipped) == 1:
            order = [r[0] for r in rows][::STRIDE]
    files = [[(n, "-", s[n][1], s[n][0]) for n in order if n in s] for s in shipped]
    names = [r[0] for r in files[0]]
    pick = rng.permutation(len(names))
    gone_b = set(names[i] for i in pick[:5])           # absent from file B
    gone_c = set(names[i] for i in pick[5:12])         # absent from file C
    only_a = set(names[i] for i in pick[12:16])        # in file A only
    only_c = set(names[i] for i in pick[16:18])        # in file C only
    flip = names[pick[18]]                             # key disagrees in file B
    files[0] = [r for r in files[0] if r[0] not in only_c]
    files[1] = [r for r in files[1] if r[0] not in gone_b | only_a | only_c]
    files[2] = [r for r in files[2] if r[0] not in gone_c | only_a]
    files[1] = [(r[0], r[1], ("spoof" if r[2] == "bonafide" else "bonafide") if r[0] == flip else r[2], r[3]) for r in files[1]]
    for i in range(N_CANCEL):
        absent = i % 9 // 3 if i % 3 == 2 else None  # a third of them: two addends
        while True:
            small = np.float32(rng.normal() * 10.0 ** rng.uniform(-4, 1))
            if i % 4 < 2:  # big, small, nearly -big: what is left is the small one and the difference
                big = np.float32(rng.normal() * 10.0 ** rng.uniform(3, 8))
                near = np.float32(-big * np.float32(1.0 + rng.normal() * 2e-6))
                vals = [big, small, near] if i % 2 else [small, big, near]
                break
            # one large and two smaller ones: the low bits the second loses to the first come back with the third -
            # drawn again until a plain and a compensated float32 sum of the row differ (rows of three addends)
            big = np.float32(small * 10.0 ** rng.uniform(0.5, 4))
            other = np.float32(rng.normal() * 10.0 ** rng.uniform(-4, 1))
            vals = [big, small, other] if i % 2 else [big, -other, small]
            if absent is not None or plain_sum(vals) != compensated_sum(vals):
                break
        row = lambda v: ("ZZ_CANCEL_%03d" % i, "A%02d" % (7 + i % 13), "spoof" if i % 3 else "bonafide", f32_text(v))
        for k in range(3):
            if k == absent:
                continue
            files[k].append(row(vals[k]))
    files[0].append(("ZZ_INF_000", "A19", "spoof", "-inf"))
    files[1].append(("ZZ_INF_000", "A19", "spoof", "-1.5"))
    files[2].append(("ZZ_INF_000", "A19", "spoof", "2.25"))
    files[0].append(("ZZ_NAN_000", "-", "bonafide", "3.5"))
    files[1].append(("ZZ_NAN_000", "-", "bonafide", "nan"))
    files[2].append(("ZZ_NAN_000", "-", "bonafide", "0.1"))
    files[1] = files[1][::-1]
    files[2] = [files[2][i] for i in rng.permutation(len(files[2]))]
    return files


def main_block_eer(em, frame):
    """score_fusion.py:111-120."""
    target_scores = frame[frame["key"] == "bonafide"]["score"]
    nontarget_scores = frame[frame["key"] == "spoof"]["score"]
    eer = em.compute_eer(target_scores, nontarget_scores)[0]
    other_eer = em.compute_eer(-target_scores, -nontarget_scores)[0]
    return min(eer, other_eer)


def main():
    import eval_metrics as ref_em
    import score_fusion as ref

    state = {"text": ""}
    real_open = open

    def fake_open(path, *a, **kw):  # cal_weight's hard-coded path only
        if path == "/data/xinhui/scores/model_eers":
            return io.StringIO(state["text"])
        return real_open(path, *a, **kw)

    ref.open = fake_open
    files = build_inputs()
    out = {"names": np.array(NAMES), "eers": np.array(EERS, dtype=np.float64)}
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for name, rows in zip(NAMES, files):
            text = "".join("%s %s %s %s\n" % r for r in rows)
            paths.append(os.path.join(tmp, name))
            with real_open(paths[-1], "w") as fh:
                fh.write(text)
            out["input_" + name[:4]] = np.frombuffer(text.encode(), dtype=np.uint8)
        for case, eers in WEIGHT_CASES.items():
            state["text"] = "".join("sys%s %r\n" % ("ABC"[i], e) for i, e in enumerate(eers))
            w = ref.cal_weight(argparse.Namespace(input=paths[:len(eers)]))
            out["weights_" + case] = np.array(w, dtype=np.float64)
            out["weights_" + case + "_eers"] = np.array(eers, dtype=np.float64)
        state["text"] = "".join("sys%s %r\n" % ("ABC"[i], e) for i, e in enumerate(EERS))
        for method, fn in (("avg", ref.avg_fuse), ("wght", ref.weighted_fuse)):
            odir = os.path.join(tmp, method) + os.sep
            os.makedirs(odir)
            frame = fn(argparse.Namespace(input=paths, output=odir))
            assert frame["score"].dtype == np.float32
            out[method + "_fname"] = frame["fname"].to_numpy().astype(str)
            out[method + "_sysid"] = frame["sysid"].to_numpy().astype(str)
            out[method + "_key"] = frame["key"].to_numpy().astype(str)
            out[method + "_bits"] = frame["score"].to_numpy().view(np.uint32).copy()
            out[method + "_file"] = np.frombuffer(real_open(odir + "avg_fuse_score", "rb").read(), dtype=np.uint8)
            out[method + "_eer"] = np.float64(main_block_eer(ref_em, frame))
    # the cancellation rows must tell the candidate arithmetics apart
    table = [{(r[0], r[1], r[2]): np.float32(float(r[3])) for r in rows} for rows in files]
    plain = fp64 = both = comp = 0
    for (fn_, sy, ke), bits in zip(zip(out["avg_fname"], out["avg_sysid"], out["avg_key"]), out["avg_bits"]):
        if not fn_.startswith("ZZ_CANCEL"):
            continue
        vals = [t[(fn_, sy, ke)] for t in table if (fn_, sy, ke) in t]
        got = np.array([bits], dtype=np.uint32).view(np.float32)[0]
        p = plain_sum(vals)
        d = np.float32(np.sum(np.array(vals, dtype=np.float64)))
        comp += int(compensated_sum(vals) == got)
        plain += int(p == got)
        fp64 += int(d == got)
        both += int(p == got and d == got)
    print("cancellation rows: %d; plain float32 agrees on %d, fp64-then-round on %d, both on %d, compensated float32 on %d"
          % (N_CANCEL, plain, fp64, both, comp))
    assert plain < N_CANCEL and fp64 < N_CANCEL and both < N_CANCEL
    path = os.path.join(HERE, "fusion.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%.1f KB); avg EER %.6f %%, wght EER %.6f %%" % (path, os.path.getsize(path) / 1024,
                                                                      100 * out["avg_eer"], 100 * out["wght_eer"]))
    assert os.path.getsize(path) <= 781392


if __name__ == "__main__":
    main()
