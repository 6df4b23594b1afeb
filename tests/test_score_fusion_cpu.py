"""CPU: the port of the reference's score_fusion.py (asvspoof2021_air_amd/score_fusion.py) and the numpy oracle of its
arithmetic (tests/fusion_oracle.py) against what the reference itself returned, wrote and printed with pandas
(tests/golden/fusion.npz, tests/golden/make_golden_fusion.py).  Every comparison is on bits and bytes."""
import numpy as np
import pytest

import fusion_oracle as fo


@pytest.fixture(scope="module")
def g(golden):
    return golden("fusion.npz")


@pytest.fixture(scope="module")
def paths(g, tmp_path_factory):
    return fo.fixture_inputs(g, tmp_path_factory.mktemp("fusion_inputs"))


def parse(path):
    """The input's rows without the package: [(fname, sysid, key)] and the float32 scores, in file order."""
    rows = [ln.split() for ln in open(path)]
    return [tuple(r[:3]) for r in rows], np.array([float(r[3]) for r in rows], dtype=np.float64).astype(np.float32)


def joined(g, paths, method):
    """(scores (K, Lmax), index (K, N)) for the oracle: the recorded key order looked up in every input."""
    want_rows, _ = fo.fixture_rows(g, method)
    parsed = [parse(p) for p in paths]
    scores = np.zeros((len(paths), max(s.size for _, s in parsed)), dtype=np.float32)
    index = np.full((len(paths), len(want_rows)), -1, dtype=np.int32)
    for k, (rows, s) in enumerate(parsed):
        where = dict(zip(rows, range(len(rows))))
        assert len(where) == len(rows)
        scores[k, :s.size] = s
        index[k] = [where.get(r, -1) for r in want_rows]
    return scores, index


def test_fixture_holds_what_the_issue_asks(g, paths):
    rows, _ = fo.fixture_rows(g, "avg")
    assert 4000 < len(rows) < 4400 and {r[2] for r in rows} == {"bonafide", "spoof"}
    _, index = joined(g, paths, "avg")
    present = (index >= 0).sum(axis=0)
    assert (present == 1).sum() >= 4 and (present == 2).sum() >= 10 and present.min() == 1
    names = [r[0] for r in rows]
    assert len(set(names)) == len(names) - 1  # the one trial whose key disagrees between the files: two rows
    assert rows == sorted(rows)
    all3 = (index >= 0).all(axis=0)  # three different row orders
    ranks = [np.argsort(np.argsort(index[k][all3])) for k in range(3)]
    assert not any(np.array_equal(ranks[a], ranks[b]) for a, b in ((0, 1), (0, 2), (1, 2)))


def test_oracle_equals_the_fixture(g, paths):
    for method, mode in (("avg", "sum"), ("wght", "mean")):
        scores, index = joined(g, paths, method)
        weights = g["weights_distinct"].astype(np.float32) if method == "wght" else None
        got, count = fo.fuse(scores, index, weights, mode)
        assert fo.same_bits(got, g[method + "_bits"]), method
        assert count.min() >= 1 and count.max() == 3
        nan_row = [r[0] for r in fo.fixture_rows(g, method)[0]].index("ZZ_NAN_000")
        assert count[nan_row] == 2 and (index[:, nan_row] >= 0).all()  # present, NaN, not counted


def test_plain_float32_sum_is_not_the_arithmetic(g, paths):
    """The guard against "simplifying" the accumulation: on the cancellation rows neither a plain left-to-right float32
    sum nor an fp64 sum rounded once gives the recorded bits, the compensated float32 sum does."""
    scores, index = joined(g, paths, "avg")
    rows, want = fo.fixture_rows(g, "avg")
    pick = np.array([r[0].startswith("ZZ_CANCEL") for r in rows])
    assert pick.sum() == 48
    have = index >= 0
    vals = np.where(have, np.take_along_axis(scores, np.maximum(index, 0), axis=1), np.float32(0.0))
    plain = np.zeros(len(rows), dtype=np.float32)
    for k in range(3):
        plain = np.where(have[k], plain + vals[k], plain)
    assert plain.dtype == np.float32
    wide = np.where(have, vals.astype(np.float64), 0.0).sum(axis=0).astype(np.float32)
    assert (fo.bits(plain)[pick] != want[pick]).sum() >= 8
    assert (fo.bits(wide)[pick] != want[pick]).sum() >= 8
    assert fo.same_bits(fo.fuse(scores, index)[0][pick], want[pick])


@pytest.mark.parametrize("method", ["avg", "wght"])
def test_port_reproduces_the_reference(g, paths, tmp_path, method):
    from asvspoof2021_air_amd import score_fusion as sf
    out = str(tmp_path / method) + "/"
    if method == "avg":
        frame = sf.avg_fuse(paths, out)
    else:
        frame = sf.weighted_fuse(paths, g["eers"].tolist(), out)
    rows, want = fo.fixture_rows(g, method)
    assert frame.rows() == rows
    assert fo.same_bits(frame.score, want)
    assert open(out + "avg_fuse_score", "rb").read() == g[method + "_file"].tobytes()
    assert sf.fused_eer(frame.rows(), frame.score) == float(g[method + "_eer"]) == sf.fused_eer(frame.key, frame.score)
    assert fo.same_bits((sf.avg_fuse(paths) if method == "avg" else sf.weighted_fuse(paths, g["eers"].tolist())).score, want)


def test_cal_weight(g, tmp_path):
    from asvspoof2021_air_amd import score_fusion as sf
    for case in ("distinct", "two_equal", "all_equal", "k2", "k1"):
        eers = g["weights_%s_eers" % case].tolist()
        assert sf.cal_weight(eers) == g["weights_" + case].tolist(), case
    assert sf.cal_weight([0.25]) == [0.25] and sf.cal_weight([0.2, 0.2]) == [0.2, 0.2]
    assert abs(sum(sf.cal_weight([0.3, 0.1, 0.2])) - 1.0) < 1e-12
    for bad in ([], [0.1, float("nan")]):
        with pytest.raises(ValueError):
            sf.cal_weight(bad)
    table = tmp_path / "model_eers"
    table.write_text("sysA 0.228\nsysB 0.237\nother 0.5\nsysC 0.197\n")
    names = ["/x/%s" % n for n in g["names"].tolist()]
    assert sf.cal_weight_from_file(names, str(table)) == g["weights_distinct"].tolist()


def test_read_file_layouts(tmp_path):
    from asvspoof2021_air_amd import score_fusion as sf
    four, three, bad, nan = (tmp_path / n for n in ("four.txt", "three.txt", "bad.txt", "nan.txt"))
    four.write_text("LA_D_1 A01 spoof -2.9228995\nLA_D_2 - bonafide 0.9985754489898682\n\n")
    three.write_text("LA_D_1 -2.9228995 spoof\nLA_D_2 0.9985754489898682 bonafide\n")
    a, b = sf.read_file(str(four)), sf.read_file(str(three))
    assert a.rows() == [("LA_D_1", "A01", "spoof"), ("LA_D_2", "-", "bonafide")]
    assert b.rows() == [("LA_D_1", "-", "spoof"), ("LA_D_2", "-", "bonafide")]
    assert a.score.dtype == np.float32 and np.array_equal(a.score, b.score)
    assert np.array_equal(a.score, np.array([-2.9228995, 0.9985754489898682], dtype=np.float32))
    bad.write_text("LA_D_1 A01 spoof 1.0\nLA_D_2 bonafide\n")
    with pytest.raises(ValueError, match=r"bad\.txt:2"):
        sf.read_file(str(bad))
    nan.write_text("LA_D_1 A01 spoof 1.0\nLA_D_2 - bonafide 1.0\nLA_D_3 - bonafide one\n")
    with pytest.raises(ValueError, match=r"nan\.txt:3"):
        sf.read_file(str(nan))


def test_align_keeps_disagreeing_keys_apart():
    from asvspoof2021_air_amd import score_fusion as sf
    a = sf.ScoreFrame(["u2", "u1", "u3"], ["-", "A01", "-"], ["bonafide", "spoof", "bonafide"], [2.0, 1.0, 3.0])
    b = sf.ScoreFrame(["u1", "u2", "u4"], ["A01", "-", "A02"], ["spoof", "spoof", "other"], [10.0, 20.0, 40.0])
    matrix, index, keys, labels = sf.align([a, b])
    assert keys == [("u1", "A01", "spoof"), ("u2", "-", "bonafide"), ("u2", "-", "spoof"), ("u3", "-", "bonafide"),
                    ("u4", "A02", "other")]
    assert index.dtype == np.int32 and index.tolist() == [[1, 0, -1, 2, -1], [0, -1, 1, -1, 2]]
    assert matrix.dtype == np.float32 and matrix.tolist() == [[1.0, 2.0, 0.0, 3.0, 0.0], [10.0, 0.0, 20.0, 0.0, 40.0]]
    assert labels.tolist() == [1, 0, 1, 0, -1]
    assert sf.avg_fuse([a, b]).score.tolist() == [11.0, 2.0, 20.0, 3.0, 40.0]
    want, _ = fo.fuse(matrix, np.where(index >= 0, np.arange(5), -1), np.array([0.2, 0.2], dtype=np.float32), "mean")
    assert fo.same_bits(sf.weighted_fuse([a, b], [0.2, 0.2]).score, fo.bits(want))  # (equal EERs: the weights are the EERs)
    with pytest.raises(ValueError):
        sf.align([a, sf.ScoreFrame(["u1", "u1"], ["-", "-"], ["spoof", "spoof"], [1.0, 2.0])])
    with pytest.raises(ValueError):
        sf.weighted_fuse([a, b], [0.2])


def test_write_fused_text(tmp_path):
    from asvspoof2021_air_amd import score_fusion as sf
    p = tmp_path / "out.txt"
    sf.write_fused(str(p), [("a", "-", "bonafide"), ("b", "A01", "spoof"), ("c", "-", "spoof"), ("d", "-", "spoof")],
                   np.array([-2.9228995, 1e-5, np.inf, np.nan], dtype=np.float32))
    assert p.read_text() == "a - bonafide -2.9228995\nb A01 spoof 1e-05\nc - spoof inf\nd - spoof \n"
