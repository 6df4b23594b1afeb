"""CPU: the oracle of the fp32 BatchNorm (tests/bn_edges_oracle.py) against fp64 F.batch_norm and its autograd, and numpy
emulations, written from the kernels' text, of the two routes to the statistics:

* bn_partial_stats_kernel + bn_finalize_kernel: x - K in fp32, lane-strided quads in fp32, a flush to fp64 per image,
  a fixed order over the splits, the tail in fp64 and the fp32 roundings of the outputs;
* records {n, K_i, sum(y - K_i), sum((y - K_i)^2)} of at most 192 values, merged as bn_finalize_records_kernel does
  (the records model the size of a convolution epilogue's, not the tile order in which it fills them).

With the shift both stay inside every bound the GPU test uses.  WITHOUT it (K = 0, or records of plain sums and sums
of squares) the variance bound is violated on classes 1 and 2 at every shape with N > 1: that is asserted, and is the
proof that tests/test_bn_edges_gpu.py would notice a kernel that lost its shift."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_edges_oracle as bo

F32 = np.float32
NT = 256
FLAT_S = 32


def T64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


# ---- the oracle against torch fp64 -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s in bo.SHAPES if s != (1, 8, 1, 1)])  # (F.batch_norm refuses N = 1 in training)
def test_oracle_is_batch_norm_and_its_autograd(shape):
    d = bo.case(shape)
    st = bo.stats(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], keep=1.0 - float(F32(bo.MOMENTUM)))  # (torch's fp64 weight)
    rm, rv = T64(d["rm"]).clone(), T64(d["rv"]).clone()
    for relu in (False, True):
        x = T64(d["x"]).requires_grad_(True)
        ga, be = T64(d["gamma"]).requires_grad_(True), T64(d["beta"]).requires_grad_(True)
        y = F.batch_norm(x, rm if not relu else None, rv if not relu else None, ga, be, True,
                         float(F32(bo.MOMENTUM)), float(F32(bo.EPS)))
        out = F.relu(y) if relu else y
        out.backward(T64(d["dy"]))
        a = bo.apply(d["x"], st["scale"], st["shift"], relu)
        # fp64 against fp64: a thousandth of what the fp32 kernel is allowed
        assert bo.worst(bo.ratios(a["y"], out.detach().numpy(), a["y_bound"])) <= 1e-3
        b = bo.bwd(d["x"], d["dy"], st["mean"], st["invstd"], d["gamma"], d["beta"], mask=(a["pre"] > 0) if relu else None)
        assert bo.worst(bo.ratios(b["dbeta"], be.grad.numpy(), b["dbeta_bound"], 0)) <= 1e-3
        assert bo.worst(bo.ratios(b["dgamma"], ga.grad.numpy(), b["dgamma_bound"], 0)) <= 1e-3
        assert bo.worst(bo.ratios(b["dx"], x.grad.numpy(), b["dx_bound"])) <= 1e-3, relu
    assert bo.worst(bo.ratios(st["running_mean"], rm.numpy(), st["running_mean_bound"], 0)) <= 1e-3
    assert bo.worst(bo.ratios(st["running_var"], rv.numpy(), st["running_var_bound"], 0)) <= 1e-3
    xd = T64(d["x"])
    ax = (0, 2, 3)
    assert bo.worst(bo.ratios(st["mean"], xd.mean(ax).numpy(), st["mean_bound"], 0)) <= 1e-3
    assert bo.worst(bo.ratios(st["var"], xd.var(ax, unbiased=False).numpy(), st["var_bound"], 0)) <= 1e-3


def test_exact_classes_of_the_oracle():
    for shape in bo.SHAPES:
        d = bo.case(shape)
        st = bo.stats(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"])
        m, v, _ = bo.exact_alternating(shape)
        for c in range(shape[1]):
            if c % 8 == 3:
                assert st["mean"][c] == 3.25 and st["var"][c] == 0.0
            if c % 8 == 7:
                assert abs(st["mean"][c] - m) <= 1e-15 and abs(st["var"][c] - v) <= 1e-15
        if shape == (1, 8, 1, 1):
            assert (st["var"] == 0).all() and (st["var_scale"] == 0).all()


# ---- the kernels' summation, in numpy --------------------------------------------------------------------------
def splits_for(B, C):
    return min(max(2048 // C, 1), B)


def _plane_sums(v, h, peel):
    """One (b, c) plane of bn_partial_stats_kernel: fp32 sums of v and v^2 per thread (v = x - K, already fp32)."""
    S = v.shape[0]
    s1, s2 = np.zeros(NT, F32), np.zeros(NT, F32)
    nq = (S - h) >> 2
    q = v[h:h + 4 * nq].reshape(nq, 4)
    q1 = (q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3])
    p = q * q
    q2 = (p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])
    for i in range(0, nq, NT):
        n = min(NT, nq - i)
        s1[:n] = s1[:n] + q1[i:i + n]
        s2[:n] = s2[:n] + q2[i:i + n]
    if peel:
        for e in list(range(h)) + list(range(h + 4 * nq, S)):
            s1[NT - 1] = s1[NT - 1] + v[e]
            s2[NT - 1] = s2[NT - 1] + v[e] * v[e]
    elif S & 2:
        s1[NT - 1] = s1[NT - 1] + (v[S - 2] + v[S - 1])
        s2[NT - 1] = s2[NT - 1] + (v[S - 2] * v[S - 2] + v[S - 1] * v[S - 1])
    return s1, s2


def emulate_stats(d, shifted=True, momentum=bo.MOMENTUM):
    """bn_partial_stats(_flat)_kernel + bn_finalize_kernel on the case ``d``.  Returns the kernel's outputs (float32)
    and the variance the finalize kernel holds in fp64."""
    x = d["x"]
    B, C, S = bo._bcs(x)
    x = x.reshape(B, C, S)
    N = float(B * S)
    nsplit = splits_for(B, C)
    per = -(-B // nsplit)
    out = {k: np.zeros(C, F32) for k in ("mean", "invstd", "scale", "shift", "running_mean", "running_var")}
    out["var"] = np.zeros(C)
    eps, mom = F32(bo.EPS), F32(momentum)
    for c in range(C):
        K = x[0, c, 0] if shifted else F32(0)
        t1 = t2 = 0.0
        for split in range(nsplit):  # the ordered fold over the splits
            d1, d2 = np.zeros(NT), np.zeros(NT)
            for b in range(split * per, min(B, split * per + per)):
                v = x[b, c] - K
                if S < FLAT_S:  # flat kernel: every element and every square, rounded to fp32, goes to fp64 at once
                    d1[0] += v.astype(np.float64).sum()
                    d2[0] += (v * v).astype(np.float64).sum()
                    continue
                peel = bool(S & 1)
                h = ((b * C + c) * S) & 1 if peel else 0
                s1, s2 = _plane_sums(v, h, peel)
                d1 += s1
                d2 += s2
            t1 += d1.sum()
            t2 += d2.sum()
        ms = t1 / N
        var = max(t2 / N - ms * ms, 0.0)
        m = ms + float(K)
        mf = F32(m)
        is_ = F32(1.0 / np.sqrt(var + float(eps)))
        sc = F32(d["gamma"][c]) * is_
        unbiased = var * N / (N - 1.0) if N > 1.0 else var
        out["var"][c], out["mean"][c], out["invstd"][c], out["scale"][c] = var, mf, is_, sc
        out["shift"][c] = F32(d["beta"][c]) - mf * sc
        out["running_mean"][c] = (F32(1) - mom) * F32(d["rm"][c]) + mom * mf
        out["running_var"][c] = (F32(1) - mom) * F32(d["rv"][c]) + mom * F32(unbiased)
    return out


def _tree16(v):
    for o in (8, 4, 2, 1):
        v = v + v[..., np.arange(16) ^ o]
    return v[..., 0]


def emulate_records(d, shifted=True):
    """A model of the record SIZE, not of the convolution epilogue's order: a record here is 192 consecutive values of the
    flattened channel (16 lanes x 12 values: each lane sums its values in turn, the lanes meet in a tree), where the
    Winograd epilogue's record is a tile group's outputs.  What is the kernel's is the arithmetic: fp32 sums of at most
    192 shifted values with the record's own K, and the fp64 merge of bn_finalize_records_kernel.  shifted=False: the
    records hold plain sums and sums of squares and are merged as such."""
    x = d["x"]
    B, C, S = bo._bcs(x)
    N = B * S
    xc = np.moveaxis(x.reshape(B, C, S), 1, 0).reshape(C, N)
    G = -(-N // 192)
    out = {"var": np.zeros(C), "mean": np.zeros(C, F32), "invstd": np.zeros(C, F32), "K": np.zeros(C)}
    for c in range(C):
        n_, K_, s1_, s2_ = [], [], [], []
        for g in range(G):
            v = xc[c, g * 192:(g + 1) * 192]
            K = v[0] if shifted else F32(0)
            dd = np.zeros(192, F32)
            dd[:v.size] = v - K  # (positions outside the tensor contribute an exact 0, as the kernel's masks do)
            dd = dd.reshape(12, 16)
            s1, s2 = np.zeros(16, F32), np.zeros(16, F32)
            for j in range(12):
                s1 = s1 + dd[j]
                s2 = (dd[j].astype(np.float64) * dd[j].astype(np.float64) + s2.astype(np.float64)).astype(F32)  # fmaf
            n_.append(float(v.size)), K_.append(float(K)), s1_.append(float(_tree16(s1))), s2_.append(float(_tree16(s2)))
        if shifted:
            K0 = K_[0]
            A = Q = 0.0
            for ni, Ki, s1, s2 in zip(n_, K_, s1_, s2_):
                dlt = Ki + s1 / ni - K0
                A += ni * dlt
                Q += (s2 - s1 * s1 / ni) + ni * dlt * dlt
            ms = A / N
            var = max(Q / N - ms * ms, 0.0)
            m = ms + K0
        else:
            m = sum(s1_) / N
            var = max(sum(s2_) / N - m * m, 0.0)
            K0 = 0.0
        out["K"][c], out["var"][c], out["mean"][c] = K0, var, F32(m)
        out["invstd"][c] = F32(1.0 / np.sqrt(var + float(F32(bo.EPS))))
    return out


def _held(name, shape, got, want, bound, record):
    rs = bo.ratios(got, want, bound, 0)
    print(bo.fmt("%s %s" % (name, shape), rs))
    record[name] = max(record.get(name, 0.0), bo.worst(rs))
    return rs


def test_shifted_emulation_is_within_every_bound_and_the_unshifted_one_is_not():
    record = {}
    for shape in bo.SHAPES:
        d = bo.case(shape)
        st = bo.stats(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"])
        e = emulate_stats(d)
        assert np.array_equal(st["K"], d["x"].reshape(shape[0], shape[1], -1)[0, :, 0].astype(np.float64))
        rs_var = _held("variance", shape, e["var"], st["var"], st["var_bound"], record)
        for k in ("mean", "invstd", "running_mean", "running_var"):
            _held(k, shape, e[k], st[k], st[k + "_bound"], record)
        co = bo.coeffs(e["mean"], e["invstd"], d["gamma"], d["beta"])
        _held("scale", shape, e["scale"], co["scale"], co["scale_bound"], record)
        _held("shift", shape, e["shift"], co["shift"], co["shift_bound"], record)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel4 = [abs(e["var"][c] - st["var"][c]) / st["var"][c] for c in range(shape[1]) if c % 8 == 4 and st["var"][c] > 0]
        if rel4:
            print("class 4 (outlier shift) %s: variance off by %.3g relative, %.3g of its bound" % (shape, max(rel4), rs_var[4]))
        # exact classes
        m7, _, unb7 = bo.exact_alternating(shape)
        e1 = emulate_stats(d, momentum=1.0)  # momentum 1: the running statistics ARE the mean and the unbiased variance
        for c in range(shape[1]):
            if c % 8 == 3:
                assert e["mean"][c] == F32(3.25) and e["invstd"][c] == bo.invstd_of_zero_variance()
            if c % 8 == 7:
                assert e["mean"][c] == F32(m7) and e1["running_mean"][c] == F32(m7) and e1["running_var"][c] == F32(unb7)
        if shape == (1, 8, 1, 1):
            assert (e["var"] == 0).all()
            assert np.array_equal(e["running_var"], (F32(1) - F32(bo.MOMENTUM)) * d["rv"])
        # the same sums without the shift
        z = emulate_stats(d, shifted=False)
        rz = bo.ratios(z["var"], st["var"], st["var_bound"], 0)
        print(bo.fmt("variance, K = 0 %s" % (shape,), rz))
        if st["N"] > 1:
            assert rz[1] > 1.0 and rz[2] > 1.0, (shape, rz)
            rel = np.abs(z["var"] - st["var"]) / np.maximum(st["var"], 1e-300)
            print("   unshifted variance off by %.3g (class 1) and %.3g (class 2) of the variance" % (rel[1], rel[2]))
    for k, v in record.items():
        print("emulation / bound  %-14s %.4f" % (k, v))
    bad = {k: v for k, v in record.items() if not v <= 1.0}
    assert not bad, bad


def test_record_merge_is_within_the_bounds_and_plain_sums_are_not():
    record = {}
    for shape in bo.SHAPES:
        d = bo.case(shape)
        e = emulate_records(d)
        st = bo.stats(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], K=e["K"])
        _held("records variance", shape, e["var"], st["var"], st["var_bound"], record)
        _held("records mean", shape, e["mean"], st["mean"], st["mean_bound"], record)
        _held("records invstd", shape, e["invstd"], st["invstd"], st["invstd_bound"], record)
        for c in range(shape[1]):
            if c % 8 == 3:
                assert e["mean"][c] == F32(3.25) and e["invstd"][c] == bo.invstd_of_zero_variance()
        z = emulate_records(d, shifted=False)
        rz = bo.ratios(z["var"], st["var"], st["var_bound"], 0)
        print(bo.fmt("records of plain sums, variance %s" % (shape,), rz))
        if st["N"] > 1:
            assert rz[1] > 1.0 and rz[2] > 1.0, (shape, rz)
    for k, v in record.items():
        print("emulation / bound  %-18s %.4f" % (k, v))
    bad = {k: v for k, v in record.items() if not v <= 1.0}
    assert not bad, bad


# ---- the mask test of the GPU module has something to decide ---------------------------------------------------
def test_elements_near_zero_exist_and_are_few():
    """Elements whose fp64 |y| is below the apply bound are the only ones whose ReLU mask the rounding of x * scale +
    shift can decide.  Classes 1 and 2 of the layer-1 map must have some (or the GPU test that the backward masks
    exactly what the forward zeroed decides nothing) and no channel more than 2 % (or the masked sums are about the
    rounding, not the data).  N = 1 is exempt from the second: there xhat is exactly 0 and y = beta, which is below
    the bound of a channel whose x * scale is ~1e6 whatever the seed - the mask of that one element is then decided by
    the rounding alone, and the GPU test still demands that forward and backward decide alike."""
    for shape in bo.SHAPES:
        d = bo.case(shape)
        st = bo.stats(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"])
        a = bo.apply(d["x"], st["scale"].astype(F32), st["shift"].astype(F32), True)
        near = np.abs(a["pre"]) < a["y_bound"]
        cnt = np.moveaxis(near, 1, 0).reshape(shape[1], -1).sum(1)
        print("near-zero elements per channel %s: %s of %d" % (shape, cnt.tolist(), st["N"]))
        if st["N"] > 1:
            assert (cnt <= 0.02 * st["N"]).all(), (shape, cnt)
        if shape == bo.MODEL_SHAPE:
            assert all(cnt[c] > 0 for c in range(shape[1]) if c % 8 in (1, 2)), cnt
    for cfg in bo.CONV_DGRAD:
        d = bo.conv_dgrad_case(cfg)
        st = bo.stats(d["x"], d["gamma"], d["beta"], np.zeros(cfg[4]), np.ones(cfg[4]))
        a = bo.apply(d["x"], st["scale"].astype(F32), st["shift"].astype(F32), True)
        near = np.abs(a["pre"]) < a["y_bound"]
        cnt = np.moveaxis(near, 1, 0).reshape(cfg[4], -1).sum(1)
        assert (cnt <= 0.02 * st["N"]).all(), (cfg, cnt)
        if cfg[2:4] == (18, 75):
            assert all(cnt[c] > 0 for c in range(cfg[4]) if c % 8 in (1, 2)), cnt
