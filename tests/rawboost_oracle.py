"""Test infrastructure (numpy only): RawBoost as include/air_hip.h ("RawBoost") specifies it, restated in float64, with
the error bound of the device arithmetic carried beside every value.

Nothing here imports the package or scipy.  tests/test_rawboost_cpu.py holds ``band`` / ``notch`` / ``centred_fir`` to
scipy.signal (firwin, convolve, freqz, lfilter); tests/test_rawboost_gpu.py holds the kernels to the stage functions, fed
with the device's own taps and the Philox words of tests/philox_oracle.py.

Bounds.  u = 2^-24 (fp32 unit roundoff), u64 = 2^-53.  Every stage function returns ``(value, err)``: the float64
reference and an array with |device - reference| <= err, derived as follows and never tuned to an observed error.

* Design (``design_bound``).  A band filter of c taps: three sinc terms (argument product, sin, quotient, coefficient:
  <= 4 roundings + the sine's error each), the window (<= 4 + the cosine's), their product and the division by a sum of c
  terms - every tap is off by at most (c + 16 + 4 D) u64 of the filter's scale ||h||_1 >= 1, D the error of a device
  transcendental in ulp (0 on the host).  The cascade is a product of polynomials: a tap of b collects every band's
  error times the other bands' l1 norms, plus a sum of at most len(b) products per convolution - together at most
  (sum_j (c_j + 16 + 4 D) + len) u64 prod_j ||h_j||_1 =: e_b per tap.  |H| is a sum of len taps, so max|H| (>= |H(0)| =
  |sum b| = 1) moves by at most len e_b + (len + 2) u64 ||b||_1, and the gain by that fraction; 10^(G/20) adds (1 + D)
  u64.  Per tap of the scaled cascade, generously: (len + 2) (sum_j (c_j + 16 + 4 D) + len + 4 + D) u64 prod_j ||h_j||_1
  gain.  D: the HIP documentation ("HIP math API", double-precision functions: sinpi, cospi, sincospi, pow) lists these
  at 1 - 2 ulp; D = 2.  The figure is six orders below the fp32 rounding of the taps (u |b|) it is added to.
* FIR (``fir_bound``).  One fmaf chain over ``terms`` products, each operand exact: (terms + 2) u sum |b| |p| (the
  standard recursive-summation bound, gamma_n <= (n + 2) u for n u < 0.01).  The powers are formed in fp32 exactly as the
  device forms them, so they carry no error.
* Mean, peak rule, ISD, SSI: one line each where they are computed below.
* Noise: the fp32 Box-Muller draw is within RANDN_ERR = 1.564e-6 of ``randn_ref`` (the bound tests/test_small_kernels_gpu.py
  holds air_randn to, four times its measured 3.91e-7); the kernel repeats air_randn's statements.
"""
import math

import numpy as np

import philox_oracle as po

FS = 16000
U = 2.0 ** -24
U64 = 2.0 ** -53
DEV_ULP = 2
RANDN_ERR = 4 * 3.91e-7

HDR, FILTERS, NF, MAXBANDS, MAXTAPS = 8, 6, 5, 8, 512
FREC = 2 + 3 * MAXBANDS
ROW = HDR + FILTERS * FREC  # 164 doubles per row
MAXL = 1 << 20
KEY_TAG = 0x5242 << 36  # "RB": the keys of the two streams are KEY_TAG | seed << 1 | {0 ISD, 1 SSI}

DEFAULTS = dict(nBands=5, minF=20.0, maxF=8000.0, minBW=100.0, maxBW=1000.0, minCoeff=10, maxCoeff=100, minG=0.0, maxG=0.0,
                minBiasLinNonLin=5.0, maxBiasLinNonLin=20.0, N_f=5, P=10.0, g_sd=2.0, SNRmin=10.0, SNRmax=40.0)

HAS_LNL, HAS_ISD, HAS_SSI = (0, 3, 4, 5, 7), (1, 3, 4, 6, 7), (2, 3, 5, 6)


# ------------------------------------------------------------------------------------------------------------ design
def band(fc, bw, c):
    """firwin(c, [f1, f2], window='hamming', fs=FS), restated: (c,) float64 of unit sum."""
    f1 = fc - bw / 2.0
    if f1 <= 0:
        f1 = 1.0 / 1000.0
    f2 = fc + bw / 2.0
    if f2 >= FS / 2:
        f2 = FS / 2 - 1.0 / 1000.0
    m = np.arange(c) - (c - 1) / 2.0
    l, r = f1 / (FS / 2), f2 / (FS / 2)
    win = np.ones(1) if c == 1 else 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(c) / (c - 1))
    h = (l * np.sinc(l * m) + np.sinc(m) - r * np.sinc(r * m)) * win
    return h / h.sum()


def notch(bands, G):
    """bands: [(fc, bw, c), ...] with c odd -> (b float64, info): the cascade scaled to 10^(G/20) / max|H(k pi / 512)|."""
    hs = [band(fc, bw, int(c)) for fc, bw, c in bands]
    b = hs[0]
    for h in hs[1:]:
        b = np.convolve(b, h)
    k = np.arange(512)[:, None] * np.arange(b.size)[None, :]
    H = (b[None, :] * np.exp(-1j * np.pi * (k % 1024) / 512.0)).sum(1)
    gain = 10.0 ** (G / 20.0) / np.abs(H).max()
    info = dict(cs=[int(c) for _, _, c in bands], l1=float(np.prod([np.abs(h).sum() for h in hs])), gain=float(gain))
    return b * gain, info


def design_bound(info, n_taps, dev_ulp=0):
    """Per-tap |b - b'| between two float64 evaluations of ``notch`` (module docstring, "Design")."""
    terms = sum(c + 16 + 4 * dev_ulp for c in info["cs"]) + n_taps + 4 + dev_ulp
    return (n_taps + 2) * terms * U64 * info["l1"] * info["gain"]


def centred_fir(b, v):
    """F(b, v)[n] = sum_k b[k] v[n + (len(b) + 1) // 2 - k], n in [0, len(v)), v zero outside: float64."""
    b, v = np.asarray(b, np.float64), np.asarray(v, np.float64)
    full = np.convolve(b, v)
    off = (b.size + 1) // 2
    out = np.zeros(v.size)
    n = max(0, min(v.size, full.size - off))
    out[:n] = full[off:off + n]
    return out


def fir_bound(b, p, terms):
    """(terms + 2) u sum_k |b[k]| |p[n + off - k]| (module docstring, "FIR")."""
    return (terms + 2) * U * centred_fir(np.abs(b), np.abs(p))


# ------------------------------------------------------------------------------------------------ the parameter table
def uniform(rng, a, b):
    return a + (b - a) * rng.random()


def draw_bands(rng, cfg):
    out = []
    for _ in range(cfg["nBands"]):
        fc = uniform(rng, cfg["minF"], cfg["maxF"])
        bw = uniform(rng, cfg["minBW"], cfg["maxBW"])
        c = int(uniform(rng, cfg["minCoeff"], cfg["maxCoeff"]))
        out.append((fc, bw, c + 1 if c % 2 == 0 else c))
    return out


def put_filter(row, slot, bands, G):
    rec = row[HDR + slot * FREC: HDR + (slot + 1) * FREC]
    rec[0], rec[1] = G, len(bands)
    for k, (fc, bw, c) in enumerate(bands):
        rec[2 + 3 * k: 5 + 3 * k] = (fc, bw, c)


def get_filter(row, slot):
    rec = row[HDR + slot * FREC: HDR + (slot + 1) * FREC]
    return [tuple(rec[2 + 3 * k: 5 + 3 * k]) for k in range(int(rec[1]))], float(rec[0])


def draw_table(rng, algos, cfg, seed, isd_base, ssi_base):
    """The documented draw order of ``RawBoostAugment.params``, restated: rows in order; a row of algorithm a draws, for
    LnL, filter by filter (i = 0 .. N_f - 1) its bands (fc, bw, c each) and then G; for ISD, beta; for SSI the bands, G
    and the SNR.  Every draw is lo + (hi - lo) * rng.random().  -1 rows draw nothing."""
    t = np.zeros((len(algos), ROW))
    for b, a in enumerate(algos):
        row = t[b]
        row[0] = a
        row[3], row[4] = isd_base, ssi_base
        row[6], row[7] = KEY_TAG | (seed << 1), KEY_TAG | (seed << 1) | 1
        if a in HAS_LNL:
            for i in range(cfg["N_f"]):
                bands = draw_bands(rng, cfg)
                lo, hi = (cfg["minG"], cfg["maxG"]) if i == 0 else (
                    cfg["minG"] - cfg["minBiasLinNonLin"], cfg["maxG"] - cfg["maxBiasLinNonLin"])
                put_filter(row, i, bands, uniform(rng, lo, hi))
        if a in HAS_ISD:
            beta = uniform(rng, 0.0, cfg["P"])
            row[1] = math.floor(beta / 100.0 * 4294967296.0)
            row[2] = cfg["g_sd"]
        if a in HAS_SSI:
            bands = draw_bands(rng, cfg)
            put_filter(row, NF, bands, uniform(rng, cfg["minG"], cfg["maxG"]))
            row[5] = uniform(rng, cfg["SNRmin"], cfg["SNRmax"])
    return t


def counter_ranges(table, B):
    """[ISD lo, hi), [SSI lo, hi) a call with this table reserves (every row carries the call's bases)."""
    return (int(table[0, 3]), int(table[0, 3]) + B * MAXL), (int(table[0, 4]), int(table[0, 4]) + B * (MAXL // 4))


# ------------------------------------------------------------------------------------------------------------ stages
def to_f32(x):
    """A row as the kernels read it: fp32, or int16 as s / 32768 (exact)."""
    x = np.asarray(x)
    return (x.astype(np.float32) / np.float32(32768.0)) if x.dtype == np.int16 else x.astype(np.float32)


def n0(y, err, lo=None, hi=None):
    """Peak rule on a reference y whose device counterpart is within err.  The device divides (one fp32 rounding) by its
    own peak, which lies within E = max(err) of the reference's: |y'/pk' - y/pk| <= err/pk' + |y| E / (pk pk') + u |y/pk|
    with pk' >= pk - E.  A peak within E of 1 could flip the branch: refused (the tests keep peaks away from 1)."""
    pk, E = float(np.abs(y).max()), float(np.max(err))
    if pk > 1.0:
        assert pk - E > 1.0, "the peak %.9g is within the error %.3g of 1" % (pk, E)
        v = y / pk
        return v, err / (pk - E) + np.abs(y) * E / (pk * (pk - E)) + U * (np.abs(v) + err / (pk - E)), pk
    assert pk + E <= 1.0, "the peak %.9g is within the error %.3g of 1" % (pk, E)
    return y.copy(), np.array(err, dtype=np.float64) + np.zeros_like(y), pk


def lnl_raw(x32, taps):
    """sum_i F(b_i, p_{i+1}) with the device's fp32 taps (a list of 1-D float32 arrays, empty = unused slot)."""
    p = x32.copy()
    y, s, terms = np.zeros(x32.size), np.zeros(x32.size), 0
    for i, b in enumerate(taps):
        if i:
            p = (p * x32).astype(np.float32)  # p_{j+1} = fl32(p_j x)
        if b.size:
            y += centred_fir(b, p)
            s += centred_fir(np.abs(b.astype(np.float64)), np.abs(p.astype(np.float64)))
            terms += b.size
    return y, (terms + 2) * U * s


def lnl(x32, taps):
    """The LnL stage: (value, err, peak before the rule)."""
    y, e = lnl_raw(x32, taps)
    # mean: an fp64 sum of the device's values (error <= mean(e), the fp64 summation is below u64 L |y|), rounded to
    # fp32 (u |mu|); the subtraction is one fp32 rounding of a result within e + dmu of the reference
    mu = y.mean()
    dmu = e.mean() + U * abs(mu) + U64 * y.size * np.abs(y).mean()
    c = y - mu
    ec = e + dmu
    ec = ec + U * (np.abs(c) + ec)
    return n0(c, ec)


def isd(v, e_in, b, Lcap, row):
    """The ISD stage on a reference input v (device input within e_in): (value, err, peak, selected mask).
    Selected: out = v + (g v) (a d), a = fl32(2 u1 - 1), d likewise, every operation one rounding: the product g v a d
    carries <= 5 roundings (a, d, a d, g v, the product), the sum one more; linear in v, so e_in passes with |1 + g a d|."""
    L = v.size
    ctr = int(row[3]) + b * Lcap + np.arange(L, dtype=np.uint64)
    w = po.philox4x32_10(ctr & np.uint64(po.MASK32), ctr >> np.uint64(32), int(row[6]))
    sel = w[:, 0].astype(np.uint64) < np.uint64(int(row[1]))
    u1 = (w[:, 1].astype(np.float32) * po.INV32).astype(np.float64)
    u2 = (w[:, 2].astype(np.float32) * po.INV32).astype(np.float64)
    g = float(np.float32(row[2]))
    r = (2.0 * u1 - 1.0) * (2.0 * u2 - 1.0)
    t = np.where(sel, g * v * r, 0.0)
    out = v + t
    e = np.where(sel, e_in * (1.0 + g * np.abs(r)) + 5.05 * U * np.abs(t) + U * (np.abs(out) + e_in * (1.0 + g * np.abs(r))), e_in)
    val, err, pk = n0(out, e)
    return val, err, pk, sel


def ssi_noise(b, Lcap, L, row):
    """The row's noise: element j of air_randn(seed = key, offset = ssi_base + b ceil(Lcap / 4)), float64."""
    return po.randn_ref(L, int(row[7]), int(row[4]) + b * ((Lcap + 3) // 4), 1.0)


def ssi(v, e_in, b, Lcap, row, taps):
    """The SSI stage: (value, err).  q' = the device's chain over its own fp32 noise: |q' - q| <= F(|b|, RANDN_ERR) +
    (len + 2) u F(|b|, |n| + RANDN_ERR) =: eq.  Norms (fp64 on the device): | ||q'|| - ||q|| | <= ||eq||, likewise for v.
    s' = fl32(||v'|| / (||q'|| 10^(SNR/20))): relative error rho <= ||e_in|| / ||v|| + ||eq|| / (||q|| - ||eq||) + u +
    8 u64.  y' = fmaf(q', s', v'): |y' - y| <= e_in + eq s (1 + rho) + |q| s rho (1 + rho)... + u |y|."""
    L = v.size
    if not taps.size:
        return v.copy(), e_in + np.zeros(L)
    n = ssi_noise(b, Lcap, L, row)
    bb = np.abs(taps.astype(np.float64))
    q = centred_fir(taps, n)
    eq = centred_fir(bb, np.full(L, RANDN_ERR)) + (taps.size + 2) * U * centred_fir(bb, np.abs(n) + RANDN_ERR)
    nq, nv, neq, nev = np.linalg.norm(q), np.linalg.norm(v), np.linalg.norm(eq), np.linalg.norm(e_in + np.zeros(L))
    if nq == 0.0:
        return v.copy(), e_in + np.zeros(L)
    assert nq > 2 * neq
    s = nv / (nq * 10.0 ** (row[5] / 20.0))
    rho = (nev / nv if nv > 0 else 0.0) + neq / (nq - neq) + U + 8 * U64
    ds = s * rho * (1.0 + rho) + (nev / (nq * 10.0 ** (row[5] / 20.0)) if nv == 0 else 0.0)
    y = v + q * s
    e = e_in + eq * (s + ds) + np.abs(q) * ds
    return y, e + U * (np.abs(y) + e)


def row_reference(x, b, Lcap, row, taps):
    """Row b end to end.  x: the row's own samples (fp32 or int16); taps: the device's six cascades (float32 arrays).
    Returns dict(y, err, peaks=[(reference peak, error at the peak's rule) ...], sel)."""
    x32 = to_f32(x)
    a = int(row[0])
    v, e, sel, peaks = x32.astype(np.float64), np.zeros(x32.size), None, []
    if a < 0 or a > 7:
        return dict(y=v, err=e, peaks=peaks, sel=sel)
    if a == 7:
        v1, e1, p1 = lnl(x32, taps[:NF])
        v2, e2, p2, sel = isd(v, e, b, Lcap, row)
        s = v1 + v2
        es = e1 + e2
        es = es + U * (np.abs(s) + es)
        y, err, p3 = n0(s, es)
        return dict(y=y, err=err, peaks=[p1, p2, p3], sel=sel)
    if a in HAS_LNL:
        v, e, pk = lnl(x32, taps[:NF])
        peaks.append(pk)
    if a in HAS_ISD:
        v, e, pk, sel = isd(v, e, b, Lcap, row)
        peaks.append(pk)
    if a in HAS_SSI:
        v, e = ssi(v, e, b, Lcap, row, taps[NF])
    return dict(y=v, err=e, peaks=peaks, sel=sel)
