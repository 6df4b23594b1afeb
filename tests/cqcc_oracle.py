"""The CQCC front-end's definition (include/air_hip.h, "CQCC front-end") restated in numpy fp64, step by step, and
the fp32 error bounds the GPU tests hold the kernels to.  Written from the definition: all that the bounds know of
the kernels is that every sum is ONE chain of fp32 fused multiply-adds in index order (which is what an fp32 MFMA
accumulates: a k-ordered fmaf chain), never how the work is tiled.

Shapes: a row is a 1-D float64 array of samples (int16 PCM: ``s / 32768``)."""
import math

import numpy as np

SR, BPO, N_OCT, HOP, N_COEF, D_LIN = 16000, 96, 9, 160, 20, 16
EPS = 2.0 ** -52
FIR_J, FIR_BETA = 47, 16.0
U32 = 2.0 ** -24  # fp32 unit roundoff


# ---- derived quantities ------------------------------------------------------------------------------------------
def n_bins(n_octaves=N_OCT, bpo=BPO):
    return bpo * n_octaves


def q_factor(bpo=BPO):
    return 1.0 / (2.0 ** (1.0 / bpo) - 1.0)


def bin_freqs(sr=SR, n_octaves=N_OCT, bpo=BPO):
    fmin = (sr / 2.0) / 2.0 ** n_octaves
    return fmin * 2.0 ** (np.arange(bpo * n_octaves) / bpo)


def octave_of(k, n_octaves=N_OCT, bpo=BPO):
    return n_octaves - 1 - k // bpo


def level_of(o):
    return 0 if o < 2 else o - 1


def n_lin(n_octaves=N_OCT, bpo=BPO, d=D_LIN):
    K = bpo * n_octaves
    return 1 + int(math.floor(d * (2.0 ** ((K - 1) / bpo) - 1.0)))


# ---- 1. pyramid ----------------------------------------------------------------------------------------------------
def fir():
    half = (FIR_J - 1) // 2
    m = np.arange(FIR_J) - half
    h = 0.5 * np.sinc(m / 2.0) * np.kaiser(FIR_J, FIR_BETA)
    return h / h.sum()


def fir_response(freqs_in_R):
    """|H| at the given frequencies (in units of the level's rate R)."""
    h = fir()
    n = np.arange(FIR_J)
    return np.abs(np.exp(-2j * np.pi * np.outer(freqs_in_R, n)) @ h)


def decimate(x, h=None):
    """x_{s+1}[n] = sum_j h[j] x_s[2 n + j - (J-1)/2], n < ceil(L_s / 2), zeros outside the row."""
    h = fir() if h is None else h
    half = (len(h) - 1) // 2
    Lo = (len(x) + 1) // 2
    xp = np.concatenate([np.zeros(half), x, np.zeros(half + 2)])
    idx = 2 * np.arange(Lo)[:, None] + np.arange(len(h))[None, :]  # into xp: (2 n + j - half) + half
    return xp[idx] @ h


def pyramid(x, n_levels, h=None):
    """[level 0, ..., level n_levels]."""
    out = [np.asarray(x, dtype=np.float64)]
    for _ in range(n_levels):
        out.append(decimate(out[-1], h))
    return out


def pyramid_error(x, n_levels):
    """[e_0 = 0, e_1, ...]: per-sample bounds (first order) on an fp32 pyramid whose taps are rounded once and whose
    sums are fmaf chains in tap order: e_{s+1}[n] = sum_j |h[j]| e_s[.] + u (sum_i |partial sum i| + sum_j |h[j] x_s[.]|)."""
    h = fir()
    half = (FIR_J - 1) // 2
    levels = pyramid(x, n_levels)
    out = [np.zeros(len(levels[0]))]
    for s in range(n_levels):
        xs = levels[s]
        Lo = (len(xs) + 1) // 2
        xp = np.concatenate([np.zeros(half), xs, np.zeros(half + 2)])
        idx = 2 * np.arange(Lo)[:, None] + np.arange(FIR_J)[None, :]
        prod = xp[idx] * h[None, :]
        own = U32 * (np.abs(np.cumsum(prod, axis=1)).sum(axis=1) + np.abs(prod).sum(axis=1))
        out.append(decimate(out[-1], np.abs(h)) + own)
    return out


# ---- 2. atoms --------------------------------------------------------------------------------------------------------
def atom_lengths(ratio, bpo=BPO):
    """N of the bpo bins of an octave whose lowest bin has R / f = ratio (4: the top octave, 8: every other)."""
    Q = q_factor(bpo)
    return np.array([2 * int(math.floor(Q * (ratio * 2.0 ** (-j / bpo)) / 2.0)) + 1 for j in range(bpo)])


def atom_table(ratio, bpo=BPO):
    """(2 H + 1, bpo) complex: column j is bin j's atom w[n] / sum w * exp(-2 pi i (f/R) m) at offsets m = -H .. H."""
    N = atom_lengths(ratio, bpo)
    H = int(N.max() // 2)
    tab = np.zeros((2 * H + 1, bpo), dtype=np.complex128)
    for j in range(bpo):
        w = np.hanning(N[j])
        m = np.arange(N[j]) - N[j] // 2
        fr = 2.0 ** (j / bpo) / ratio
        tab[H + m, j] = w / w.sum() * np.exp(-2j * np.pi * fr * m)
    return tab, H


def frame_count(L, hop=HOP):
    return 1 + L // hop


def _frames(level, centres, H):
    xp = np.concatenate([np.zeros(H), level, np.zeros(H + 1)])
    return xp[np.asarray(centres)[:, None] + np.arange(2 * H + 1)[None, :]]  # [t, m + H] = level[c_t + m]


def transform(x, n_octaves=N_OCT, hop=HOP, bpo=BPO, with_envelope=False, frames=None):
    """X (T, K) complex (``frames``: those frame indices only).  with_envelope: also what the error bound of ``power_bounds`` is made of -
    R (T, K) = sum_i |s_i|, s_i the partial sums of X's defining sum taken in index order n = 0 .. N - 1;
    G (T, K) = sum_n w[n] / sum w * |x_s[c + n - (N-1)/2]|;
    E (T, K) = sum_n w[n] / sum w * e_s[c + n - (N-1)/2], e_s the level's own error bound (``pyramid_error``)."""
    x = np.asarray(x, dtype=np.float64)
    t = np.arange(frame_count(len(x), hop)) if frames is None else np.asarray(frames)
    T, K = len(t), bpo * n_octaves
    n_levels = max(0, n_octaves - 2)
    levels = pyramid(x, n_levels)
    X = np.zeros((T, K), dtype=np.complex128)
    if with_envelope:
        err = pyramid_error(x, n_levels)
        G, R, E = np.zeros((T, K)), np.zeros((T, K)), np.zeros((T, K))
    for o in range(n_octaves):
        s = level_of(o)
        ratio = 4.0 if o == 0 else 8.0
        tab, H = atom_table(ratio, bpo)
        centres = (t * hop) >> s
        k0 = (n_octaves - 1 - o) * bpo
        F = _frames(levels[s], centres, H)
        X[:, k0:k0 + bpo] = F @ tab
        if with_envelope:
            G[:, k0:k0 + bpo] = np.abs(F) @ np.abs(tab)
            E[:, k0:k0 + bpo] = _frames(err[s], centres, H) @ np.abs(tab)
            for j0 in range(0, bpo, 16):  # (T, 2 H + 1, 16) products at a time
                part = np.cumsum(F[:, :, None] * tab[None, :, j0:j0 + 16], axis=1)
                R[:, k0 + j0:k0 + j0 + 16] = np.abs(part).sum(axis=1)
    return (X, R, G, E) if with_envelope else X


# ---- 4. log power ----------------------------------------------------------------------------------------------------
def log_power(X, eps=EPS):
    return np.log(np.abs(X) ** 2 + eps)


# ---- 5. uniform resampling and DCT -----------------------------------------------------------------------------------
def interp_matrix(n_octaves=N_OCT, bpo=BPO, d=D_LIN):
    """(M, K): row m reads S by linear interpolation in k at bpo * log2(g_m / fmin), g_m = fmin (1 + m / d)."""
    K, M = bpo * n_octaves, n_lin(n_octaves, bpo, d)
    pos = bpo * np.log2(1.0 + np.arange(M) / d)
    k0 = np.minimum(np.floor(pos).astype(int), K - 1)
    fr = pos - k0
    W = np.zeros((M, K))
    W[np.arange(M), k0] += 1.0 - fr
    ok = k0 + 1 < K
    W[np.arange(M)[ok], k0[ok] + 1] += fr[ok]
    return W


def dct_matrix(M, n_coef=N_COEF):
    """Orthonormal DCT-II, the first n_coef rows: (n_coef, M)."""
    q = np.arange(n_coef)[:, None]
    m = np.arange(M)[None, :]
    C = np.sqrt(2.0 / M) * np.cos(np.pi * (m + 0.5) * q / M)
    C[0] *= math.sqrt(0.5)
    return C


def projection(n_octaves=N_OCT, n_coef=N_COEF, bpo=BPO, d=D_LIN):
    """The fused (n_coef, K) matrix."""
    W = interp_matrix(n_octaves, bpo, d)
    return dct_matrix(W.shape[0], n_coef) @ W


# ---- 6. deltas -------------------------------------------------------------------------------------------------------
def delta(c):
    """(T, n): x[t + 1] - x[t - 1] with the edge frames repeated."""
    cp = np.concatenate([c[:1], c, c[-1:]], axis=0)
    return cp[2:] - cp[:-2]


def cqcc(x, n_octaves=N_OCT, hop=HOP, n_coef=N_COEF, bpo=BPO, d=D_LIN, eps=EPS):
    """(T, 3 n_coef): [static, delta, delta-delta]."""
    S = log_power(transform(x, n_octaves, hop, bpo), eps)
    c = S @ projection(n_octaves, n_coef, bpo, d).T
    dl = delta(c)
    return np.concatenate([c, dl, delta(dl)], axis=1)


# ---- fp32 error bounds -----------------------------------------------------------------------------------------------
def power_bounds(X, R, G, E, eps=EPS):
    """Bound on |exp(S_fp32) - exp(S)| per element, for an fp32 evaluation of steps 1 - 4 whose sums are fmaf chains
    in index order.

    X's real and imaginary parts are chains s_i = fl(s_{i-1} + a_i x_i): each link rounds the partial sum once, so
    the chain is off by at most u sum_i |s_i| = u R to first order (the table's zero rows change nothing).  Rounding
    the table once costs u per term, u G in all, and the samples of level s are themselves off by e_s, E in all;
    both hit real and imaginary part alike, hence sqrt(2).
    delta = 2 (u R + sqrt(2) (u G + E)), the factor 2 covering what first order leaves out.  Then |X|^2 moves
    by at most 2 |X| delta + delta^2; squaring, adding, eps and an fp32 logarithm accurate to 2 ulp of S (read back
    through exp) add the relative term r."""
    dlt = 2.0 * (U32 * R + math.sqrt(2.0) * (U32 * G + E))
    P = np.abs(X) ** 2
    S = np.log(P + eps)
    r = U32 * (8.0 + 4.0 * np.abs(S))
    move = 2.0 * np.abs(X) * dlt + dlt ** 2
    return move + (P + eps + move) * r


def cqcc_bounds(S, tolP, proj):
    """Bound on the 60 columns: tolP through the logarithm (exactly: -log1p(-tolP / exp(S)), which needs tolP below
    the power itself - the floor the test asserts), through the projection's |P| row by row plus its own roundoff
    ((K + 2) u sum |P S|), through the two differences."""
    rel = tolP / np.exp(S)
    assert rel.max() < 1.0
    dS = -np.log1p(-rel)
    K = S.shape[1]
    bs = dS @ np.abs(proj).T + (K + 2) * U32 * (np.abs(S) @ np.abs(proj).T)

    def dbound(b, val):
        bp = np.concatenate([b[:1], b, b[-1:]], axis=0)
        return bp[2:] + bp[:-2] + U32 * np.abs(val)
    c = S @ proj.T
    d1 = delta(c)
    bd = dbound(bs, d1)
    bdd = dbound(bd, delta(d1))
    return np.concatenate([bs, bd, bdd], axis=1)


def make_signal(B, L, seed, sigma=0.1, n_octaves=N_OCT):
    """White noise plus a few tones at bin centres, (B, L) float32 inside (-1, 1)."""
    rng = np.random.RandomState(seed)
    f = bin_freqs(SR, n_octaves)
    n = np.arange(L)
    x = sigma * rng.randn(B, L)
    for b in range(B):
        for k in rng.choice(len(f), 4, replace=False):
            x[b] += 0.1 * np.cos(2 * np.pi * f[k] * n / SR + rng.uniform(0, 2 * np.pi))
    return np.clip(x, -0.99, 0.99).astype(np.float32)


# ---- the cases the CPU and GPU tests share ---------------------------------------------------------------------------
# n_octaves -> (rows, samples, seed): 2 = the top octave with one sibling, 3 = the first decimated level, 9 = every
# level.  10 403 samples are 66 frames, two more than a 64-frame tile holds, and no multiple of anything.  The seeds are
# ones whose smallest |X|^2 stays above the floor ``reference`` asserts (with nine octaves over a quarter of a second
# the lowest bins see a few samples of their level, and about half of all seeds put one of them too close to zero).
CASES = {2: (2, 10403, 21), 3: (2, 10403, 22), 9: (2, 4000, 30)}
_REF = {}


def reference(n_octaves):
    """x (B, L) float32; P = |X|^2 + eps, S = log P (B, T, K); tolP, the bound on exp(S); feats (B, T, 60) and their
    bounds.  Computed once per case.  Asserts the floor the bounds assume: tolP below half of P everywhere."""
    if n_octaves not in _REF:
        B, L, seed = CASES[n_octaves]
        x = make_signal(B, L, seed, n_octaves=n_octaves)
        proj = projection(n_octaves)
        P, tolP, feats, bounds = [], [], [], []
        for b in range(B):
            X, R, G, E = transform(x[b].astype(np.float64), n_octaves, with_envelope=True)
            P.append(np.abs(X) ** 2 + EPS)
            tolP.append(power_bounds(X, R, G, E))
            S = np.log(P[-1])
            c = S @ proj.T
            d1 = delta(c)
            feats.append(np.concatenate([c, d1, delta(d1)], axis=1))
            bounds.append(cqcc_bounds(S, tolP[-1], proj))
        ref = {"x": x, "P": np.stack(P), "tolP": np.stack(tolP), "feats": np.stack(feats), "bounds": np.stack(bounds)}
        ref["S"] = np.log(ref["P"])
        assert (ref["tolP"] / ref["P"]).max() < 0.5
        _REF[n_octaves] = ref
    return _REF[n_octaves]
