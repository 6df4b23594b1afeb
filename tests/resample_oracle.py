"""The sample-rate conversion of include/air_hip.h ("WAV decode / resample") restated in numpy fp64, from its formulas:

    Z = 64, R = 0.9475937167399596, BETA = 14.769656459379492
    w(u) = I0(BETA sqrt(1 - (u / Z)^2)) / I0(BETA);  h(u) = R sinc(R u) w(u) for |u| < Z, else 0   (numpy's sinc)
    g = gcd(sr, tg), L = tg / g, M = sr / g, s = min(1, L / M), H = ceil(Z / s), K = 2 H
    y[t] = sum_{j < K} c[p][j] x[n0 - H + 1 + j],  n0 = floor(t M / L), p = (t M) mod L, x = 0 outside [0, n)
    c[p][j] = s h(s (p / L + H - 1 - j)),  len(y) = ceil(n L / M)

I0 is scipy.special.i0; nothing here is taken from the device code.  ``resample`` also returns, per output sample, the
bound the GPU tests hold the fp32 device sum to: (K + 3) 2^-24 sum_j |c_j x_j| + 2^-24 |y| - K - 1 roundings of an fp32
accumulation of K products in any order, one for the coefficient's rounding to fp32, one to spare, and the rounding of
the result itself.
"""
import math

import numpy as np
from scipy.special import i0

Z = 64
R = 0.9475937167399596
BETA = 14.769656459379492
EPS = 2.0 ** -24


def geometry(sr, tg=16000):
    """(L, M, K).  H = ceil(Z / s) in exact integer arithmetic: ceil(Z M / L) when s = L / M < 1."""
    g = math.gcd(int(sr), int(tg))
    L, M = int(tg) // g, int(sr) // g
    H = Z if L >= M else -(-Z * M // L)
    return L, M, 2 * H


def out_length(n, sr, tg=16000):
    L, M, _ = geometry(sr, tg)
    return -(-int(n) * L // M)


def h(u):
    u = np.asarray(u, dtype=np.float64)
    inside = np.abs(u) < Z
    r = np.where(inside, u / Z, 0.0)
    w = i0(BETA * np.sqrt(1.0 - r * r)) / i0(BETA)
    return np.where(inside, R * np.sinc(R * u) * w, 0.0)


def table(sr, tg=16000):
    """c (L, K) in fp64."""
    L, M, K = geometry(sr, tg)
    H = K // 2
    s = min(1.0, L / M)
    p = np.arange(L, dtype=np.float64)[:, None]
    j = np.arange(K, dtype=np.float64)[None, :]
    return s * h(s * (p / L + (H - 1) - j))


_tables = {}


def resample(x, sr, tg=16000):
    """x (n,) -> (y (ceil(n L / M),) fp64, bound (same shape) fp64)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = len(x)
    L, M, K = geometry(sr, tg)
    if L == M:
        return x.copy(), np.zeros(n)
    H = K // 2
    c = _tables.get((sr, tg))
    if c is None:
        c = _tables[(sr, tg)] = table(sr, tg)
    nout = -(-n * L // M)
    t = np.arange(nout, dtype=np.int64)
    n0, p = (t * M) // L, (t * M) % L
    idx = n0[:, None] - H + 1 + np.arange(K, dtype=np.int64)[None, :]
    ok = (idx >= 0) & (idx < n)
    xs = np.where(ok, x[np.clip(idx, 0, n - 1)], 0.0)
    prod = c[p] * xs
    y = prod.sum(axis=1)
    return y, (K + 3) * EPS * np.abs(prod).sum(axis=1) + EPS * np.abs(y)
