"""Plain numpy fp64 statement of the GMM back-end (include/air_hip.h, "GMM back-end"), and the error bounds the GPU
tests hold the kernels to.  tests/test_gmm_cpu.py pins it to scikit-learn's GaussianMixture(covariance_type="diag").

    lp[n,k]  = log w_k - 0.5 * (D log(2 pi) + sum_d mu^2 p + sum_d log var) + sum_d x (mu p) - 0.5 sum_d x^2 p
    lse[n]   = logsumexp_k lp[n,k]
    r[n,k]   = exp(lp[n,k] - lse[n])
    S0 = sum_n r, S1 = sum_n r x, S2 = sum_n r x^2, LL = sum_n lse, Nf = N
    nk = S0 + 10 eps; mu = S1 / nk; var = S2 / nk - mu^2 + reg_covar; w = nk / sum nk; lower_bound = LL / Nf

Bounds (u = 2^-53, the unit roundoff of fp64; every input is taken as exact, frames are fp32 widened exactly).  Both
the kernel and this oracle are roundings of the same exact quantity, each within the bound, so two results are
compared within TWICE the bound (``BOTH``).
"""
import numpy as np

U = 2.0 ** -53
BOTH = 2.0          # |a - b| <= |a - exact| + |exact - b|
TINY = 10 * np.finfo(np.float64).eps
LOG_2PI = float(np.log(2.0 * np.pi))


# ------------------------------------------------------------------------------------------------------ the model
def constants(w, mu, var):
    """c_k = log w_k - 0.5 (D log(2 pi) + sum_d mu^2 p + sum_d log var)."""
    D = mu.shape[1]
    with np.errstate(divide="ignore"):
        return np.log(w) - 0.5 * (D * LOG_2PI + np.sum(mu * mu / var, axis=1) + np.sum(np.log(var), axis=1))


def logits(x, w, mu, var):
    x = np.asarray(x, dtype=np.float64)
    p = 1.0 / var
    return constants(w, mu, var)[None, :] + x @ (mu * p).T - 0.5 * ((x * x) @ p.T)


def logsumexp(lp):
    m = lp.max(axis=1)
    return m + np.log(np.exp(lp - m[:, None]).sum(axis=1))


def e_step(x, w, mu, var):
    lp = logits(x, w, mu, var)
    lse = logsumexp(lp)
    return lp, lse, np.exp(lp - lse[:, None])


def statistics(x, w, mu, var):
    """(S0 (K), S1 (K, D), S2 (K, D), LL, Nf)."""
    x = np.asarray(x, dtype=np.float64)
    _, lse, r = e_step(x, w, mu, var)
    return r.sum(axis=0), r.T @ x, r.T @ (x * x), float(lse.sum()), x.shape[0]


def m_step(S0, S1, S2, LL, Nf, reg_covar):
    """-> (w, mu, var, lower_bound)."""
    nk = S0 + TINY
    mu = S1 / nk[:, None]
    var = S2 / nk[:, None] - mu * mu + reg_covar
    with np.errstate(invalid="ignore", divide="ignore"):
        return nk / nk.sum(), mu, var, np.float64(LL) / np.float64(Nf)


def fit(x, w, mu, var, reg_covar=1e-6, max_iter=100, tol=1e-3):
    """scikit-learn's loop (BaseMixture.fit, n_init = 1, warm parameters given) -> dict with the final parameters,
    ``lower_bound`` (of the last E-step), ``n_iter``, ``converged`` and ``bounds`` (the lower bound per iteration)."""
    lower, converged, n_iter, bounds = -np.inf, False, 0, []
    for n_iter in range(1, max_iter + 1):
        prev = lower
        w, mu, var, lower = m_step(*statistics(x, w, mu, var), reg_covar)
        bounds.append(float(lower))
        if abs(lower - prev) < tol:
            converged = True
            break
    return dict(w=w, mu=mu, var=var, lower_bound=float(lower), n_iter=n_iter, converged=converged, bounds=bounds)


def score_samples(x, w, mu, var):
    return logsumexp(logits(x, w, mu, var))


def row_scores(rows, w, mu, var):
    """Mean of lse over each row's frames; ``rows`` is a list of (n_b, D) arrays."""
    return np.array([score_samples(r, w, mu, var).mean() if len(r) else np.nan for r in rows])


def llr(rows, bona, spoof):
    """mean lse_bona - mean lse_spoof per row; ``bona`` / ``spoof`` are (w, mu, var)."""
    return row_scores(rows, *bona) - row_scores(rows, *spoof)


# -------------------------------------------------------------------------------------------------------- bounds
def logit_bound(x, w, mu, var):
    """(N, K).  A logit is a sum of 2 D + 1 products plus a constant, each operand (mu p, -0.5 p, c_k) itself rounded
    a couple of times: |d lp| <= (2 D + 3) u (|c_k| + sum_d |x mu p| + 0.5 sum_d x^2 p).  2 D + 1 terms summed in any
    order carry at most 2 D u relative on the sum of magnitudes; the +3 covers the roundings of the product, of p and
    of mu p / c_k."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    p = 1.0 / var
    D = mu.shape[1]
    mag = np.abs(constants(w, mu, var))[None, :] + x @ np.abs(mu * p).T + 0.5 * ((x * x) @ p.T)
    return (2 * D + 3) * U * np.where(np.isfinite(mag), mag, 0.0)


def lse_bound(x, w, mu, var):
    """(N,).  An ALLOWANCE rather than a tight bound: its K-proportional term is a worst case for any summation order,
    not the 'few u' a particular order would give (2052 u at K = 1024).  lse moves by at most the largest logit error of its frame (logsumexp is 1-Lipschitz in the max norm).
    On top: each of the K terms exp(lp - m) carries 1 ulp of exp and u |lp - m| from the rounded shift, the latter at
    most u d exp(-d) <= u of the term's weight - 2 u per term; K terms summed in any order (K - 1) u relative; the
    log 1 ulp and the final sum 1 ulp of |lse|: (2 K + 4) u + 2 u |lse|, the 'few u for exp / log' times the K terms
    a tree sums."""
    K = mu.shape[0]
    lse = score_samples(x, w, mu, var)
    return logit_bound(x, w, mu, var).max(axis=1) + (2 * K + 4) * U + 2 * U * np.abs(lse)


def resp_eps(x, w, mu, var):
    """(N, K) relative error of r = exp(lp - lse): the absolute error of the exponent - the logit's, lse's and the
    rounded difference's - plus 2 u for exp."""
    lp, lse, _ = e_step(x, w, mu, var)
    with np.errstate(invalid="ignore"):
        diff = np.where(np.isfinite(lp), np.abs(lp - lse[:, None]), 0.0)
    return logit_bound(x, w, mu, var) + lse_bound(x, w, mu, var)[:, None] + U * diff + 2 * U


def statistics_bound(x, w, mu, var, n_terms=None):
    """Bounds of (S0, S1, S2, LL): a statistic over n terms carries sum_n r |x| (eps_n + (n_terms + 2) u) - the form
    the RawBoost and resampler oracles use: each term is off by its relative error eps_n, the product adds one
    rounding, and n_terms terms summed in any order (a tree of partials included) carry at most n_terms u relative on
    the sum of magnitudes."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    n_terms = N if n_terms is None else n_terms
    _, lse, r = e_step(x, w, mu, var)
    e = r * (resp_eps(x, w, mu, var) + (n_terms + 2) * U)
    ax = np.abs(x)
    b_ll = float(lse_bound(x, w, mu, var).sum() + (n_terms + 2) * U * np.abs(lse).sum())
    return e.sum(axis=0), e.T @ ax, e.T @ (ax * ax), b_ll


def m_step_bound(S0, S1, S2, reg_covar):
    """Bounds of (w, mu, var) of ``m_step`` fed the SAME statistics: mu one division (1 ulp, 2 u with nk's own
    rounding), var a division, a square, a difference and a sum - 4 u of (S2 / nk + mu^2 + reg_covar), w a division by
    a K-term sum in any order, (K + 2) u."""
    nk = S0 + TINY
    mu = S1 / nk[:, None]
    K = S0.shape[0]
    return (K + 2) * U * nk / nk.sum(), 2 * U * np.abs(mu), 4 * U * (np.abs(S2) / nk[:, None] + mu * mu + reg_covar)


# ---------------------------------------------------------------------------------------------------------- data
def lfcc_like(N, D, seed, clusters=4):
    """LFCC-like fp32 frames: coefficient 0 sits at an offset of 25, the variances fall from 1 to 1e-4 over the
    coefficients (the delta streams), a few overlapping clusters about a standard deviation apart."""
    rng = np.random.default_rng(seed)
    std = np.logspace(0.0, -2.0, D)
    centres = rng.normal(size=(clusters, D)) * 1.0 * std
    centres[:, 0] += 25.0
    z = rng.integers(0, clusters, size=N)
    return (centres[z] + rng.normal(size=(N, D)) * std).astype(np.float32)


def separable(N, D, K, seed, offset=0.0):
    """A mixture of K well separated unit-variance clusters (centres 8 apart per coordinate draw), fp32."""
    rng = np.random.default_rng(seed)
    centres = rng.integers(-2, 3, size=(K, D)) * 8.0 + offset
    z = rng.integers(0, K, size=N)
    return (centres[z] + rng.normal(size=(N, D))).astype(np.float32)


def init_from_data(x, K, seed, reg_covar=1e-6):
    """Uniform weights, K distinct frames as means, the global variance in every covariance row."""
    x = np.asarray(x, dtype=np.float64)
    pick = np.sort(np.random.default_rng(seed).choice(x.shape[0], K, replace=False))
    var = x.var(axis=0) + reg_covar
    return np.full(K, 1.0 / K), x[pick].copy(), np.tile(var, (K, 1))


def integer_frames(N, D):
    """x[n, d] = (3 n + 7 d) % 11 - 5: small integers, asymmetric in n and d."""
    n, d = np.arange(N)[:, None], np.arange(D)[None, :]
    return ((3 * n + 7 * d) % 11 - 5).astype(np.float32)


def params_bound(x, w, mu, var, reg_covar, n_terms=None):
    """Bounds of (w, mu, var, lower_bound) after ONE EM step from exact (w, mu, var): the statistics' bounds pushed
    through the M-step's quotients to first order, plus ``m_step_bound`` for the M-step's own roundings.
      mu = S1 / nk:               (b1 + |mu| b0) / nk
      var = S2 / nk - mu^2 + reg: (b2 + (S2 / nk) b0) / nk + 2 |mu| |d mu|
      w = nk / sum nk:            b0 / sum nk + w sum b0 / sum nk
      lower_bound = LL / N:       bLL / N + 2 u |LL / N|"""
    S0, S1, S2, LL, Nf = statistics(x, w, mu, var)
    b0, b1, b2, bll = statistics_bound(x, w, mu, var, n_terms)
    nk = (S0 + TINY)[:, None]
    m = S1 / nk
    rw, rm, rv = m_step_bound(S0, S1, S2, reg_covar)
    dmu = (b1 + np.abs(m) * b0[:, None]) / nk + rm
    dvar = (b2 + (S2 / nk) * b0[:, None]) / nk + 2 * np.abs(m) * dmu + rv
    tot = nk.sum()
    dw = b0 / tot + (nk[:, 0] / tot) * b0.sum() / tot + rw
    return dw, dmu, dvar, bll / Nf + 2 * U * abs(LL / Nf)
