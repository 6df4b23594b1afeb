"""Plain numpy statements of what csrc/embed_vis.hip computes: scikit-learn's exact t-SNE (_binary_search_perplexity,
_joint_probabilities, _kl_divergence, _gradient_descent with TSNE._tsne's two phases) and PCA with scikit-learn's sign
rule.  fp64 by default - the reference of the GPU tests; every function also runs with ``dtype=np.float32``, where each
array and each scalar of the arithmetic is fp32: that restatement's distance from fp64 is the yardstick the tests'
tolerances are derived from (profiles/embedding_vis.md)."""
import numpy as np

EPS = np.finfo(np.float64).eps  # MACHINE_EPSILON of sklearn/manifold/_t_sne.py
# sklearn/manifold/_utils.pyx declares both as C floats
PERPLEXITY_TOLERANCE = float(np.float32(1e-5))
EPSILON_DBL = float(np.float32(1e-8))


def sqdist(X, dtype=np.float64):
    """(N, N) squared Euclidean distances, summed as (x_i - x_j)^2."""
    X = np.asarray(X, dtype=dtype)
    diff = X[:, None, :] - X[None, :, :]
    return np.sum(diff * diff, axis=2, dtype=dtype)


def binary_search_perplexity(D, perplexity, dtype=np.float64, n_steps=100):
    """_binary_search_perplexity over dense squared distances: (conditional P (N, N), beta (N,), entropy error (N,))."""
    D = np.asarray(D, dtype=dtype)
    N = D.shape[0]
    f = dtype
    target = f(np.log(f(perplexity)))
    P = np.zeros((N, N), dtype=dtype)
    betas = np.zeros(N, dtype=dtype)
    errs = np.zeros(N, dtype=dtype)
    for i in range(N):
        d = np.delete(D[i], i)
        beta, lo, hi = f(1.0), f(-np.inf), f(np.inf)
        for _ in range(n_steps):
            with np.errstate(under="ignore", over="ignore"):
                e = np.exp(-d * beta)
            s = e.sum(dtype=dtype)
            if s == 0.0:
                s = f(EPSILON_DBL)
            p = e / s
            h = f(np.log(s)) + beta * np.sum(d * p, dtype=dtype)
            diff = f(h - target)
            used = beta
            if abs(diff) <= f(PERPLEXITY_TOLERANCE):
                break
            if diff > 0.0:
                lo = beta
                beta = beta * f(2.0) if np.isinf(hi) else (beta + hi) / f(2.0)
            else:
                hi = beta
                beta = beta / f(2.0) if np.isinf(lo) else (beta + lo) / f(2.0)
        P[i] = np.insert(p, i, 0.0)
        betas[i] = used
        errs[i] = diff
    return P, betas, errs


def joint(cond, dtype=np.float64):
    """_joint_probabilities' last three lines on the dense matrix: off-diagonal max((C + C^T) / max(sum, eps), eps)."""
    C = np.asarray(cond, dtype=dtype)
    P = C + C.T
    s = max(P.sum(dtype=dtype), dtype(EPS))
    P = np.maximum(P / s, dtype(EPS))
    np.fill_diagonal(P, 0.0)
    return P.astype(dtype)


def condensed(P):
    """The upper triangle in scipy.spatial.distance.squareform's order."""
    i, j = np.triu_indices(P.shape[0], 1)
    return P[i, j]


def kl_grad(P, Y, exaggeration=1.0, dtype=np.float64, floor_q_in_grad=True):
    """_kl_divergence on dense matrices: (kl, grad (N, 2), Z).  ``P`` is the joint WITHOUT exaggeration."""
    P = np.asarray(P, dtype=dtype) * dtype(exaggeration)
    Y = np.asarray(Y, dtype=dtype)
    diff = Y[:, None, :] - Y[None, :, :]
    n = dtype(1.0) / (dtype(1.0) + np.sum(diff * diff, axis=2, dtype=dtype))
    np.fill_diagonal(n, 0.0)
    Z = n.sum(dtype=dtype)
    Q = np.maximum(n / Z, dtype(EPS))
    off = ~np.eye(P.shape[0], dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        kl = np.sum(P[off] * np.log(np.maximum(P[off], dtype(EPS)) / Q[off]), dtype=dtype)
    Qg = Q if floor_q_in_grad else n / Z
    W = (P - Qg) * n
    np.fill_diagonal(W, 0.0)
    grad = dtype(4.0) * np.einsum("ij,ijk->ik", W, diff).astype(dtype)
    return dtype(kl), grad.astype(dtype), Z


def descent(P, Y0, max_iter=1000, exploration_iter=250, n_iter_check=50, n_iter_without_progress=300, min_grad_norm=1e-7,
            learning_rate=200.0, early_exaggeration=12.0, dtype=np.float64, trace=None):
    """TSNE._tsne's two _gradient_descent calls as one loop over iterations 0 .. max_iter - 1: momentum 0.5 with
    exaggeration below ``exploration_iter``, then update = 0, gains = 1, best error forgotten, momentum 0.8, exaggeration 1
    and the stop rules every ``n_iter_check`` iterations.  The first phase always runs its full length.  Returns a dict:
    y, update, gains, kl (of the last iteration that computed it), n_iter, stopped.  ``trace``: a list that gets
    (i, y, update, gains) after every iteration."""
    f = dtype
    P = np.asarray(P, dtype=dtype)
    y = np.array(Y0, dtype=dtype)
    update = np.zeros_like(y)
    gains = np.ones_like(y)
    best_error, best_iter = np.finfo(np.float64).max, 0
    kl, n_iter, stopped = np.nan, 0, False
    for i in range(max_iter):
        second = i >= exploration_iter
        if i > 0 and i == exploration_iter:
            update[:] = 0
            gains[:] = 1
            best_error, best_iter = np.finfo(np.float64).max, i
        check = second and (i + 1) % n_iter_check == 0
        want_kl = check or i == max_iter - 1
        err, grad, _ = kl_grad(P, y, early_exaggeration if not second else 1.0, dtype)
        inc = update * grad < 0.0
        gains = np.where(inc, gains + f(0.2), gains * f(0.8)).astype(dtype)
        gains = np.maximum(gains, f(0.01))
        grad = grad * gains
        update = (f(0.8 if second else 0.5) * update - f(learning_rate) * grad).astype(dtype)
        y = (y + update).astype(dtype)
        if trace is not None:
            trace.append((i, y.copy(), update.copy(), gains.copy()))
        if want_kl:
            kl, n_iter = float(err), i
        if check:
            if err < best_error:
                best_error, best_iter = err, i
            elif i - best_iter > n_iter_without_progress:
                stopped = True
                break
            if np.sqrt(np.sum(grad.astype(np.float64) ** 2)) <= min_grad_norm:
                stopped = True
                break
    return dict(y=y, update=update, gains=gains, kl=kl, n_iter=n_iter, stopped=stopped)


def pca(X, n_components=2, dtype=np.float64):
    """PCA as scikit-learn >= 1.5 returns it: (projection, components (k, D), mean, explained_variance_ratio, Gram).
    Sign rule svd_flip(u_based_decision=False): each component's largest-magnitude loading is positive."""
    X = np.asarray(X, dtype=dtype)
    mean = X.mean(axis=0, dtype=dtype)
    Xc = X - mean
    gram = (Xc.T @ Xc).astype(dtype)
    w, v = np.linalg.eigh(gram.astype(np.float64))
    order = np.argsort(w)[::-1][:n_components]
    comps = v[:, order].T
    top = np.argmax(np.abs(comps), axis=1)
    comps = comps * np.sign(comps[np.arange(comps.shape[0]), top])[:, None]
    comps = comps.astype(dtype)
    ratio = np.maximum(w[order], 0.0) / np.maximum(w, 0.0).sum()
    return (Xc @ comps.T).astype(dtype), comps, mean, ratio, gram


def pca_init(X, dtype=np.float64):
    """TSNE(init="pca")'s start: the 2-component projection scaled to std 1e-4 in its first column."""
    proj = pca(X, 2, dtype)[0]
    return (proj / np.std(proj[:, 0]) * dtype(1e-4)).astype(dtype)


def nn_purity(Y, labels):
    """Share of points whose nearest embedded neighbour carries their own label."""
    d = sqdist(Y)
    np.fill_diagonal(d, np.inf)
    return float(np.mean(labels[np.argmin(d, axis=1)] == labels))


def clusters(n, d, seed, k=3, sep=4.0):
    """The synthetic embeddings of the fixtures: k Gaussian clusters of unit spread, centres ``sep`` apart per axis."""
    rng = np.random.RandomState(seed)
    labels = np.arange(n) % k
    centres = rng.randn(k, d) * sep
    return (centres[labels] + rng.randn(n, d)).astype(np.float32), labels
