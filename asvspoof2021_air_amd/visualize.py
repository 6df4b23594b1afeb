"""The reference's embedding figure (visualize.py, behind main_train.py --visualize) with both projections on the GPU.

``pca_device``: column means and the centred D x D Gram matrix on the device (two passes), numpy.linalg.eigh of that
small matrix in fp64 on the host, projection on the device; scikit-learn's sign rule.  ``tsne_device``: scikit-learn's
exact t-SNE (TSNE(method="exact")) - pairwise squared distances, the perplexity bisection, the joint distribution and
the whole descent with its stop rules run on the device without a host synchronisation; the host reads the embedding,
the KL divergence and n_iter in one copy at the end.  The reference calls TSNE in its default Barnes-Hut form, an
approximation of the same objective: the two embeddings agree in what they show, not point by point.

One deviation from scikit-learn's schedule: the first (exaggerated) phase always runs ``exploration_iter`` iterations;
scikit-learn could leave it early on the gradient-norm rule alone.  No CPU fallback: CPU tensors raise AirError."""
import collections
import os

import numpy as np
import torch

from . import ops
from ._hip import AirError

PCAResult = collections.namedtuple("PCAResult", ("projection", "components", "mean", "explained_variance_ratio"))
Embedding = collections.namedtuple("Embedding", (
    "center", "feat_dev", "feat_eval", "center_pca", "feat_pca_dev", "feat_pca_eval", "explained_variance_ratio",
    "kl_divergence", "n_iter", "ind_dev", "ind_eval"))


def _device_matrix(X, what="X"):
    if not torch.is_tensor(X) or not X.is_cuda:
        raise AirError("%s must be a GPU tensor (the HIP path has no CPU fallback)" % what)
    if X.dim() != 2:
        raise ValueError("%s must be 2-d, got %s" % (what, tuple(X.shape)))
    return X.float().contiguous()


def pca_device(X, n_components=2):
    """PCA(n_components).fit_transform of the fp32 (N, D) GPU tensor ``X``: a PCAResult of the projection (N, k, on the
    device), the components (k, D) and the mean (D,) (both on the device) and explained_variance_ratio_ (numpy fp64).
    Each component's largest-magnitude loading is positive (scikit-learn >= 1.5).  One device-to-host copy (the Gram
    matrix) and one small upload (the components)."""
    X = _device_matrix(X)
    N, D = X.shape
    k = int(n_components)
    if k < 1 or k > min(N, D, ops.vis_limits()[2]):
        raise ValueError("n_components must be 1 .. min(N, D, %d), got %d" % (ops.vis_limits()[2], k))
    mean, gram = ops.pca_gram(X)
    w, v = np.linalg.eigh(gram.cpu().numpy())
    order = np.argsort(w)[::-1][:k]
    comps = v[:, order].T
    top = np.argmax(np.abs(comps), axis=1)
    sign = np.sign(comps[np.arange(k), top])
    comps = comps * np.where(sign == 0, 1.0, sign)[:, None]
    w = np.maximum(w, 0.0)
    ratio = w[order] / w.sum() if w.sum() > 0 else np.zeros(k)
    comps_dev = torch.from_numpy(np.ascontiguousarray(comps, dtype=np.float32)).to(X.device)
    return PCAResult(ops.pca_project(X, mean, comps_dev), comps_dev, mean, ratio)


def _pca_init(projection):
    """TSNE(init="pca")'s start from a 2-component projection: scaled to a standard deviation of 1e-4 in column 0."""
    return projection / torch.std(projection[:, 0], unbiased=False) * 1e-4


def tsne_device(X, perplexity=40.0, early_exaggeration=40.0, max_iter=1000, learning_rate="auto", init="pca",
                exploration_iter=250, n_iter_check=50, n_iter_without_progress=300, min_grad_norm=1e-7, return_state=False):
    """Exact t-SNE of the fp32 (N, D) GPU tensor ``X`` into two dimensions (Euclidean metric), after scikit-learn's
    TSNE(method="exact").  ``learning_rate="auto"``: max(N / early_exaggeration / 4, 50).  ``init``: "pca" - the PCA
    projection scaled to a standard deviation of 1e-4 in its first column - or an (N, 2) GPU tensor.  Returns
    (embedding (N, 2) on the device, kl_divergence, n_iter); with ``return_state`` also a dict of the final ``update``
    and ``gains`` tensors and the status record's fields."""
    if torch.is_tensor(X) and X.dim() == 2:  # (scikit-learn's argument check, ahead of the device's)
        if perplexity >= X.shape[0]:
            raise ValueError("perplexity (%s) must be less than n_samples (%d)" % (perplexity, X.shape[0]))
        if not perplexity > 0:
            raise ValueError("perplexity must be positive")
    X = _device_matrix(X)
    N = X.shape[0]
    if learning_rate == "auto":
        learning_rate = max(N / float(early_exaggeration) / 4.0, 50.0)
    if isinstance(init, str):
        if init != "pca":
            raise ValueError("init must be 'pca' or an (N, 2) GPU tensor, got %r" % (init,))
        if X.shape[1] < 2:
            raise ValueError("init='pca' needs at least 2 features")
        y0 = _pca_init(pca_device(X, 2).projection)
    else:
        y0 = _device_matrix(init, "init")
        if tuple(y0.shape) != (N, 2):
            raise ValueError("init must have shape (%d, 2), got %s" % (N, tuple(y0.shape)))
    ws = torch.empty(ops.tsne_ws_bytes(N), dtype=torch.uint8, device=X.device)
    if ws.numel() == 0:
        raise AirError("t-SNE on the device takes 2 .. %d points, got %d" % (ops.vis_limits()[0], N))
    P = ops.pairwise_sqdist(X)
    P, _ = ops.tsne_affinities(P, perplexity)
    ops.tsne_joint(P, ws)
    # [status record | embedding]: what the host reads at the end is one tensor
    pack = torch.empty(ops.TSNE_STATUS_BYTES + N * 8, dtype=torch.uint8, device=X.device)
    status = pack[:ops.TSNE_STATUS_BYTES]
    y = pack[ops.TSNE_STATUS_BYTES:].view(torch.float32).view(N, 2)
    y.copy_(y0)
    update, gains = torch.empty_like(y0), torch.empty_like(y0)
    ops.tsne_run(P, y, update, gains, status, max_iter=max_iter, exploration_iter=exploration_iter,
                 n_iter_check=n_iter_check, n_iter_without_progress=n_iter_without_progress, min_grad_norm=min_grad_norm,
                 learning_rate=learning_rate, early_exaggeration=early_exaggeration, ws=ws)
    rec = pack[:ops.TSNE_STATUS_BYTES].cpu().numpy().view(ops.TSNE_STATUS_DTYPE)[0]  # (syncs: the run is done)
    out = (y.clone(), float(rec["kl"]), int(rec["n_iter"]))
    if return_state:
        state = {k: rec[k].item() for k in ("stopped", "reason", "best_iter", "best_error", "grad_norm")}
        state.update(update=update, gains=gains)
        return out + (state,)
    return out


def sample_indices(n_dev, n_eval, k=5000, seed=888):
    """The two index draws of the reference's figure (visualize.py:18-21): the first ``k`` of a permutation of the dev
    trials, then - continuing the same stream - of the eval trials.  Drawn from a local generator: the caller's global
    generator is untouched; the sequence is the one torch.manual_seed(seed) would give."""
    g = torch.Generator()
    g.manual_seed(int(seed))
    return torch.randperm(int(n_dev), generator=g)[:k], torch.randperm(int(n_eval), generator=g)[:k]


def _to_device(t, device, dtype=None):
    t = t if torch.is_tensor(t) else torch.from_numpy(np.asarray(t))
    return t.to(device=device, dtype=dtype)


def embed_dev_and_eval(dev_feat, dev_labels, eval_feat, eval_labels, center, seed=88, k=5000, **tsne_kw):
    """The projections behind the reference's figure: ``k`` sampled dev and eval embeddings (sample_indices) are
    gathered on the device, stacked as [center; dev; eval] (visualize.py:28) and projected once by tsne_device
    (perplexity 40, early exaggeration 40 unless ``tsne_kw`` says otherwise) and once by pca_device.  Returns an
    Embedding: the six blocks of visualize.py:32-40 (device tensors), explained_variance_ratio, kl_divergence, n_iter
    and the two index draws.  ``seed`` is accepted for the signature: with PCA initialisation scikit-learn uses
    random_state only for the start vector of its ARPACK solver, which has no counterpart here."""
    if not torch.is_tensor(dev_feat) or not dev_feat.is_cuda or not torch.is_tensor(eval_feat) or not eval_feat.is_cuda:
        raise AirError("dev_feat and eval_feat must be GPU tensors (the HIP path has no CPU fallback)")
    dev = dev_feat.device
    center = _to_device(center, dev, torch.float32).reshape(-1, dev_feat.shape[1])
    ind_dev, ind_eval = sample_indices(dev_feat.shape[0], eval_feat.shape[0], k)
    X = torch.cat((center, dev_feat.float()[ind_dev.to(dev)], eval_feat.float()[ind_eval.to(dev)]), 0)
    nc, nd = center.shape[0], ind_dev.numel()
    kw = dict(perplexity=40.0, early_exaggeration=40.0)
    kw.update(tsne_kw)
    pca = pca_device(X, 2)  # (once: the figure's PCA panels and the t-SNE's start)
    pr = pca.projection
    if isinstance(kw.get("init", "pca"), str) and kw.get("init", "pca") == "pca":
        kw["init"] = _pca_init(pr)
    emb, kl, n_iter = tsne_device(X, **kw)
    return Embedding(emb[:nc], emb[nc:nc + nd], emb[nc + nd:], pr[:nc], pr[nc:nc + nd], pr[nc + nd:],
                     pca.explained_variance_ratio, kl, n_iter, ind_dev, ind_eval)


def visualize_dev_and_eval(dev_feat, dev_labels, dev_tags, eval_feat, eval_labels, eval_tags, center, seed, out_fold,
                           k=5000, **tsne_kw):
    """The reference's figure (visualize.py:13-65) written to ``out_fold/_vis_feat.pdf``: t-SNE of the dev and of the
    eval sample on one pair of axes limits (top), PCA likewise (bottom), bona fide and spoof in two colours, the
    centre as a cross on the t-SNE panels.  Host arrays or device tensors; the tags are accepted for the signature (the
    reference does not use them either).  Nothing is shown, no global seed or environment variable is written.
    Returns the Embedding."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    device = next((t.device for t in (dev_feat, eval_feat) if torch.is_tensor(t) and t.is_cuda), torch.device("cuda"))
    dev_feat, eval_feat = _to_device(dev_feat, device, torch.float32), _to_device(eval_feat, device, torch.float32)
    e = embed_dev_and_eval(dev_feat, dev_labels, eval_feat, eval_labels, center, seed, k, **tsne_kw)
    labels = (_to_device(dev_labels, "cpu")[e.ind_dev].numpy(), _to_device(eval_labels, "cpu")[e.ind_eval].numpy())
    host = lambda t: t.cpu().numpy()
    colours = ("#7030a0", "#ff0000", "#ffff00")
    fig, axes = plt.subplots(2, 2, figsize=(8, 8))
    rows = ((host(e.feat_dev), host(e.feat_eval), host(e.center)), (host(e.feat_pca_dev), host(e.feat_pca_eval), None))
    for ax_row, (left, right, cross) in zip(axes, rows):
        for ax, pts, lab in zip(ax_row, (left, right), labels):
            if ax is ax_row[1]:  # the eval panel shares the dev panel's limits
                ax.set_xlim(ax_row[0].get_xlim())
                ax.set_ylim(ax_row[0].get_ylim())
            for cls in (0, 1):
                ax.plot(pts[lab == cls, 0], pts[lab == cls, 1], ".", c=colours[cls], markersize=1.2)
            if cross is not None:
                ax.plot(cross[:, 0], cross[:, 1], "x", c=colours[2], markersize=5)
            ax.axis("off")
    os.makedirs(out_fold, exist_ok=True)
    fig.savefig(os.path.join(out_fold, "_vis_feat.pdf"), dpi=500, bbox_inches="tight")
    fig.clf()
    plt.close(fig)
    return e


def get_features(trainer, batches):
    """The reference's get_features (visualize.py:67-89) on the sync-free pass: ``trainer.evaluate(batches,
    keep_feats=True)`` reduced to (feats (trials, enc_dim) fp32, labels (trials,) int64), both on the device."""
    r = trainer.evaluate(batches, keep_feats=True)
    return r.feats, r.labels
