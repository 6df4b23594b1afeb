"""Writes tests/golden/visualize.npz: scikit-learn's own outputs (1.7, with scipy) for two small synthetic embedding
sets, and the run-to-run spread of the fp64 oracle (tests/tsne_oracle.py).

    python tests/golden/make_golden_visualize.py

Per set (N = 96 and N = 192, D = 16, three clusters, perplexity 40, early exaggeration 40):
  x_N, labels_N            the inputs (tsne_oracle.clusters(N, 16, seed=N))
  p_N                      _joint_probabilities(squared distances as fp32), condensed
  y_N (3, N, 2)            three embeddings: the PCA start, and the fp64 oracle's after 5 and after 300 iterations
  kl_N (3, 2), grad_N      _kl_divergence's value and gradient at each, with exaggeration 1 and 40
  pca_N, pca_ratio_N       PCA(2).fit_transform and explained_variance_ratio_
  sk_kl_N                  kl_divergence_ of TSNE(method="exact", init="pca", perplexity=40, early_exaggeration=40)
  spread_kl_N, spread_nn_N final KL and nearest-neighbour purity of the fp64 oracle's full schedule from eight starts
                           that differ by 1e-7 relative: trajectories diverge after some 20 iterations whatever the
                           arithmetic, so the end of a run is comparable only within this spread
The reference's sampling lines (visualize.py:18-21) are restated here - its module cannot be imported, it imports a
class its dataset.py lacks: ind_dev / ind_eval for (n_dev, n_eval, k) = (300, 400, 64)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tsne_oracle as o  # noqa: E402

PERPLEXITY, EXAGGERATION = 40.0, 40.0


def main():
    from sklearn.decomposition import PCA
    from sklearn.manifold import TSNE, _t_sne
    out = {}
    for N in (96, 192):
        X, labels = o.clusters(N, 16, seed=N)
        D = o.sqdist(X).astype(np.float32)
        p = _t_sne._joint_probabilities(D, PERPLEXITY, 0)
        P = o.joint(o.binary_search_perplexity(D, PERPLEXITY)[0])
        lr = max(N / EXAGGERATION / 4.0, 50.0)
        y0 = o.pca_init(X)
        trace = []
        o.descent(P, y0, max_iter=300, learning_rate=lr, early_exaggeration=EXAGGERATION, trace=trace)
        ys = np.stack([y0, trace[4][1], trace[299][1]])
        kls = np.zeros((3, 2))
        grads = np.zeros((3, 2, N, 2))
        for a, y in enumerate(ys):
            for b, ex in enumerate((1.0, EXAGGERATION)):
                kl, g = _t_sne._kl_divergence(y.ravel().copy(), p * ex, 1.0, N, 2)
                kls[a, b], grads[a, b] = kl, g.reshape(N, 2)
        pca = PCA(n_components=2)
        proj = pca.fit_transform(X)
        sk = TSNE(method="exact", init="pca", perplexity=PERPLEXITY, early_exaggeration=EXAGGERATION, random_state=88)
        sk.fit(X)
        rng = np.random.RandomState(7)
        spread_kl, spread_nn = [], []
        for _ in range(8):
            start = y0 * (1.0 + 1e-7 * rng.uniform(-1.0, 1.0, y0.shape))
            r = o.descent(P, start, learning_rate=lr, early_exaggeration=EXAGGERATION)
            spread_kl.append(r["kl"])
            spread_nn.append(o.nn_purity(r["y"], labels))
        out.update({"x_%d" % N: X, "labels_%d" % N: labels.astype(np.int32), "p_%d" % N: p, "y_%d" % N: ys,
                    "kl_%d" % N: kls, "grad_%d" % N: grads, "pca_%d" % N: proj, "pca_ratio_%d" % N: pca.explained_variance_ratio_,
                    "sk_kl_%d" % N: np.float64(sk.kl_divergence_), "spread_kl_%d" % N: np.array(spread_kl),
                    "spread_nn_%d" % N: np.array(spread_nn)})
        print(N, "sklearn exact KL", sk.kl_divergence_, "oracle KLs", spread_kl, "purity", spread_nn)
    state = torch.get_rng_state()
    torch.manual_seed(888)
    out["ind_dev"] = torch.randperm(300)[:64].numpy()
    out["ind_eval"] = torch.randperm(400)[:64].numpy()
    torch.set_rng_state(state)
    out["sample_args"] = np.array([300, 400, 64])
    path = os.path.join(HERE, "visualize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
