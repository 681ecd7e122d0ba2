"""Writes tests/golden/tsne_small.npz: what scikit-learn's exact t-SNE gives on two small inputs,
for tests/test_latent_cpu.py and tests/test_latent_gpu.py (data only; needs scikit-learn).

    python tools/gen_golden_tsne.py

p150   X 150 x 16 (three Gaussian clusters), sklearn's condensed joint P at perplexity 20 (of the
       fp64 squared distances from the differences, which sklearn rounds to fp32) and, for
       two probes Y (1e-4 * randn and 10 * randn), the kl and grad of _kl_divergence.
kl450  X 450 x 16 of the same recipe with its cluster labels and, for init seeds 0-3, the final
       kl_divergence_ of TSNE(method="exact", perplexity=30, max_iter=500, learning_rate=200)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import sklearn
    from sklearn.manifold import TSNE, _t_sne

    from tests import tsne_reference as R
    out = {"sklearn_version": np.array(sklearn.__version__)}

    X, _ = R.clusters(150)
    D = R.sqdist(X)                     # fp64 from the differences; _joint_probabilities rounds it to fp32
    P = _t_sne._joint_probabilities(D, 20, 0)
    out.update(p150_X=X, p150_P=np.asarray(P, dtype=np.float64))
    rs = np.random.RandomState(1)
    for k, scale in enumerate((1e-4, 10.0)):
        Y = (scale * rs.randn(150, 2)).astype(np.float32)
        kl, grad = _t_sne._kl_divergence(Y.astype(np.float64).ravel(), P, 1.0, 150, 2)
        out.update({f"p150_Y{k}": Y, f"p150_kl{k}": np.float64(kl), f"p150_grad{k}": grad.reshape(150, 2)})

    X, labels = R.clusters(450)
    kls, purities = [], []
    for seed in range(4):
        t = TSNE(method="exact", perplexity=30, max_iter=500, learning_rate=200.0, init=R.random_init(450, seed),
                 min_grad_norm=0.0, n_iter_without_progress=10 ** 6, early_exaggeration=12.0)
        Y = t.fit_transform(X)
        kls.append(t.kl_divergence_)
        purities.append(R.purity(Y, labels))
    out.update(kl450_X=X, kl450_labels=labels.astype(np.int64), kl450_kl=np.array(kls, dtype=np.float64),
               kl450_purity=np.array(purities))
    path = os.path.join(ROOT, "tests", "golden", "tsne_small.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes; kl450 {kls} purity {purities}")


if __name__ == "__main__":
    main()
