"""Exact t-SNE on MI355X (mdil_ss_amd.latent / libmdil_tsne.so) at the two sizes the latent-space
plots use -- 8192 x 128 (one image's encoder output) and 20000 x 20 (sampled logits) -- against the
same iteration written with dense torch ops on the same device, and against scikit-learn's exact
objective on the host when scikit-learn is importable.

    python tools/bench_tsne.py [--iters 200 --rounds 5 --perplexity 100] [--no-sklearn] [--out FILE]

Per size: the time of ``sqdist``, of ``affinities`` and per iteration of ``run`` (device events
around one call of ``--iters`` iterations, KL logging off, after a warm-up call; the variants
alternate over ``--rounds`` rounds; median and spread reported), the sweep's achieved bytes/s
counting the N^2 fp32 entries of P once per iteration, and the torch iteration (``cdist``,
elementwise, ``sum``, one ``matmul`` for the weighted sums); every timed call starts from the same
state and must leave finite coordinates.  The two routes' gradients are compared before anything is
timed, and the tool fails when they differ by more than N * 2^-24 of the largest component.  scikit-learn: the wall time of one call of
``_kl_divergence`` (objective + gradient, what one of its iterations costs) on the host, for sizes
up to ``--sklearn-max-points``.  No GPU: it fails, it does not fall back."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools._bench_common import HBM_PEAK, spread, timed, write_report  # noqa: E402

SIZES = (("encoder", 8192, 128), ("logits", 20000, 20))


def points(n, d, dev):
    """20 Gaussian classes, as a segmentation network's features of one image roughly are."""
    g = torch.Generator(device=dev).manual_seed(n + d)
    centres = 4.0 * torch.randn(20, d, device=dev, generator=g)
    which = torch.randint(0, 20, (n,), device=dev, generator=g)
    return (centres[which] + torch.randn(n, d, device=dev, generator=g)).contiguous()


def torch_iteration(P, Y, update, gains, e, momentum, lr):
    """One iteration of the same descent with dense torch ops."""
    n = 1.0 / (1.0 + torch.cdist(Y, Y).square_())
    n.fill_diagonal_(0.0)
    Z = n.sum()
    w = (e * P - n / Z) * n
    grad = 4.0 * (w.sum(1, keepdim=True) * Y - w @ Y)
    inc = update * grad < 0
    gains.copy_(torch.where(inc, gains + 0.2, gains * 0.8).clamp_(min=0.01))
    update.mul_(momentum).sub_(lr * gains * grad)
    Y.add_(update)
    return grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="iterations per timed call of run")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--perplexity", type=float, default=100.0)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--sklearn-max-points", type=int, default=8192)
    ap.add_argument("--out", help="also write the JSON report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsne needs an MI355X")
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import latent as L
    dev = torch.device("cuda", 0)
    report = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds,
              "perplexity": args.perplexity, "sizes": {}}
    with torch.no_grad():
        for name, N, d in SIZES:
            X = points(N, d, dev)
            ws = L.workspace(N, dev)
            D = L.sqdist(X)
            P, _ = L.affinities(D, args.perplexity, ws)
            Y0 = (L.random_init(N, 2) * 1e4).to(dev)          # unit scale: past the first iterations
            lr, e = 200.0, 12.0

            def state():
                return Y0.clone(), torch.zeros_like(Y0), torch.ones_like(Y0)

            # the two routes give the same gradient
            Y, u, g = state()
            L.run(P, Y, u, g, 1, exaggeration=e, learning_rate=1.0, kl_every=0, workspace=ws)
            grad_hip = -u / 0.8
            grad_torch = torch_iteration(P, *state(), e, 0.5, 1.0)
            differ = float((grad_hip - grad_torch).abs().max() / grad_torch.abs().max())
            # two fp32 sums of N terms in different orders: at worst N * 2^-24 of the largest component
            if not differ <= N * 2.0 ** -24:
                raise SystemExit(f"bench_tsne: {name}: the gradients of the two routes differ by {differ:.3e} of the "
                                 f"largest component (bound {N * 2.0 ** -24:.3e})")

            def hip_run():                                      # every call starts from the same state
                s = state()
                L.run(P, *s, args.iters, exaggeration=e, learning_rate=lr, kl_every=0, workspace=ws)
                return s[0]

            def torch_run():
                s = state()
                for _ in range(args.iters):
                    torch_iteration(P, *s, e, 0.5, lr)
                return s[0]

            for fn in (hip_run, torch_run):
                if not bool(torch.isfinite(fn()).all()):
                    raise SystemExit(f"bench_tsne: {name}: {fn.__name__} left non-finite coordinates")
            variants = {
                "sqdist": (lambda: L.sqdist(X), 1),
                "affinities": (lambda: L.affinities(D, args.perplexity, ws), 1),
                "run: per iteration": (hip_run, args.iters),
                "torch: per iteration": (torch_run, args.iters),
            }
            samples = {k: [] for k in variants}
            for fn, _ in variants.values():
                timed(fn, 1)                                        # warm-up of every shape
            for _ in range(args.rounds):
                for k, (fn, per) in variants.items():
                    samples[k].append(timed(fn, 1) / per)
            rows = {k: spread(v) for k, v in samples.items()}
            p_bytes = N * N * 4
            med = statistics.median(samples["run: per iteration"])
            rows["run: per iteration"].update(
                p_matrix_bytes=p_bytes, achieved_bytes_per_s=round(p_bytes / (med * 1e-6), -9),
                share_of_hbm_peak=round(p_bytes / (med * 1e-6) / HBM_PEAK, 4),
                speedup_over_torch=round(statistics.median(samples["torch: per iteration"]) / med, 2))
            entry = {"points": N, "dimensions": d, "variants_us": rows, "gradient_difference_between_routes": differ}
            if not args.no_sklearn and N <= args.sklearn_max_points:
                try:
                    from scipy.spatial.distance import squareform
                    from sklearn.manifold import _t_sne
                except ImportError:
                    entry["sklearn"] = "not importable"
                else:
                    Pc = squareform(P.double().cpu().numpy(), checks=False)
                    params = Y0.double().cpu().numpy().ravel()
                    walls = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        _t_sne._kl_divergence(params, Pc, 1.0, N, 2)
                        walls.append(time.perf_counter() - t0)
                    entry["sklearn"] = dict(spread([w * 1e6 for w in walls], prefix="kl_divergence_host_us_"),
                                            host_cpus=len(os.sched_getaffinity(0)))
            report["sizes"][name] = entry
            del X, D, P, ws
            torch.cuda.empty_cache()
    write_report(report, args.out)


if __name__ == "__main__":
    main()
