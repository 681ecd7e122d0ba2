"""Drift head on MI355X: the fused twin-head call (mdil_ss_amd.drift) against the unfused torch route
it replaces, on the same device and in the same process: two stored-logit heads -> two
``log_softmax`` -> the KL sum -> two ``max(1)`` -> ``bincount``, at 6 x 256 x 512 x 16 features,
20 and 27 classes by default.

    python tools/bench_drift.py [--batch 6 --height 256 --width 512 --classes 20 27 --iters 20 --rounds 5]
                                [--out FILE]

The two routes' outputs are compared first, and the tool fails if they disagree: the labels may
differ at fp32 near-ties only (at most 0.1 % of the pixels, the cap of tests/test_drift_gpu.py), the
transition counts by no more than those pixels move, and the KL maps by no more than both routes'
tolerances against the fp64 value together (tests/test_drift_gpu.py: the kernel is held to 4 x the
torch route's measured constant, so 5 x that constant between the two).

Timed with device events around ``--iters`` back-to-back calls after a warm-up of every variant; the
variants alternate over ``--rounds`` rounds and each reports its median and spread.  The unfused
route is timed twice: from the stored logits (what storing them costs is left out) and from the
features (with the project's output_conv in front, twice, which the fused call contains).  Bytes are
what each route must move, computed from the shapes, over the median time as a share of the 8 TB/s
HBM peak; peak memory is the allocator's high-water mark of one call above what was allocated before
it.  No GPU: it fails, it does not fall back."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools._bench_common import peak_bytes, timed, variant_rows, write_report  # noqa: E402

K_KL_TORCH = 3.034                       # tests/test_drift_gpu.py
MAX_LABELS_DIFFERING = 1e-3


def bench(nc, N, H, W, iters, rounds, dev):
    from mdil_ss_amd import ops
    from mdil_ss_amd.drift import drift_head, workspace_bytes
    g = torch.Generator(device=dev).manual_seed(nc)
    fa = F.relu(torch.randn(N, H, W, 16, device=dev, generator=g))
    wa = torch.randn(16, nc, 2, 2, device=dev, generator=g) * 0.3
    ba = torch.randn(nc, device=dev, generator=g) * 0.2
    fb = fa + 0.1 * F.relu(torch.randn(N, H, W, 16, device=dev, generator=g))
    wb = wa + 0.05 * torch.randn(16, nc, 2, 2, device=dev, generator=g) * 0.3
    bb = ba.clone()
    target = torch.randint(0, nc, (N, 2 * H, 2 * W), device=dev, generator=g, dtype=torch.uint8)
    z = lambda *s: torch.zeros(s, dtype=torch.int64, device=dev)  # noqa: E731
    counters = {"transition": z(nc, nc), "bad_targets": z(1), "sums": torch.zeros(nc + 1, dtype=torch.float64, device=dev),
                "workspace": torch.empty(workspace_bytes(N, H, W, nc) // 8, dtype=torch.float64, device=dev)}
    scored = dict(counters, confusion_a=z(nc, nc), confusion_b=z(nc, nc), outcome=z(nc, 4))
    heads = (fa, wa, ba, fb, wb, bb)

    def logits_of(f, w, b):                               # NCHW view of the stored NHWC logits
        return ops.OutFn.apply(f, w, b).permute(0, 3, 1, 2)[:, :nc]

    def unfused(la, lb, with_target=False):
        za, zb = F.log_softmax(la, 1), F.log_softmax(lb, 1)
        kl = (za.exp() * (za - zb)).sum(1)
        pa, pb = la.max(1)[1], lb.max(1)[1]
        out = [kl, pa, pb, torch.bincount(pa.view(-1) * nc + pb.view(-1), minlength=nc * nc)]
        if with_target:
            t = target.view(-1).long()
            out += [torch.bincount(t * nc + pa.view(-1), minlength=nc * nc),
                    torch.bincount(t * nc + pb.view(-1), minlength=nc * nc)]
        return out

    with torch.no_grad():
        sa, sb = logits_of(*heads[:3]), logits_of(*heads[3:])
        # ---- the two routes agree
        fused = drift_head(*heads, labels=True, kl=True, counters={"transition": z(nc, nc)})
        transition = z(nc, nc)
        drift_head(*heads, counters={"transition": transition})
        kl_u, pa_u, pb_u, trans_u = unfused(sa, sb)
        differing = (fused["label_a"].long() != pa_u) | (fused["label_b"].long() != pb_u)
        share = differing.float().mean().item()
        moved = int((transition.view(-1) - trans_u).abs().sum())
        Sa = logits_of(fa.abs(), wa.abs(), ba.abs()).max(1)[0]
        Sb = logits_of(fb.abs(), wb.abs(), bb.abs()).max(1)[0]
        za, zb = F.log_softmax(sa, 1), F.log_softmax(sb, 1)
        tol = 2.0 ** -24 * (1 + Sa + Sb) * (1 + (za.exp() * (za - zb).abs()).sum(1))
        kl_constant = ((fused["kl"] - kl_u).abs() / tol).max().item()
        del za, zb, tol, Sa, Sb
        if share > MAX_LABELS_DIFFERING or moved > 2 * int(differing.sum()) or not kl_constant <= 5 * K_KL_TORCH:
            raise SystemExit(f"bench_drift: the routes disagree at {nc} classes: labels differ at {share:.2e} of the "
                             f"pixels, {moved} transition counts moved for {int(differing.sum())} pixels, kl maps "
                             f"apart by {kl_constant:.2f} tolerance units (allowed {5 * K_KL_TORCH:.2f})")
        # ---- time
        variants = {
            "fused: transition + sums": lambda: drift_head(*heads, counters=counters),
            "fused: all counters against a target": lambda: drift_head(*heads, target=target, ignore_index=nc - 1,
                                                                       counters=scored),
            "fused: all counters + labels, kl and change maps": lambda: drift_head(
                *heads, target=target, ignore_index=nc - 1, labels=True, kl=True, change=True, counters=scored),
            "unfused from stored logits: kl + labels + transition": lambda: unfused(sa, sb),
            "unfused from stored logits: + both confusion matrices": lambda: unfused(sa, sb, True),
            "unfused from features: kl + labels + transition": lambda: unfused(logits_of(*heads[:3]), logits_of(*heads[3:])),
        }
        samples = {k: [] for k in variants}
        for fn in variants.values():
            timed(fn, 3)
        peaks = {k: peak_bytes(fn) for k, fn in variants.items()}
        for _ in range(rounds):
            for k, fn in variants.items():
                samples[k].append(timed(fn, iters))
    npf, npl = N * H * W, N * 4 * H * W
    lg = npl * sa.shape[1] * 4                            # one stored logit tensor
    # unfused: log_softmax reads and writes each tensor (4 lg); exp, the difference and the product are
    # one pass each over two or three tensors (2 + 3 + 3 lg); the sum reads one (1 lg); two max(1) read
    # both (2 lg) and write int64 labels and fp32 maxima; bincount reads two int64 maps and writes one
    stored = 15 * lg + npl * 4 + 2 * npl * 12 + npl * 24
    bytes_moved = {
        "fused: transition + sums": 2 * npf * 64,
        "fused: all counters against a target": 2 * npf * 64 + npl,
        "fused: all counters + labels, kl and change maps": 2 * npf * 64 + npl + npl * (1 + 1 + 1 + 4),
        "unfused from stored logits: kl + labels + transition": stored,
        "unfused from stored logits: + both confusion matrices": stored + npl * (1 + 8 + 2 * 24),
        "unfused from features: kl + labels + transition": stored + 2 * (npf * 64 + lg),
    }
    return {"variants": variant_rows(samples, bytes_moved, peaks), "stored_logits_bytes_each": lg,
            "fused_fma_per_call_three_walks": npl * nc * 16 * 2 * 3, "labels_differing_between_routes": share,
            "transition_counts_moved": moved, "kl_maps_apart_in_tolerance_units": round(kl_constant, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--height", type=int, default=256, help="feature height (half the network's)")
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--classes", type=int, nargs="+", default=[20, 27])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_drift needs an MI355X")
    import mdil_ss_amd  # noqa: F401
    dev = torch.device("cuda", 0)
    report = {
        "shape": {"batch": args.batch, "feature_height": args.height, "feature_width": args.width},
        "device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds,
        "classes": {str(nc): bench(nc, args.batch, args.height, args.width, args.iters, args.rounds, dev)
                    for nc in args.classes},
    }
    write_report(report, args.out)


if __name__ == "__main__":
    main()
