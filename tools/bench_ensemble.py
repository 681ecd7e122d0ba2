"""Ensemble head on MI355X: the fused multi-view call (mdil_ss_amd.ensemble: per view output_conv +
un-mirroring + bilinear resize, then the vote + argmax, + confusion, + confidence) against the
unfused route it replaces, on the same device and in the same process -- per view the stored logits
-> ``flip`` (mirrored views) -> ``F.interpolate(..., mode="bilinear", align_corners=False)`` ->
``softmax`` (prob mode) -> running sum; then ``max(1)`` (+ ``bincount``) -- and against ``nviews``
calls of the single-view ``fullres_head`` on the same features, the yardstick of what the gathers
and the 64-FMA chains alone cost.  Default: 6 views at batch 6 into 1024 x 2048 with 20 classes,
features 192 x 384, 256 x 512 and 320 x 640 (scales 0.75 / 1 / 1.25 of a 512 x 1024 input), each
plain and mirrored.

    python tools/bench_ensemble.py [--batch 6 --height 256 --width 512 --scales 0.75 1 1.25 --no-flip
                                    --out-height 1024 --out-width 2048 --classes 20 --iters 20 --rounds 5]
                                   [--out FILE]

Timed with device events around ``--iters`` back-to-back calls after a warm-up of every variant;
the variants alternate over ``--rounds`` rounds and each reports its median and spread.  Bytes are
what each route must move, computed from the shapes, over the median time as a share of the 8 TB/s
HBM peak; peak memory is the allocator's high-water mark of one call above what was allocated
before it.  The fused call must come out faster than the unfused route and its peak memory below
one view's resized logits: the tool fails otherwise.  No GPU: it fails, it does not fall back."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools._bench_common import peak_bytes, timed, variant_rows, write_report  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--height", type=int, default=256, help="feature height at scale 1 (half the network's)")
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--scales", type=float, nargs="+", default=[0.75, 1.0, 1.25])
    ap.add_argument("--no-flip", action="store_true", help="plain views only")
    ap.add_argument("--out-height", type=int, default=1024)
    ap.add_argument("--out-width", type=int, default=2048)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble needs an MI355X")
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import ops
    from mdil_ss_amd.ensemble import ensemble_head
    from mdil_ss_amd.fullres import fullres_head
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    nc, N, Ho, Wo = args.classes, args.batch, args.out_height, args.out_width
    size = (Ho, Wo)
    shapes = [(4 * round(s * args.height / 4), 4 * round(s * args.width / 4)) for s in args.scales]
    views = [(F.relu(torch.randn(N, h, w_, 16, device=dev, generator=g)), m)
             for h, w_ in shapes for m in ((False,) if args.no_flip else (False, True))]
    nv = len(views)
    w = torch.randn(16, nc, 2, 2, device=dev, generator=g)
    b = torch.randn(nc, device=dev, generator=g) * 0.2
    target = torch.randint(0, nc, (N, Ho, Wo), device=dev, generator=g, dtype=torch.uint8)
    conf = torch.zeros(nc, nc, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    counted = dict(target=target, ignore_index=nc - 1, confusion=conf, bad_targets=bad)

    def unfused(stored, mode, with_confusion):
        total = None
        for lg, (_, mirrored) in zip(stored, views):
            up = F.interpolate(lg.flip(3) if mirrored else lg, size, mode="bilinear", align_corners=False)
            if mode == "prob":
                up = up.softmax(1)
            total = up if total is None else total.add_(up)
        best, pred = total.max(1)
        if with_confusion:
            return pred, torch.bincount(target.view(-1).long() * nc + pred.view(-1), minlength=nc * nc)
        return pred, best

    with torch.no_grad():
        # NCHW views of the stored NHWC logits, as the shipped forward leaves them
        stored = [ops.OutFn.apply(f, w, b).permute(0, 3, 1, 2)[:, :nc] for f, _ in views]
        variants = {}
        for mode in ("prob", "logit"):
            variants[f"fused {mode}: label"] = lambda mode=mode: ensemble_head(views, w, b, size, mode=mode)
            variants[f"fused {mode}: label + confusion"] = \
                lambda mode=mode: ensemble_head(views, w, b, size, mode=mode, **counted)
            variants[f"fused {mode}: label + confusion + confidence"] = \
                lambda mode=mode: ensemble_head(views, w, b, size, mode=mode, confidence=True, **counted)
            variants[f"unfused {mode} from stored logits: label"] = lambda mode=mode: unfused(stored, mode, False)
            variants[f"unfused {mode} from stored logits: label + confusion"] = \
                lambda mode=mode: unfused(stored, mode, True)
        variants[f"{nv} x fullres_head: labels"] = lambda: [fullres_head(f, w, b, size) for f, _ in views]
        differ = {mode: (ensemble_head(views, w, b, size, mode=mode)[0].long()
                         != unfused(stored, mode, False)[0]).float().mean().item() for mode in ("prob", "logit")}
        samples = {k: [] for k in variants}
        for fn in variants.values():
            timed(fn, 2)
        peaks = {k: peak_bytes(fn) for k, fn in variants.items()}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                samples[k].append(timed(fn, args.iters))
    npo = N * Ho * Wo
    up_b = npo * nc * 4                                                   # one view's resized logits
    feat_b = sum(f.numel() * 4 for f, _ in views)
    lg_b = [lg.shape[0] * lg.shape[2] * lg.shape[3] * nc * 4 for lg in stored]
    bytes_moved = {}
    for mode in ("prob", "logit"):
        bytes_moved[f"fused {mode}: label"] = feat_b + npo
        bytes_moved[f"fused {mode}: label + confusion"] = feat_b + 2 * npo
        bytes_moved[f"fused {mode}: label + confusion + confidence"] = feat_b + 6 * npo
        # per view: logits read (mirrored: flipped copy written and read too), resized logits written,
        # softmax reads and writes them, the running sum reads both and writes one (not the first view);
        # then max(1) reads the sum and writes int64 labels and fp32 maxima
        route = sum(lb * (3 if m else 1) for lb, (_, m) in zip(lg_b, views)) \
            + nv * up_b * (1 + (2 if mode == "prob" else 0)) + (nv - 1) * 3 * up_b + up_b + npo * 12
        bytes_moved[f"unfused {mode} from stored logits: label"] = route
        bytes_moved[f"unfused {mode} from stored logits: label + confusion"] = route + npo * (1 + 8 + 8 + 8)
    bytes_moved[f"{nv} x fullres_head: labels"] = feat_b + nv * npo
    rows = variant_rows(samples, bytes_moved, peaks)
    yard = rows[f"{nv} x fullres_head: labels"]["us_median"]
    report = {
        "shape": {"batch": N, "features": [list(s) for s in shapes], "flip": not args.no_flip, "views": nv,
                  "out_height": Ho, "out_width": Wo, "classes": nc},
        "device": torch.cuda.get_device_name(0),
        "iters": args.iters, "rounds": args.rounds,
        "variants": rows,
        "fused_fma_per_call": nv * npo * nc * 64,
        "one_view_resized_logits_bytes": up_b,
        "fused_over_unfused": {mode: round(rows[f"fused {mode}: label"]["us_median"]
                                           / rows[f"unfused {mode} from stored logits: label"]["us_median"], 4)
                               for mode in ("prob", "logit")},
        "fused_over_nviews_fullres": {mode: round(rows[f"fused {mode}: label"]["us_median"] / yard, 4)
                                      for mode in ("prob", "logit")},
        "labels_differing_between_routes": differ,
    }
    write_report(report, args.out)
    for mode in ("prob", "logit"):
        for kind in ("label", "label + confusion"):
            fused, unf = rows[f"fused {mode}: {kind}"], rows[f"unfused {mode} from stored logits: {kind}"]
            if fused["us_median"] >= unf["us_median"]:
                raise SystemExit(f"fused {mode} ({kind}) took {fused['us_median']} us, the unfused route "
                                 f"{unf['us_median']} us: the fused call must be faster")
        for k, row in rows.items():
            if k.startswith(f"fused {mode}") and row["peak_memory_bytes"] >= up_b:
                raise SystemExit(f"{k}: peak memory {row['peak_memory_bytes']} B is not below one view's resized "
                                 f"logits ({up_b} B)")


if __name__ == "__main__":
    main()
