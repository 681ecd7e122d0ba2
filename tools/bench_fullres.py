"""Full-resolution head on MI355X: the fused output_conv + bilinear resize + argmax (+ confusion,
+ colour) call (mdil_ss_amd.fullres) against the unfused route it replaces, on the same device and
in the same process: stored logits -> ``F.interpolate(..., mode="bilinear", align_corners=False)``
-> ``max(1)`` (+ ``bincount`` for the confusion matrix), at 6 x 256 x 512 x 16 features ->
1024 x 2048, 20 classes by default.

    python tools/bench_fullres.py [--batch 6 --height 256 --width 512 --out-height 1024 --out-width 2048
                                   --classes 20 --iters 20 --rounds 5] [--out FILE]

Timed with device events around ``--iters`` back-to-back calls after a warm-up of every variant;
the variants alternate over ``--rounds`` rounds and each reports its median and spread.  The
unfused route is timed twice: from the stored logits (what the issue of storing them costs is left
out) and from the features (with the project's output_conv in front, which the fused call contains).
Bytes are what each route must move, computed from the shapes, over the median time as a share of
the 8 TB/s HBM peak; peak memory is the allocator's high-water mark of one call above what was
allocated before it.  No GPU: it fails, it does not fall back."""
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
    ap.add_argument("--height", type=int, default=256, help="feature height (half the network's)")
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--out-height", type=int, default=1024)
    ap.add_argument("--out-width", type=int, default=2048)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fullres needs an MI355X")
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import ops
    from mdil_ss_amd.fullres import fullres_head
    from mdil_ss_amd.predict import default_palette
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    nc, N, H, W, Ho, Wo = args.classes, args.batch, args.height, args.width, args.out_height, args.out_width
    size = (Ho, Wo)
    feat = F.relu(torch.randn(N, H, W, 16, device=dev, generator=g))
    w = torch.randn(16, nc, 2, 2, device=dev, generator=g) * 0.3
    b = torch.randn(nc, device=dev, generator=g) * 0.2
    target = torch.randint(0, nc, (N, Ho, Wo), device=dev, generator=g, dtype=torch.uint8)
    pal = default_palette(nc).to(dev)
    conf = torch.zeros(nc, nc, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)

    def logits_of():                                      # NCHW view of the stored NHWC logits
        return ops.OutFn.apply(feat, w, b).permute(0, 3, 1, 2)[:, :nc]

    def unfused_label(lg):
        return F.interpolate(lg, size, mode="bilinear", align_corners=False).max(1)[1]

    def unfused_confusion(lg):
        pred = unfused_label(lg)
        return pred, torch.bincount(target.view(-1).long() * nc + pred.view(-1), minlength=nc * nc)

    def unfused_colour(lg):
        pred = unfused_label(lg)
        return pred, pal[pred]

    with torch.no_grad():
        stored = logits_of()
        variants = {
            "fused: label": lambda: fullres_head(feat, w, b, size),
            "fused: label + confusion": lambda: fullres_head(feat, w, b, size, target=target, ignore_index=nc - 1,
                                                             confusion=conf, bad_targets=bad),
            "fused: label + colour": lambda: fullres_head(feat, w, b, size, palette=pal),
            "unfused from stored logits: label": lambda: unfused_label(stored),
            "unfused from stored logits: label + confusion": lambda: unfused_confusion(stored),
            "unfused from stored logits: label + colour": lambda: unfused_colour(stored),
            "unfused from features: label": lambda: unfused_label(logits_of()),
            "unfused from features: label + confusion": lambda: unfused_confusion(logits_of()),
            "unfused from features: label + colour": lambda: unfused_colour(logits_of()),
        }
        # same labels from both routes, up to fp32 near-ties (tests/test_fullres_gpu.py has the bound)
        differ = (fullres_head(feat, w, b, size)[0].long() != unfused_label(stored)).float().mean().item()
        samples = {k: [] for k in variants}
        for fn in variants.values():
            timed(fn, 3)
        peaks = {k: peak_bytes(fn) for k, fn in variants.items()}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                samples[k].append(timed(fn, args.iters))
    npf, npl, npo = N * H * W, N * 4 * H * W, N * Ho * Wo
    lg_b, up_b = npl * stored.shape[1] * 4, npo * nc * 4              # logits, resized logits
    extra = {"label": 0, "label + confusion": npo, "label + colour": npo * 3}
    unf_extra = {"label": 0, "label + confusion": npo * (1 + 8 + 8 + 8), "label + colour": npo * (8 + 3)}
    bytes_moved = {}
    for kind in extra:
        bytes_moved[f"fused: {kind}"] = npf * 64 + npo + extra[kind]
        # resized logits written and read back, int64 labels and fp32 maxima written
        stored_route = lg_b + 2 * up_b + npo * 12 + unf_extra[kind]
        bytes_moved[f"unfused from stored logits: {kind}"] = stored_route
        bytes_moved[f"unfused from features: {kind}"] = stored_route + npf * 64 + lg_b
    rows = variant_rows(samples, bytes_moved, peaks)
    report = {
        "shape": {"batch": N, "feature_height": H, "feature_width": W, "out_height": Ho, "out_width": Wo, "classes": nc},
        "device": torch.cuda.get_device_name(0),
        "iters": args.iters, "rounds": args.rounds,
        "variants": rows,
        "fused_fma_per_call": npo * nc * 64,
        "labels_differing_between_routes": differ,
    }
    write_report(report, args.out)


if __name__ == "__main__":
    main()
