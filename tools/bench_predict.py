"""Prediction head on MI355X: the fused output_conv + argmax call (mdil_ss_amd.predict) against the
unfused path it replaces (``model(images, task)`` -> stored logits -> ``torch.max(1)``), at the
evaluation shape (batch 6, 1024x512 by default).

    python tools/bench_predict.py [--batch 6 --height 512 --width 1024 --classes 20 --iters 50] [--out FILE]

Timed with device events around ``--iters`` back-to-back calls after a warm-up of every variant;
the variants alternate over ``--rounds`` rounds and each reports its median and spread.  ``head``
rows time the head alone on precomputed decoder features; ``net`` rows the whole forward.  Bytes
are what the algorithm must move, computed from the shapes.  No GPU: it fails, it does not fall back."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


from tools._bench_common import spread, timed, write_report  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_predict needs an MI355X")
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import ops
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    from mdil_ss_amd.predict import default_palette, predict, predict_head
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    nc, N, H, W = args.classes, args.batch, args.height, args.width
    model = Net([nc], 1, 0).to(dev).eval()
    images = torch.rand(N, 3, H, W, device=dev)
    pal = default_palette(nc).to(dev)
    with torch.no_grad():
        feat = model.features(images, 0).contiguous()
        w, b = (t.detach() for t in model.head_params(0))
        variants = {
            "head fused: label": lambda: predict_head(feat, w, b),
            "head fused: label + colour": lambda: predict_head(feat, w, b, pal),
            "head fused: label + colour + confidence": lambda: predict_head(feat, w, b, pal, True),
            "head unfused: output_conv + torch.max(1)": lambda: ops.OutFn.apply(feat, w, b).permute(0, 3, 1, 2).max(1),
            "net fused: predict()": lambda: predict(model, images, 0),
            "net unfused: model() + torch.max(1)": lambda: model(images, 0).max(1),
            "net: features only": lambda: model.features(images, 0),
        }
        # same labels from both paths, up to fp32 near-ties (tests/test_predict_gpu.py has the bound)
        differ = (predict(model, images, 0)[0].long() != model(images, 0).max(1)[1]).float().mean().item()
        samples = {k: [] for k in variants}
        for fn in variants.values():
            timed(fn, 5)
        for _ in range(args.rounds):
            for k, fn in variants.items():
                samples[k].append(timed(fn, args.iters))
    npix = N * (H // 2) * (W // 2)
    r4 = (nc + 3) // 4 * 4
    report = {
        "shape": {"batch": N, "height": H, "width": W, "classes": nc},
        "device": torch.cuda.get_device_name(0),
        "us_per_call": {k: spread(v, 2, "") for k, v in samples.items()},
        "algorithmic_bytes": {
            "features read": npix * 64,
            "fused maps written (label / + colour / + confidence)": [npix * 4, npix * 16, npix * 32],
            "unfused logits written, then read back": [npix * 4 * r4 * 4] * 2,
            "unfused labels written (int64) + max values (fp32)": npix * 4 * 12,
        },
        "labels_differing_between_paths": differ,
    }
    write_report(report, args.out)


if __name__ == "__main__":
    main()
