"""The refinement kernel on MI355X (mdil_ss_amd.refine) at the evaluation shape: 6 x 256 x 512 x 16
features, 20 and 27 classes, five mean-field steps at (radius, dilation) = (5, 2) and (3, 1).

    python tools/bench_refine.py [--batch 6 --height 512 --width 1024 --classes 20 27 --iters 10] [--out FILE]

``refine_head`` (label + confidence) against ``predict_head`` (what the refinement adds to a plain
prediction) and against the same result from torch ops on the same device: stored logits, then per
step an ``F.unfold`` of the probabilities, one image at a time, with peak memory for both.  Timed
with device events around ``--iters`` back-to-back calls after a warm-up of every variant; the
variants alternate over ``--rounds`` rounds and report medians.  The operation counts are computed
from the shapes.  No GPU: it fails, it does not fall back."""
import argparse
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


from tools._bench_common import peak_bytes, spread, timed, write_report  # noqa: E402

WINDOWS = ((5, 2), (3, 1))
FP32_PEAK = 157.3e12                                                  # FLOP / s, vector


def torch_route(feat, w, b, images, p):
    """Stored logits -> per image: the window's weights from an unfold of the image, then per step an
    unfold of Q, the weighted sum and a softmax -> labels u8 [N,H,W]."""
    from mdil_ss_amd import ops
    logits = ops.OutFn.apply(feat, w, b).permute(0, 3, 1, 2)
    N, nc, H, W = logits.shape
    r, d = p.radius, p.dilation
    side = 2 * r + 1
    K = side * side
    off = torch.arange(-r, r + 1, device=feat.device, dtype=torch.float32)
    d2 = ((off[:, None] ** 2 + off[None, :] ** 2) * d * d).reshape(K)
    fa, fs = torch.exp(-d2 / (2 * p.theta_alpha ** 2)), torch.exp(-d2 / (2 * p.theta_gamma ** 2))
    fa[K // 2] = fs[K // 2] = 0.0
    fa, fs = p.w_appearance * fa / fa.sum(), p.w_smooth * fs / fs.sum()
    kw = dict(kernel_size=side, dilation=d, padding=r * d)
    out = []
    for n in range(N):
        l, img = logits[n:n + 1], images[n:n + 1]
        di2 = ((F.unfold(img, **kw).view(1, 3, K, H * W) - img.view(1, 3, 1, H * W)) ** 2).sum(1)
        k = fa[None, :, None] * torch.exp(-di2 / (2 * p.theta_beta ** 2)) + fs[None, :, None]
        q = torch.softmax(l, 1)
        for _ in range(p.iterations):
            m = (F.unfold(q, **kw).view(1, nc, K, H * W) * k.unsqueeze(1)).sum(2).view(1, nc, H, W)
            q = torch.softmax(l + m, 1)
        out.append(q.max(1)[1].to(torch.uint8))
    return torch.cat(out)


def one_width(nc, args, dev):
    from mdil_ss_amd import refine as RF
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    from mdil_ss_amd.predict import predict_head
    N, H, W = args.batch, args.height, args.width
    torch.manual_seed(0)
    model = Net([nc], 1, 0).to(dev).eval()
    images = torch.rand(N, 3, H // 8, W // 8, device=dev)
    images = F.interpolate(images, size=(H, W), mode="nearest").add_(0.02 * torch.randn(N, 3, H, W, device=dev)).clamp_(0, 1)
    with torch.no_grad():
        feat = model.features(images, 0).contiguous()
        w, b = (t.detach().contiguous() for t in model.head_params(0))
    npix = N * H * W
    rows = {}
    variants = {"predict_head: label + confidence": lambda: predict_head(feat, w, b, None, True)}
    for r, d in WINDOWS:
        p = RF.RefineParams(radius=r, dilation=d)
        ws = torch.empty(RF.workspace_bytes(N, H // 2, W // 2, nc, p.iterations), dtype=torch.uint8, device=dev)
        variants[f"refine_head r{r} d{d}: label + confidence"] = \
            lambda p=p, ws=ws: RF.refine_head(feat, w, b, images, p, want_confidence=True, workspace=ws)
        variants[f"torch route r{r} d{d}: logits, unfold per step"] = lambda p=p: torch_route(feat, w, b, images, p)
    iters = {k: (1 if k.startswith("torch") else args.iters) for k in variants}
    samples = {k: [] for k in variants}
    with torch.no_grad():
        for k, fn in variants.items():
            timed(fn, 1 if k.startswith("torch") else 2)
        for _ in range(args.rounds):
            for k, fn in variants.items():
                samples[k].append(timed(fn, iters[k]))
        med = {k: statistics.median(v) for k, v in samples.items()}
        for r, d in WINDOWS:
            p = RF.RefineParams(radius=r, dilation=d)
            fused, route = f"refine_head r{r} d{d}: label + confidence", f"torch route r{r} d{d}: logits, unfold per step"
            ours = RF.refine_head(feat, w, b, images, p)[0]
            plain = RF.refine_head(feat, w, b, images, RF.RefineParams(iterations=0))[0]
            theirs = torch_route(feat, w, b, images, p)
            taps = (2 * r + 1) ** 2 - 1
            flop = p.iterations * npix * (taps * (2 * nc + 12) + 32 * nc) + npix * 32 * nc
            rows[f"r{r} d{d}"] = {
                "us_per_call": {"refine_head": spread(samples[fused], 1, ""), "torch route": spread(samples[route], 1, "")},
                "us_per_image_and_step": round(med[fused] / N / p.iterations, 1),
                "torch_route_over_refine_head": round(med[route] / med[fused], 1),
                "refine_head_over_predict_head": round(med[fused] / med["predict_head: label + confidence"], 1),
                "peak_memory_bytes": {
                    "refine_head (workspace, label, confidence)": peak_bytes(
                        lambda: RF.refine_head(feat, w, b, images, p, want_confidence=True)),
                    "torch route": peak_bytes(lambda: torch_route(feat, w, b, images, p))},
                "counted_from_shapes": {
                    "flop": flop, "share_of_fp32_vector_peak": round(flop / (med[fused] * 1e-6) / FP32_PEAK, 4),
                    "lds_bytes_read": p.iterations * npix * taps * (nc + 3) * 4,
                    "q_bytes_per_step_read_and_written": [npix * nc * 4] * 2,
                    "unfold_bytes_per_image_and_step": npix // N * nc * (taps + 1) * 4},
                "labels_differing_from_torch_route": (ours != theirs).float().mean().item(),
                "labels_changed_by_the_refinement": (ours != plain).float().mean().item(),
            }
    return {"predict_head_us": spread(samples["predict_head: label + confidence"], 1, ""), "windows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--classes", type=int, nargs="+", default=[20, 27])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", help="also write the JSON report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_refine needs an MI355X")
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd.refine import DEFAULTS
    dev = torch.device("cuda", 0)
    report = {"shape": {"batch": args.batch, "height": args.height, "width": args.width},
              "device": torch.cuda.get_device_name(0),
              "params": dict(DEFAULTS._asdict(), radius_dilation=[list(w) for w in WINDOWS]),
              "what": "random-weight model on a blocky random image; times are device events, medians over rounds; "
                      "the default CRF parameters are untuned",
              "classes": {str(nc): one_width(nc, args, dev) for nc in args.classes}}
    write_report(report, args.out)


if __name__ == "__main__":
    main()
