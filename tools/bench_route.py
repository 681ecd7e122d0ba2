"""Routing kernels on MI355X (mdil_ss_amd.route) at the evaluation shape: 6 x 3 x 512 x 1024 images for
the stem, 6 x 256 x 512 x 16 features for the head at 20 and 27 classes.

    python tools/bench_route.py [--batch 6 --height 512 --width 1024 --classes 20 27 --iters 30] [--out FILE]

``stem_moments`` against the dense torch route on the same device (``conv2d``, ``max_pool2d``,
``cat``, then per-image mean and variance), with the stem call's algorithmic bytes (the image read
once) over its median as a share of the HBM peak, for the wrapper and for the C entry point called
with outputs and workspace allocated once (what the wrapper's host work costs); ``route_head``
against stored logits (``F.conv_transpose2d``) -> ``softmax`` -> entropy / ``max`` / ``topk(2)`` ->
per-image sums; peak memory for every variant.
Timed with device events around ``--iters`` back-to-back calls after a warm-up of every variant;
the variants alternate over ``--rounds`` rounds and report medians.  No ratio is a target here: the
report says what came out.  No GPU: it fails, it does not fall back."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


from tools._bench_common import HBM_PEAK, peak_bytes, spread, timed, write_report  # noqa: E402


def torch_stem(images, w, b):
    """conv2d, max_pool2d, cat, per-image mean and variance of the 16 channels -> [N,16,2]."""
    act = torch.cat([F.conv2d(images, w, b, stride=2, padding=1), F.max_pool2d(images, 2)], 1)
    var, mean = torch.var_mean(act, (2, 3), unbiased=False)
    return torch.stack([mean, var], 2)


def torch_head(feat, w, b):
    """Stored logits (``F.conv_transpose2d`` on the NCHW view of the features) -> ``softmax`` -> entropy
    (``special.entr``: -p ln p, 0 at p = 0) / ``max`` / ``topk(2)`` -> per-image sums [N,3]."""
    logits = F.conv_transpose2d(feat.permute(0, 3, 1, 2), w, b, stride=2)
    p = F.softmax(logits, 1)
    conf = p.max(1)[0]
    top = p.topk(2, dim=1)[0]
    return torch.stack([torch.special.entr(p).sum(1).sum((1, 2)), conf.sum((1, 2)),
                        (top[:, 0] - top[:, 1]).sum((1, 2))], 1)


def run(variants, slow, args):
    """-> ({name: samples}, {name: peak bytes}) after a warm-up of every variant."""
    samples = {k: [] for k in variants}
    with torch.no_grad():
        for fn in variants.values():
            timed(fn, 2)
        for _ in range(args.rounds):
            for k, fn in variants.items():
                samples[k].append(timed(fn, 3 if k in slow else args.iters))
        peaks = {k: peak_bytes(fn) for k, fn in variants.items()}
    return samples, peaks


def stem(args, dev):
    from mdil_ss_amd import _route_lib
    from mdil_ss_amd import route as P
    N, H, W = args.batch, args.height, args.width
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(3, 13, (3, 3), stride=2, padding=1).to(dev)
    w, b = conv.weight.detach().contiguous(), conv.bias.detach().contiguous()
    images = torch.rand(N, 3, H, W, device=dev)
    lib = _route_lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    mom = torch.empty(N, 16, 2, dtype=torch.float64, device=dev)
    ws = torch.empty(P.stem_workspace_bytes(N, H, W) // 8, dtype=torch.float64, device=dev)
    direct = lambda: lib.mdil_route_stem(images.data_ptr(), w.data_ptr(), b.data_ptr(), N, H, W, mom.data_ptr(), None,  # noqa: E731
                                         None, ws.data_ptr(), ws.numel() * 8, stream)
    variants = {"stem_moments": lambda: P.stem_moments(images, w, b),
                "mdil_route_stem, outputs and workspace allocated once": direct,
                "stem_moments + act": lambda: P.stem_moments(images, w, b, act=True),
                "torch route: conv2d, max_pool2d, cat, var_mean": lambda: torch_stem(images, w, b)}
    samples, peaks = run(variants, (), args)
    with torch.no_grad():
        m = P.stem_moments(images, w, b)[0]
        n = (H // 2) * (W // 2)
        mean = m[:, :, 0] / n
        ours = torch.stack([mean, m[:, :, 1] / n - mean * mean], 2)
        theirs = torch_stem(images, w, b).double()
    image_bytes = N * 3 * H * W * 4
    med = statistics.median(samples["stem_moments"])
    med_direct = statistics.median(samples["mdil_route_stem, outputs and workspace allocated once"])
    return {"us_per_call": {k: spread(v, 2, "") for k, v in samples.items()}, "peak_memory_bytes": peaks,
            "algorithmic_bytes": {"image read": image_bytes, "act written (on request)": N * n * 64,
                                  "torch route: act written, then read back": [N * n * 64] * 2},
            "stem_moments_share_of_hbm_peak": round(image_bytes / (med * 1e-6) / HBM_PEAK, 4),
            "mdil_route_stem_share_of_hbm_peak": round(image_bytes / (med_direct * 1e-6) / HBM_PEAK, 4),
            "torch_route_over_stem_moments": round(statistics.median(samples["torch route: conv2d, max_pool2d, cat, "
                                                                             "var_mean"]) / med, 3),
            "worst_mean_variance_difference_from_torch_route": float((ours - theirs).abs().max())}


def head(nc, args, dev):
    from mdil_ss_amd import _route_lib
    from mdil_ss_amd import route as P
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    N, H, W = args.batch, args.height, args.width
    torch.manual_seed(0)
    model = Net([nc], 1, 0).to(dev).eval()
    with torch.no_grad():
        feat = model.features(torch.rand(N, 3, H, W, device=dev), 0).contiguous()
        w, b = (t.detach().contiguous() for t in model.head_params(0))
    lib = _route_lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    sc = torch.empty(N, 3, dtype=torch.float64, device=dev)
    ws = torch.empty(P.head_workspace_bytes(N, H // 2, W // 2, nc) // 8, dtype=torch.float64, device=dev)
    direct = lambda: lib.mdil_route_head(feat.data_ptr(), w.data_ptr(), b.data_ptr(), N, H // 2, W // 2, nc, None, None,  # noqa: E731
                                         None, None, sc.data_ptr(), None, ws.data_ptr(), ws.numel() * 8, stream)
    variants = {"route_head: scores": lambda: P.route_head(feat, w, b, label=False),
                "mdil_route_head: scores, outputs and workspace allocated once": direct,
                "route_head: label + scores": lambda: P.route_head(feat, w, b),
                "route_head: label + three maps + scores": lambda: P.route_head(feat, w, b, maps=True),
                "torch route: logits, softmax, entropy, topk(2), sums": lambda: torch_head(feat, w, b)}
    slow = ("torch route: logits, softmax, entropy, topk(2), sums",)
    samples, peaks = run(variants, slow, args)
    with torch.no_grad():
        ours = P.route_head(feat, w, b, label=False)["scores"]
        theirs = torch_head(feat, w, b).double()
    npix = N * H * W
    med = {k: statistics.median(v) for k, v in samples.items()}
    return {"us_per_call": {k: spread(v, 2, "") for k, v in samples.items()}, "peak_memory_bytes": peaks,
            "algorithmic_bytes": {"features read": npix // 4 * 64, "label written": npix, "three maps written": npix * 12,
                                  "torch route: logits written, then read back": [npix * ((nc + 3) // 4 * 4) * 4] * 2},
            "torch_route_over_route_head": round(med[slow[0]] / med["route_head: label + scores"], 3),
            "worst_relative_score_difference_from_torch_route": float(((ours - theirs).abs() / theirs.abs()).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--classes", type=int, nargs="+", default=[20, 27])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_route needs an MI355X")
    import mdil_ss_amd  # noqa: F401
    dev = torch.device("cuda", 0)
    report = {"shape": {"batch": args.batch, "height": args.height, "width": args.width},
              "device": torch.cuda.get_device_name(0), "stem": stem(args, dev),
              "head": {str(nc): head(nc, args, dev) for nc in args.classes}}
    write_report(report, args.out)


if __name__ == "__main__":
    main()
