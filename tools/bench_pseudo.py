"""Pseudo-label kernels on MI355X (mdil_ss_amd.pseudo) at the evaluation shape: 6 x 256 x 512 x 16
features, 20 and 27 classes.

    python tools/bench_pseudo.py [--batch 6 --height 512 --width 1024 --classes 20 27 --iters 30] [--out FILE]

``pseudo_head`` against ``predict_head(..., want_confidence=True)``, the kernel it extends (the
difference is what the 16-bit store and the histogram cost), on three inputs that load the histogram differently -- the head
as initialised (confidences near 1 / nc: a handful of bins), its weights times 64 (hundreds of bins)
and the worst case for the LDS atomics (one class's bias raised by 30: every pixel in ONE bin); ``refine`` + ``apply`` over the stored maps
against the torch route on the same device (stored logits, ``softmax``, ``max(1)``, per-class
``kthvalue``, ``where``), with peak memory for both; and a PROJECTION for a 2,975-image split from
those per-batch times.  Timed with device events around ``--iters`` back-to-back calls after a
warm-up of every variant; the variants alternate over ``--rounds`` rounds and report medians.
No GPU: it fails, it does not fall back."""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


from tools._bench_common import peak_bytes, spread, timed, write_report  # noqa: E402

PORTION = 0.2
SPLIT_IMAGES = 2975


def torch_route(feat, w, b, nc, portion):
    """Stored logits -> softmax -> max(1) -> per-class kthvalue -> where: the pseudo-label map of one batch."""
    from mdil_ss_amd import ops
    logits = ops.OutFn.apply(feat, w, b).permute(0, 3, 1, 2)
    conf, label = torch.softmax(logits, 1).max(1)
    out = torch.full_like(label, 255)
    for c in range(nc):
        mine = label == c
        n = int(mine.sum())
        k = math.floor(portion * n)
        if k:
            thr = conf[mine].kthvalue(n - k + 1)[0]
            out = torch.where(mine & (conf >= thr), label, out)
    return out.to(torch.uint8)


def one_width(nc, args, dev):
    from mdil_ss_amd import pseudo as P
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    from mdil_ss_amd.predict import predict_head
    N, H, W = args.batch, args.height, args.width
    torch.manual_seed(0)
    model = Net([nc], 1, 0).to(dev).eval()
    images = torch.rand(N, 3, H, W, device=dev)
    with torch.no_grad():
        feat = model.features(images, 0).contiguous()
        w, b = (t.detach().contiguous() for t in model.head_params(0))
    heads = {"as initialised": (w, b), "weights x 64": ((w * 64).contiguous(), b), "one bin": (w, b + 30 * (torch.arange(nc, device=dev) == 0))}
    hist = torch.zeros(nc, 256, dtype=torch.int64, device=dev)
    nonf = torch.zeros(1, dtype=torch.int64, device=dev)
    hists = {}
    for name, (weight, bias) in heads.items():
        hist.zero_()
        P.pseudo_head(feat, weight, bias, hist, nonf, False, False)
        hists[name] = hist.cpu()
    label, qconf = P.pseudo_head(feat, w, b)
    hist2 = torch.zeros(nc, 256, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)

    def refine(sel):
        hist2.zero_()
        P.pseudo_refine(label, qconf, nc, sel, hist2, bad)
        return hist2.cpu()

    thr = P.thresholds(hists["as initialised"], refine, PORTION)
    sel = torch.tensor([t >> 8 if t < P.Q_ONE else -1 for t in thr], dtype=torch.int32).to(dev)
    thr_d = torch.tensor(thr, dtype=torch.int32).to(dev)
    counters = P.new_apply_counters(nc, dev)
    seen_kept = {k: counters[k] for k in ("seen", "kept")}
    variants = {
        "predict_head: label + confidence": lambda: predict_head(feat, w, b, None, True),
        "pseudo_head as initialised: label + qconf": lambda: P.pseudo_head(feat, w, b),
        "pseudo_head as initialised: label + qconf + hist": lambda: P.pseudo_head(feat, w, b, hist, nonf),
        "pseudo_head weights x 64: label + qconf + hist": lambda: P.pseudo_head(feat, *heads["weights x 64"], hist, nonf),
        "pseudo_head one bin: label + qconf + hist": lambda: P.pseudo_head(feat, *heads["one bin"], hist, nonf),
        "pseudo_head as initialised: hist only": lambda: P.pseudo_head(feat, w, b, hist, nonf, False, False),
        "pseudo_refine": lambda: P.pseudo_refine(label, qconf, nc, sel, hist2, bad),
        "pseudo_apply: out + seen + kept": lambda: P.pseudo_apply(label, qconf, nc, thr_d, counters=seen_kept),
        "torch route: logits, softmax, max, kthvalue, where": lambda: torch_route(feat, w, b, nc, PORTION),
    }
    iters = {k: (3 if k.startswith("torch") else args.iters) for k in variants}
    samples = {k: [] for k in variants}
    with torch.no_grad():
        for k, fn in variants.items():
            timed(fn, 2)
        for _ in range(args.rounds):
            for k, fn in variants.items():
                samples[k].append(timed(fn, iters[k]))
        fused_peak = peak_bytes(lambda: (P.pseudo_head(feat, w, b, hist, nonf),
                                         P.pseudo_apply(label, qconf, nc, thr_d, counters=seen_kept)))
        torch_peak = peak_bytes(lambda: torch_route(feat, w, b, nc, PORTION))
        same = torch_route(feat, w, b, nc, PORTION)
        ours = P.pseudo_apply(label, qconf, nc, thr_d)
        differ = (same != ours).float().mean().item()
    med = {k: statistics.median(v) for k, v in samples.items()}
    npix = N * H * W
    batches = math.ceil(SPLIT_IMAGES / N)
    per_batch = med["pseudo_head as initialised: label + qconf + hist"] + med["pseudo_refine"] + \
        med["pseudo_apply: out + seen + kept"]
    busiest = {name: float(h.max() / h.sum()) for name, h in hists.items()}
    occupied = {name: int((h > 0).sum()) for name, h in hists.items()}
    return {
        "us_per_call": {k: spread(v, 2, "") for k, v in samples.items()},
        "pseudo_head_over_predict_head": round(med["pseudo_head as initialised: label + qconf + hist"] /
                                               med["predict_head: label + confidence"], 3),
        "weights_x64_over_as_initialised": round(med["pseudo_head weights x 64: label + qconf + hist"] /
                                     med["pseudo_head as initialised: label + qconf + hist"], 3),
        "one_bin_over_as_initialised": round(med["pseudo_head one bin: label + qconf + hist"] /
                                     med["pseudo_head as initialised: label + qconf + hist"], 3),
        "share_of_pixels_in_the_busiest_bin": busiest,
        "bins_occupied": occupied,
        "peak_memory_bytes": {"pseudo_head + pseudo_apply (label, qconf, out)": fused_peak, "torch route": torch_peak},
        "algorithmic_bytes": {"features read": npix // 4 * 64, "label + qconf written": npix * 3,
                              "predict_head label + confidence written": npix * 5,
                              "refine reads": npix * 3, "apply reads + writes": npix * 4,
                              "torch route: logits written, then read back": [npix * ((nc + 3) // 4 * 4) * 4] * 2},
        "maps_differing_from_torch_route": differ,
        "projection_2975_images": {
            "what": "PROJECTED, not measured: ceil(2975 / batch) x (pseudo_head + refine + apply) medians above; "
                    "the network forward and the PNG writing are not in it",
            "ms": round(batches * per_batch / 1e3, 1),
            "torch_route_ms": round(batches * med["torch route: logits, softmax, max, kthvalue, where"] / 1e3, 1),
            "stored_maps_gb": round(SPLIT_IMAGES * H * W * 3 / 1e9, 2),
        },
    }


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
        raise SystemExit("bench_pseudo needs an MI355X")
    import mdil_ss_amd  # noqa: F401
    dev = torch.device("cuda", 0)
    report = {"shape": {"batch": args.batch, "height": args.height, "width": args.width},
              "device": torch.cuda.get_device_name(0), "portion": PORTION,
              "classes": {str(nc): one_width(nc, args, dev) for nc in args.classes}}
    write_report(report, args.out)


if __name__ == "__main__":
    main()
