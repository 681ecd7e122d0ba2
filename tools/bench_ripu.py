"""Sliding-region acquisition kernels on MI355X (mdil_ss_amd.ripu) at the evaluation shape: label and q
maps of 6 x 512 x 1024, 20 and 27 classes, radii 1, 8 and 32.

    python tools/bench_ripu.py [--batch 6 --height 512 --width 1024 --classes 20 27 --radii 1 8 32 --iters 20] [--out FILE]

``ripu_score`` (criterion ripu: the sum of q and every class count of the window) on the network's own maps
(``acquire_head`` on a randomly initialised network), on one label everywhere and on noise labels;
``ripu_select`` in region mode (r = k, 5 % of every image) and in pixel mode (r = 0, a budget of
``--pixel-picks`` pixels per image) with the time per pick of the image that picked most (the images run side
by side, one work-group each; every call starts from a cleared ``taken`` map, whose memset is inside the
timing); ``ripu_apply`` with every output.  Against, in the same run on the same card: ``acquire_head`` with
label and q map, which writes what these kernels read, and the torch route: ``one_hot`` -> per-class window
shares by ``avg_pool2d`` (count_include_pad=False clips the window as RIPU does) -> entropy -> product with the
pooled uncertainty, in fp32, then ``argmax`` + a masked fill per pick, with its peak memory.  The torch route
computes floats: it is timed, not compared bit for bit.  Timed with device events around ``--iters``
back-to-back calls after a warm-up of every variant; the variants alternate over ``--rounds`` rounds and
report median, min and max.  No GPU: it fails, it does not fall back."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


from tools._bench_common import HBM_PEAK, peak_bytes, spread, timed, write_report  # noqa: E402


def torch_score(label, q, nc, k):
    """RIPU's score by torch ops: [N, nc, H, W] one-hot, window shares, entropy, times the window's mean q."""
    import torch.nn.functional as F
    one = F.one_hot(label.long(), nc).permute(0, 3, 1, 2).float()
    p = F.avg_pool2d(one, 2 * k + 1, 1, k, count_include_pad=False)
    imp = -(p * torch.log(p.clamp(min=1e-12))).sum(1)
    unc = F.avg_pool2d(q.float()[:, None], 2 * k + 1, 1, k, count_include_pad=False)[:, 0]
    return imp * unc


def torch_picks(score, r, picks):
    """``picks`` greedy picks on image 0 by ``argmax`` + a masked fill of the region; one host round trip each."""
    s = score[0].clone()
    H, W = s.shape
    for _ in range(picks):
        i = int(s.argmax())
        y, x = divmod(i, W)
        s[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = -1.0
    return s


def one_width(nc, args, dev):
    from mdil_ss_amd import acquire as A
    from mdil_ss_amd import ripu as P
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    N, H, W = args.batch, args.height, args.width
    npix = N * H * W
    torch.manual_seed(0)
    model = Net([nc], 1, 0).to(dev).eval()
    images = torch.rand(N, 3, H, W, device=dev)
    with torch.no_grad():
        feat = model.features(images, 0).contiguous()
        w, b = (t.detach().contiguous() for t in model.head_params(0))
        label, qmap = A.acquire_head(feat, w, b, (2, 2), "entropy", want_label=True, want_qmap=True)
    noise_q = torch.randint(0, 65536, (N, H, W), device=dev, dtype=torch.int32).to(torch.int16).view(torch.uint16)
    inputs = {"network maps": (label, qmap), "one label": (torch.zeros_like(label), qmap),
              "noise labels": (torch.randint(0, nc, (N, H, W), device=dev, dtype=torch.uint8), noise_q)}
    target = torch.randint(0, nc, (N, H, W), device=dev, dtype=torch.uint8)
    taken = torch.zeros(N, H, W, dtype=torch.uint8, device=dev)
    counters = P.new_apply_counters(nc, dev)
    region_budget, pixel_budget = int(0.05 * H * W), args.pixel_picks

    def select(key, r, budget):
        def fn():
            taken.zero_()
            return P.ripu_select(key, taken, r, budget, P._ripu_lib.MAX_PICKS, picks)
        return fn

    picks = torch.zeros(N, P._ripu_lib.MAX_PICKS, 4, dtype=torch.int64, device=dev)
    variants, per_pick = {}, {}
    variants["acquire_head, network features: label + q"] = \
        lambda: A.acquire_head(feat, w, b, (2, 2), "entropy", want_label=True, want_qmap=True)
    keys = {}
    for k in args.radii:
        for name, (lab, qm) in inputs.items():
            variants[f"ripu_score, k {k}, {name}"] = (lambda lab=lab, qm=qm, k=k: P.ripu_score(lab, k, nc, "ripu", qm))
        for by in ("uncertainty", "impurity"):
            variants[f"ripu_score, k {k}, network maps, by {by}"] = (lambda k=k, by=by: P.ripu_score(label, k, nc, by, qmap))
        keys[k] = P.ripu_score(label, k, nc, "ripu", qmap)
        variants[f"ripu_select, region mode r {k}, 5 % per image"] = select(keys[k], k, region_budget)
        variants[f"torch route score, k {k}, network maps"] = (lambda k=k: torch_score(label, A.q_values(qmap), nc, k))
    variants[f"ripu_select, pixel mode r 0, {pixel_budget} pixels per image"] = select(keys[args.radii[0]], 0, pixel_budget)
    variants["ripu_apply: out + mask + counters"] = \
        lambda: P.ripu_apply(taken, nc, target, None, None, label, nc - 1, 255, counters, want_mask=True)
    score0 = torch_score(label, A.q_values(qmap), nc, args.radii[0])
    variants[f"torch route picks, r {args.radii[0]}, 50 picks on one image"] = lambda: torch_picks(score0, args.radii[0], 50)

    def iters_of(name):
        return 2 if name.startswith("torch") else 3 if name.startswith("ripu_select") else args.iters

    samples = {name: [] for name in variants}
    with torch.no_grad():
        for name, fn in variants.items():
            timed(fn, 1)
        for _ in range(args.rounds):
            for name, fn in variants.items():
                samples[name].append(timed(fn, iters_of(name)))
        for name in variants:                                          # what each select picked, from one more call
            if name.startswith("ripu_select"):
                got = variants[name]()
                torch.cuda.synchronize()
                count = got["count"].cpu()
                per_pick[name] = {"picks_per_image_max": int(count.max()), "picks_total": int(count.sum()),
                                  "shown_total": int(got["shown"].sum()), "stops": got["stop"].cpu().tolist()}
        fused_peak = peak_bytes(lambda: P.ripu_score(label, args.radii[-1], nc, "ripu", qmap))
        torch_peak = peak_bytes(lambda: torch_score(label, A.q_values(qmap), nc, args.radii[-1]))
    med = {name: statistics.median(v) for name, v in samples.items()}
    for name, row in per_pick.items():
        row["us_per_pick"] = round(med[name] / max(1, row["picks_per_image_max"]), 3)
    per_pick["torch route"] = {"us_per_pick": round(med[f"torch route picks, r {args.radii[0]}, 50 picks on one image"] / 50, 3)}
    score_bytes = npix * (1 + 2 + 4)                                   # label and q read once, key written
    apply_bytes = npix * (1 + 1 + 1 + 1 + 1)                           # selected, target, label read; out and mask written
    return {
        "us_per_call": {name: spread(v, 2, "") for name, v in samples.items()},
        "select": per_pick,
        "torch_route_over_ripu_score": {str(k): round(med[f"torch route score, k {k}, network maps"] /
                                                      med[f"ripu_score, k {k}, network maps"], 3) for k in args.radii},
        "ripu_score_over_acquire_head": {str(k): round(med[f"ripu_score, k {k}, network maps"] /
                                                       med["acquire_head, network features: label + q"], 3) for k in args.radii},
        "peak_memory_bytes": {f"ripu_score, k {args.radii[-1]} (the key map)": fused_peak,
                              f"torch route score, k {args.radii[-1]}": torch_peak},
        "algorithmic_bytes": {"ripu_score": score_bytes, "ripu_apply": apply_bytes,
                              "torch route: the one-hot tensor alone, written once": npix * nc * 4},
        "share_of_hbm_peak": dict(
            {f"ripu_score, k {k}, network maps": round(score_bytes / (med[f"ripu_score, k {k}, network maps"] * 1e-6) / HBM_PEAK, 4)
             for k in args.radii},
            **{"ripu_apply": round(apply_bytes / (med["ripu_apply: out + mask + counters"] * 1e-6) / HBM_PEAK, 4)}),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--classes", type=int, nargs="+", default=[20, 27])
    ap.add_argument("--radii", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--pixel-picks", type=int, default=3000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ripu needs an MI355X")
    import mdil_ss_amd  # noqa: F401
    dev = torch.device("cuda", 0)
    report = {"shape": {"batch": args.batch, "height": args.height, "width": args.width, "radii": args.radii},
              "device": torch.cuda.get_device_name(0), "what": "a randomly initialised network; timings only",
              "classes": {str(nc): one_width(nc, args, dev) for nc in args.classes}}
    write_report(report, args.out)


if __name__ == "__main__":
    main()
