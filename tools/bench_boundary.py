"""Boundary counters on MI355X: the fused call (mdil_ss_amd.boundary.boundary_count: a row pass and a
column pass over two label maps) against the torch route it replaces, on the same device and in the
same process: per class and per map, ``cap`` iterations of 3x3 erosion with a zero border
(``-max_pool2d(-mask, 3, 1)`` on the zero-padded mask), the band of each width taken when the
iteration passes it, then ``bincount`` for the four counters; at 6 x 1024 x 2048 and 20 classes by
default, for widths [46] (the published 0.02 of the Cityscapes diagonal) and [1, 2, 4, 8, 16, 32].

    python tools/bench_boundary.py [--batch 6 --height 1024 --width 2048 --classes 20 --iters 20 --rounds 5
                                    --torch-iters 1] [--resources FILE] [--out FILE]

Inputs: ``ProceduralSeg`` targets at the native size; the prediction is the ``fullres_head`` label
map of a randomly initialised network on the images at half that size (``realistic``), and one
label everywhere in both maps (``one label``), where every column walk runs to the cap.  Timed with
device events around ``--iters`` back-to-back calls after a warm-up of every variant; the variants
alternate over ``--rounds`` rounds and each reports its median and spread.  Both routes must give
the same counters; the report says whether they did.  Bytes: what the two launches must move through
HBM (both maps in, the run distances out and in again, both maps in again), and what the column walks
load on top of that (16 bytes per step of a lane, counted exactly from the distance maps), which the
caches serve.  No GPU: it fails, it does not fall back."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools._bench_common import HBM_PEAK, peak_bytes, spread, timed, write_report  # noqa: E402

WIDTH_SETS = ((46,), (1, 2, 4, 8, 16, 32))


def torch_route(pred, target, nc, widths, ignore_index):
    """The four counters by iterated erosion, one class and one map at a time."""
    nb, cap = len(widths) + 1, widths[-1]
    bins = []
    for m in (pred, target):
        binmap = torch.full(m.shape, nb - 1, dtype=torch.int64, device=m.device)
        for c in m.unique().tolist():                       # every label has a contour, counted or not
            mask = (m == c)
            e = mask.float().unsqueeze(1)
            for k in range(1, cap + 1):
                e = -F.max_pool2d(-F.pad(e, (1, 1, 1, 1)), 3, 1)
                if k in widths:
                    binmap[mask & (e[:, 0] == 0) & (binmap == nb - 1)] = widths.index(k)
        bins.append(binmap.view(-1))
    kp, kt = bins
    g, q = target.view(-1).long(), pred.view(-1).long()
    ok = (g != ignore_index) & (g < nc) & (q < nc)
    g, q, kp, kt = g[ok], q[ok], kp[ok], kt[ok]
    eq = g == q
    return {"target_hist": torch.bincount(g * nb + kt, minlength=nc * nb).view(nc, nb),
            "pred_hist": torch.bincount(q * nb + kp, minlength=nc * nb).view(nc, nb),
            "both_hist": torch.bincount(g[eq] * nb + torch.maximum(kt, kp)[eq], minlength=nc * nb).view(nc, nb),
            "confusion": torch.bincount((kt * nc + g) * nc + q, minlength=nb * nc * nc).view(nb, nc, nc)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--height", type=int, default=1024, help="the labels' own height")
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-iters", type=int, default=1, help="calls per timed window of the torch route")
    ap.add_argument("--resources", help="JSON of the kernels' registers / LDS / scratch as the compiler reports them "
                                        "(-Rpass-analysis=kernel-resource-usage), copied into the report")
    ap.add_argument("--out", help="also write the JSON report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_boundary needs an MI355X")
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import boundary as B
    from mdil_ss_amd.dataset import ProceduralSeg
    from mdil_ss_amd.fullres import predict_fullres
    from mdil_ss_amd.models.erfnet_RA_parallel import Net as Net_RAP
    dev = torch.device("cuda", 0)
    nc, N, H, W = args.classes, args.batch, args.height, args.width
    ignore = nc - 1
    ds = ProceduralSeg(N, H, W, nc, seed=12, domain=0)
    items = [ds[i] for i in range(N)]
    target = torch.stack([lab[0] for _, lab in items]).to(torch.uint8).to(dev)
    torch.manual_seed(0)
    model = Net_RAP([nc], 1, 0).to(dev).eval()
    with torch.no_grad():
        images = F.interpolate(torch.stack([im for im, _ in items]).to(dev), (H // 2, W // 2), mode="bilinear",
                               align_corners=False)
        pred = predict_fullres(model, images, 0, (H, W))[0]
    del model, images, items
    flat = torch.full_like(target, 3)
    inputs = {"realistic": (pred, target), "one label": (flat, flat)}
    ws = torch.empty(B.workspace_bytes(N, H, W), dtype=torch.uint8, device=dev)
    npx = N * H * W

    held = {len(w): B.new_counters(nc, len(w) + 1, dev) for w in WIDTH_SETS}      # accumulated into while timing

    def fused(maps, widths, dist=False):
        counters = B.new_counters(nc, len(widths) + 1, dev) if dist else held[len(widths)]
        return B.boundary_count(*maps, nc, widths, ignore_index=ignore, counters=counters, workspace=ws, dist=dist), counters

    variants, walk_bytes, equal = {}, {}, {}
    with torch.no_grad():
        for name, maps in inputs.items():
            for widths in WIDTH_SETS:
                key = f"{name}, widths {list(widths)}"
                variants["fused: " + key] = (lambda m=maps, w=widths: fused(m, w), args.iters)
                variants["torch: " + key] = (lambda m=maps, w=widths: torch_route(*m, nc, w, ignore), args.torch_iters)
                (dp, dt), counters = fused(maps, widths, dist=True)
                steps = sum(int((d.view(N, H, W // 4, 4).amax(-1).long() - 1).sum()) for d in (dp, dt))
                walk_bytes[key] = steps * 16
                want = torch_route(*maps, nc, widths, ignore)
                equal[key] = all(torch.equal(counters[k], want[k]) for k in want)
                del dp, dt, want
        samples = {k: [] for k in variants}
        for fn, _ in variants.values():
            timed(fn, 1)
        peaks = {k: peak_bytes(fn) for k, (fn, _) in variants.items()}
        for _ in range(args.rounds):
            for k, (fn, iters) in variants.items():
                samples[k].append(timed(fn, iters))
    hbm = 8 * npx                                             # rows: 2 in, 2 out; columns: 4 in (first touch)
    rows = {}
    for k, v in samples.items():
        rows[k] = dict(spread(v), peak_memory_bytes=peaks[k])
        if k.startswith("fused: "):
            med = rows[k]["us_median"] * 1e-6
            wb = walk_bytes[k[len("fused: "):]]
            rows[k].update(hbm_bytes=hbm, share_of_hbm_peak=round(hbm / med / HBM_PEAK, 4), walk_load_bytes=wb,
                           walk_load_bytes_per_s=round(wb / med, 1))
    for key in walk_bytes:
        rows["fused: " + key]["speedup_over_torch"] = round(rows["torch: " + key]["us_median"] /
                                                            rows["fused: " + key]["us_median"], 2)
    report = {
        "shape": {"batch": N, "height": H, "width": W, "classes": nc, "ignore_index": ignore},
        "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
        "iters": args.iters, "torch_iters": args.torch_iters, "rounds": args.rounds,
        "labels_in_prediction": int(pred.unique().numel()), "labels_in_target": int(target.unique().numel()),
        "prediction_agrees_with_target": round(float((pred == target).float().mean()), 4),
        "variants": rows,
        "both_routes_give_the_same_counters": equal,
    }
    if args.resources:
        with open(args.resources) as f:
            report["kernel_resources"] = json.load(f)
    write_report(report, args.out)


if __name__ == "__main__":
    main()
