"""Superpixel acquisition kernels on MI355X (mdil_ss_amd.superpixel) at the evaluation shape: images of
6 x 3 x 512 x 1024, steps 8, 16 and 32 at compactness 10 and 10 iterations, 20 and 27 classes.

    python tools/bench_spx.py [--batch 6 --height 512 --width 1024 --classes 20 27 --steps 8 16 32 --iterations 10 --iters 10] [--out FILE]

``spx_slic`` on procedural images, on a constant image and on noise; ``spx_table`` and ``spx_apply`` (every output,
one-click answers) on the maps of ``acquire_head`` of a randomly initialised network and the ids of the procedural
images at the middle step.  Against, in the same run on the same card: ``acquire_head`` with label and q map, which
writes what the table reads, and the torch-op route: per iteration nine gathered-centre distances in int64
([N, H, W, 5] temporaries each), ``minimum`` over D << 24 | k, then one ``index_add_`` of the six sums; and
``index_add_`` per field for the table.  The torch route follows the header's rule in integers, so whether it gives
identical ids is reported, with its peak memory.  Timed with device events around ``--iters`` back-to-back calls after
a warm-up of every variant; the variants alternate over ``--rounds`` rounds and report median, min and max.  No GPU:
it fails, it does not fall back."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


from tools._bench_common import HBM_PEAK, peak_bytes, spread, timed, write_report  # noqa: E402


def torch_slic(images, S, m, T):
    """include/mdil_spx.h's rule by torch ops on the device -> (id int64 [N,H,W], centres, sums)."""
    N, _, H, W = images.shape
    dev = images.device
    v = torch.where(torch.isnan(images), torch.zeros_like(images), images).clamp(0.0, 1.0)
    codes = torch.floor((v.double() * 255.0 + 0.5).float()).long()        # one rounding to fp32: the header's fmaf
    Gy, Gx = -(-H // S), -(-W // S)
    K = Gy * Gx
    ys = torch.clamp(torch.arange(Gy, device=dev) * S + S // 2, max=H - 1)
    xs = torch.clamp(torch.arange(Gx, device=dev) * S + S // 2, max=W - 1)
    yy, xx = ys[:, None].expand(Gy, Gx).reshape(-1), xs[None].expand(Gy, Gx).reshape(-1)
    centres = 16 * torch.cat([torch.stack([yy, xx], 1)[None].expand(N, -1, -1), codes[:, :, yy, xx].permute(0, 2, 1)], 2)
    py, px = torch.arange(H, device=dev), torch.arange(W, device=dev)
    y16, x16 = (16 * py)[None, :, None], (16 * px)[None, None, :]
    hy, hx = (py // S)[:, None].expand(H, W), (px // S)[None].expand(H, W)
    base = (torch.arange(N, device=dev) * K)[:, None, None]
    vals = torch.stack([torch.ones(N, H, W, dtype=torch.int64, device=dev), py[None, :, None].expand(N, H, W),
                        px[None, None, :].expand(N, H, W), codes[:, 0], codes[:, 1], codes[:, 2]], -1).reshape(-1, 6)

    def assign():
        best = torch.full((N, H, W), 1 << 62, dtype=torch.int64, device=dev)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                gy, gx = hy + dy, hx + dx
                ok = (gy >= 0) & (gy < Gy) & (gx >= 0) & (gx < Gx)
                k = torch.where(ok, gy * Gx + gx, torch.zeros_like(gy))
                c = centres[:, k.reshape(-1)].reshape(N, H, W, 5)
                dc = (16 * codes[:, 0] - c[..., 2]) ** 2 + (16 * codes[:, 1] - c[..., 3]) ** 2 + (16 * codes[:, 2] - c[..., 4]) ** 2
                D = S * S * dc + m * m * ((y16 - c[..., 0]) ** 2 + (x16 - c[..., 1]) ** 2)
                best = torch.minimum(best, torch.where(ok[None], (D << 24) | k[None], torch.full_like(D, 1 << 62)))
        ids = best & ((1 << 24) - 1)
        sums = torch.zeros(N * K, 6, dtype=torch.int64, device=dev).index_add_(0, (base + ids).reshape(-1), vals)
        return ids, sums.reshape(N, K, 6)

    for _ in range(T):
        _, sums = assign()
        n = sums[..., :1]
        centres = torch.where(n > 0, (16 * sums[..., 1:] + n // 2) // n.clamp(min=1), centres)
    ids, sums = assign()
    return ids, centres, sums


def torch_table(label, q, ids, K, nc):
    """[pixels, sum q, label counts] per superpixel by ``index_add_`` / ``bincount`` (no target)."""
    N = label.shape[0]
    cell = ((torch.arange(N, device=ids.device) * K)[:, None, None] + ids).reshape(-1)
    table = torch.zeros(N * K, 4 + nc, dtype=torch.int64, device=ids.device)
    table[:, 0] = torch.bincount(cell, minlength=N * K)
    table[:, 1].index_add_(0, cell, q.reshape(-1))
    table[:, 4:] = torch.bincount(cell * nc + label.reshape(-1).long(), minlength=N * K * nc).reshape(N * K, nc)
    return table


def images_of(args, dev):
    from mdil_ss_amd.dataset import ProceduralSeg
    N, H, W = args.batch, args.height, args.width
    ds = ProceduralSeg(N, H, W, 20, seed=13, domain=1)
    return {"procedural images": torch.stack([ds[i][0] for i in range(N)]).to(dev).contiguous(),
            "a constant image": torch.full((N, 3, H, W), 0.3, device=dev),
            "noise": torch.rand(N, 3, H, W, device=dev)}


def slic_rows(args, dev, images):
    from mdil_ss_amd import superpixel as P
    m, T = args.compactness, args.iterations
    variants = {}
    for S in args.steps:
        for name, img in images.items():
            variants[f"spx_slic, S {S}, {name}"] = (lambda img=img, S=S: P.spx_slic(img, S, m, T))
        variants[f"torch route slic, S {S}, procedural images"] = (lambda S=S: torch_slic(images["procedural images"], S, m, T))
    samples = {name: [] for name in variants}
    with torch.no_grad():
        for fn in variants.values():
            timed(fn, 1)
        for _ in range(args.rounds):
            for name, fn in variants.items():
                samples[name].append(timed(fn, 1 if name.startswith("torch") else args.iters))
        same, peaks = {}, {}
        for S in args.steps:
            ours, theirs = P.spx_slic(images["procedural images"], S, m, T), torch_slic(images["procedural images"], S, m, T)
            same[str(S)] = all(bool(torch.equal(a.long(), b)) for a, b in zip(ours, theirs))
        S = args.steps[len(args.steps) // 2]
        peaks[f"spx_slic, S {S} (id, centres, sums)"] = peak_bytes(lambda: P.spx_slic(images["procedural images"], S, m, T))
        peaks[f"torch route slic, S {S}"] = peak_bytes(lambda: torch_slic(images["procedural images"], S, m, T))
    med = {name: statistics.median(v) for name, v in samples.items()}
    npix = args.batch * args.height * args.width
    slic_bytes = npix * (12 + 4) + (T + 1) * npix * 4 + npix * 4       # codes pass; a 4-byte read per assign; the ids written
    return {"us_per_call": {name: spread(v, 1, "") for name, v in samples.items()},
            "torch_route_identical_ids_centres_sums": same,
            "torch_route_over_spx_slic": {str(S): round(med[f"torch route slic, S {S}, procedural images"] /
                                                        med[f"spx_slic, S {S}, procedural images"], 2) for S in args.steps},
            "peak_memory_bytes": peaks, "algorithmic_bytes": {"spx_slic": slic_bytes},
            "share_of_hbm_peak": {f"spx_slic, S {S}, procedural images":
                                  round(slic_bytes / (med[f"spx_slic, S {S}, procedural images"] * 1e-6) / HBM_PEAK, 4)
                                  for S in args.steps},
            "what_bounds_the_assign_kernel": "not determined"}, med


def one_width(nc, args, dev, images):
    from mdil_ss_amd import acquire as A
    from mdil_ss_amd import superpixel as P
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    N, H, W = args.batch, args.height, args.width
    npix = N * H * W
    S = args.steps[len(args.steps) // 2]
    torch.manual_seed(0)
    model = Net([nc], 1, 0).to(dev).eval()
    img = images["procedural images"]
    with torch.no_grad():
        feat = model.features(img, 0).contiguous()
        w, b = (t.detach().contiguous() for t in model.head_params(0))
        label, qmap = A.acquire_head(feat, w, b, (2, 2), "entropy", want_label=True, want_qmap=True)
        ids, centres, _ = P.spx_slic(img, S, args.compactness, args.iterations)
    K = centres.shape[1]
    target = torch.randint(0, nc, (N, H, W), device=dev, dtype=torch.uint8)
    scattered = torch.randint(0, K, (N, H, W), device=dev, dtype=torch.int32)
    table, tcount = P.spx_table(label, qmap, ids, K, nc, target, nc - 1)
    answer = P.dominant_answers(tcount, 255)
    selected = (torch.rand(N, K, device=dev) < 0.05).to(torch.uint8) * 255
    counters = P.new_apply_counters(nc, dev)
    q64, ids64 = A.q_values(qmap), ids.long()
    variants = {
        "acquire_head, network features: label + q": lambda: A.acquire_head(feat, w, b, (2, 2), "entropy", want_label=True, want_qmap=True),
        "spx_table, SLIC ids, with target: table + tcount": lambda: P.spx_table(label, qmap, ids, K, nc, target, nc - 1, table, tcount),
        "spx_table, SLIC ids, no target": lambda: P.spx_table(label, qmap, ids, K, nc, table=table),
        "spx_table, scattered ids, no target": lambda: P.spx_table(label, qmap, scattered, K, nc, table=table),
        "torch route table, SLIC ids, no target": lambda: torch_table(label, q64, ids64, K, nc),
        "spx_apply: out + mask + counters, one-click answers": lambda: P.spx_apply(ids, selected, nc, answer, target, None, None, label,
                                                                                  nc - 1, 255, counters, want_mask=True),
    }
    samples = {name: [] for name in variants}
    with torch.no_grad():
        for fn in variants.values():
            timed(fn, 1)
        for _ in range(args.rounds):
            for name, fn in variants.items():
                samples[name].append(timed(fn, 2 if name.startswith("torch") else args.iters))
        peaks = {"spx_table (nothing allocated)": peak_bytes(lambda: P.spx_table(label, qmap, ids, K, nc, table=table)),
                 "torch route table": peak_bytes(lambda: torch_table(label, q64, ids64, K, nc))}
    med = {name: statistics.median(v) for name, v in samples.items()}
    table_bytes, apply_bytes = npix * (1 + 2 + 4), npix * (4 + 1 + 1 + 1 + 1)
    return {"step": S, "superpixels_per_image": K, "us_per_call": {name: spread(v, 2, "") for name, v in samples.items()},
            "torch_route_over_spx_table": round(med["torch route table, SLIC ids, no target"] / med["spx_table, SLIC ids, no target"], 2),
            "peak_memory_bytes": peaks, "algorithmic_bytes": {"spx_table, no target": table_bytes, "spx_apply": apply_bytes},
            "share_of_hbm_peak": {"spx_table, SLIC ids, no target": round(table_bytes / (med["spx_table, SLIC ids, no target"] * 1e-6) / HBM_PEAK, 4),
                                  "spx_apply": round(apply_bytes / (med["spx_apply: out + mask + counters, one-click answers"] * 1e-6) / HBM_PEAK, 4)}}, med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--classes", type=int, nargs="+", default=[20, 27])
    ap.add_argument("--steps", type=int, nargs="+", default=[8, 16, 32])
    ap.add_argument("--compactness", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spx needs an MI355X")
    import mdil_ss_amd  # noqa: F401
    dev = torch.device("cuda", 0)
    images = images_of(args, dev)
    slic, slic_med = slic_rows(args, dev, images)
    classes, head_us = {}, {}
    for nc in args.classes:
        classes[str(nc)], med = one_width(nc, args, dev, images)
        head_us[str(nc)] = med["acquire_head, network features: label + q"]
    slic["spx_slic_over_acquire_head"] = {f"S {S}, {nc} classes": round(slic_med[f"spx_slic, S {S}, procedural images"] / head_us[nc], 2)
                                          for S in args.steps for nc in head_us}
    report = {"shape": {"batch": args.batch, "height": args.height, "width": args.width, "steps": args.steps,
                        "compactness": args.compactness, "iterations": args.iterations},
              "device": torch.cuda.get_device_name(0), "what": "a randomly initialised network; timings only",
              "slic": slic, "classes": classes}
    write_report(report, args.out)


if __name__ == "__main__":
    main()
