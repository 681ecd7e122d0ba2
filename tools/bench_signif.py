"""Bootstrap resampling of the mIoU on MI355X: the two calls of the significance add-on
(mdil_ss_amd.significance: ``image_counts`` on 6 x 1024 x 2048 label maps, ``resample`` at 500
images, 20 classes, two predictors and 10,000 replicates by default) against torch-ops routes on the
same device and in the same process.

    python tools/bench_signif.py [--batch 6 --height 1024 --width 2048 --classes 20 --images 500 --images-l2 600
                                  --replicates 10000 --iters 10 --rounds 5 --torch-chunk 250]
                                  [--out profiles/signif_bench.json]

The torch routes.  Counts: one ``bincount`` of (image, target, prediction) over the batch, its
diagonal and margins per image.  Replicates: the draws from the same hash written in int64 tensor
ops (a logical shift is an arithmetic one and a mask; the multiplications wrap as the kernel's do),
then either ``counts[idx].sum(1)`` in chunks of ``--torch-chunk`` replicates (gather) or the
multiplicity matrix [B,M] -- how often each image was drawn -- times the table as one fp64 GEMM,
which is exact below 2^53 (gemm); the swap by two masked sums.  The bootstrap is timed twice: at
``--images`` rows, where one predictor's slice of the table fits in LDS, and at ``--images-l2`` rows,
where the kernel reads the table from the L2.  Both score with the same fp64
expression.  Every route must give the fused route's integers bit for bit, or the run aborts; the
scores may differ in the order of the mean's adds, and the largest difference is reported.

Inputs of the count: ``ProceduralSeg`` targets with a perturbed copy as the prediction, one label
everywhere (every add of an image on one address) and noise over all classes.  Timed with device
events around ``--iters`` back-to-back calls after a warm-up of every variant; the variants alternate
over the rounds and each reports its median and spread.  Bytes of the count: both maps in once (2 per
pixel).  No GPU: it fails, it does not fall back."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools._bench_common import HBM_PEAK, peak_bytes, spread, timed, write_report  # noqa: E402
from tools.bench_segments import perturbed  # noqa: E402

GOLDEN, MUL1, MUL2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def signed(c):
    return c - (1 << 64) if c >= 1 << 63 else c


def lsr(z, n):
    return (z >> n) & ((1 << (64 - n)) - 1)


def torch_hash(seed, first, B, M, dev):
    """int64 [B,M]: the bits of the kernel's hash of K = (b << 32) + j + 1."""
    b = torch.arange(first, first + B, dtype=torch.int64, device=dev)[:, None]
    j = torch.arange(M, dtype=torch.int64, device=dev)[None, :]
    z = signed(seed) + signed(GOLDEN) * ((b << 32) + j + 1)
    z = z ^ lsr(z, 30)
    z = z * signed(MUL1)
    z = z ^ lsr(z, 27)
    z = z * signed(MUL2)
    return z ^ lsr(z, 31)


def torch_score(sums, k):
    tp, pr, lb = (sums[:, :, p].double() for p in range(3))
    iou = (tp / (tp + (pr - tp) + (lb - tp) + 1e-15))[..., :k]
    return iou.mean(-1), iou


def torch_bootstrap_gather(counts, k, B, seed, chunk):
    M = counts.shape[0]
    out = []
    for s in range(0, B, chunk):
        idx = lsr(lsr(torch_hash(seed, s, min(chunk, B - s), M, counts.device), 32) * M, 32)
        out.append(counts[idx].sum(1))
    sums = torch.cat(out)
    return (sums,) + torch_score(sums, k)


def torch_bootstrap_gemm(counts, k, B, seed):
    M = counts.shape[0]
    idx = lsr(lsr(torch_hash(seed, 0, B, M, counts.device), 32) * M, 32)
    times = torch.zeros(B, M, dtype=torch.float64, device=counts.device)
    times.scatter_add_(1, idx, torch.ones_like(idx, dtype=torch.float64))
    sums = (times @ counts.reshape(M, -1).double()).round().long().reshape(B, *counts.shape[1:])
    return (sums,) + torch_score(sums, k)


def torch_swap_gemm(counts, k, B, seed):
    M = counts.shape[0]
    bit = lsr(torch_hash(seed, 0, B, M, counts.device), 63).double()                # [B,M]
    flat, other = counts.reshape(M, -1).double(), counts.flip(1).reshape(M, -1).double()
    sums = ((1.0 - bit) @ flat + bit @ other).round().long().reshape(B, *counts.shape[1:])
    return (sums,) + torch_score(sums, k)


def torch_jackknife(counts, k):
    sums = counts.sum(0, keepdim=True) - counts
    return (sums,) + torch_score(sums, k)


def torch_counts(pred, target, nc, ignore):
    """int64 [N,3,nc] by one bincount over the batch; predictions outside the classes share a column."""
    N = pred.shape[0]
    t, p = target.reshape(N, -1).long(), pred.reshape(N, -1).long().clamp(max=nc)
    seen = (t != ignore) & (t < nc)
    n = torch.arange(N, device=pred.device)[:, None].expand_as(t)
    cell = ((n * nc + t) * (nc + 1) + p)[seen]
    m = torch.bincount(cell, minlength=N * nc * (nc + 1)).reshape(N, nc, nc + 1)
    return torch.stack([m[:, :, :nc].diagonal(dim1=1, dim2=2), m[:, :, :nc].sum(1), m.sum(2)], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--height", type=int, default=1024, help="the labels' own height")
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--images", type=int, default=500, help="rows of the resampled table")
    ap.add_argument("--images-l2", type=int, default=600, help="rows of a second table, too large for LDS (above 546 "
                                                                "at 20 classes): the bootstrap that reads the L2")
    ap.add_argument("--replicates", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-chunk", type=int, default=250, help="replicates per gather of the torch route")
    ap.add_argument("--out", help="also write the JSON report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_signif needs an MI355X")
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import significance as S
    from mdil_ss_amd.dataset import ProceduralSeg
    dev = torch.device("cuda", 0)
    nc, N, H, W, M, B, seed = args.classes, args.batch, args.height, args.width, args.images, args.replicates, args.seed
    ignore, k = nc - 1, nc - 1
    ds = ProceduralSeg(N, H, W, nc, seed=12, domain=0)
    target = torch.stack([ds[i][1][0] for i in range(N)]).to(torch.uint8)
    flat = torch.full((N, H, W), 3, dtype=torch.uint8)
    noise = torch.randint(0, nc, (N, H, W), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    maps = {"procedural": (perturbed(target, nc, 1), target), "one label": (flat.clone(), flat),
            "noise": (perturbed(noise, nc, 3, share=0.5), noise)}
    maps = {name: tuple(t.to(dev) for t in v) for name, v in maps.items()}
    npx = N * H * W

    # the table to resample: the procedural images' own rows, drawn with replacement up to M rows of two predictors
    rows = torch_counts(*maps["procedural"], nc, ignore)
    pick = torch.randint(0, N, (M, 2), generator=torch.Generator().manual_seed(2))
    scale = torch.randint(1, 4, (M, 2, 1, 1), generator=torch.Generator().manual_seed(3))
    counts = (rows.cpu()[pick] // scale).contiguous().to(dev)                           # [M,2,3,nc], entries < 2^31
    more = torch.randint(0, M, (args.images_l2,), generator=torch.Generator().manual_seed(4))
    counts_l2 = counts[more.to(dev)].contiguous()
    held = S.new_counts(N, 1, nc, dev)                                                  # accumulated into while timing

    variants, facts = {}, {}
    with torch.no_grad():
        for name, (p, t) in maps.items():
            got = S.new_counts(N, 1, nc, dev)
            S.image_counts(p, t, nc, ignore_index=ignore, counts=got, first_image=0)
            if not torch.equal(got[:, 0], torch_counts(p, t, nc, ignore)):
                raise SystemExit(f"bench_signif: the torch route and the fused route count {name!r} differently")
            facts[f"count: {name}"] = {"both_routes_give_the_same_counts": True}
            variants[f"fused count: {name}"] = lambda p=p, t=t: S.image_counts(p, t, nc, ignore_index=ignore,
                                                                              counts=held, first_image=0)
            variants[f"torch count (bincount): {name}"] = lambda p=p, t=t: torch_counts(p, t, nc, ignore)

        def fused(mode, n, table=counts):
            return lambda: S.resample(table, nc, ignore, mode, n, seed, sums=True, check_entries=False)
        routes = {
            "bootstrap": (fused("bootstrap", B), {"torch bootstrap (gather)": lambda: torch_bootstrap_gather(
                counts, k, B, seed, args.torch_chunk), "torch bootstrap (fp64 gemm)": lambda: torch_bootstrap_gemm(
                counts, k, B, seed)}),
            "swap": (fused("swap", B), {"torch swap (fp64 gemm)": lambda: torch_swap_gemm(counts, k, B, seed)}),
            "jackknife": (fused("jackknife", M), {"torch jackknife": lambda: torch_jackknife(counts, k)}),
            f"bootstrap from the L2 ({args.images_l2} images)": (
                fused("bootstrap", B, counts_l2),
                {f"torch bootstrap (fp64 gemm, {args.images_l2} images)": lambda: torch_bootstrap_gemm(counts_l2, k, B,
                                                                                                       seed)}),
        }
        for mode, (fn, others) in routes.items():
            want = fn()
            variants[f"fused {mode}"] = fn
            for name, other in others.items():
                sums, miou, iou = other()
                if not torch.equal(sums, want["sums"]):
                    raise SystemExit(f"bench_signif: {name} and the fused route give different sums")
                facts[name] = {"sums_identical_to_the_fused_route": True,
                               "max_abs_miou_difference": float((miou - want["miou"]).abs().max()),
                               "max_abs_iou_difference": float((iou - want["iou"]).abs().max())}
                variants[name] = other
            del want
        samples, peaks = {name: [] for name in variants}, {}
        for name, fn in variants.items():
            timed(fn, 1)
            peaks[name] = peak_bytes(fn)
        for _ in range(args.rounds):
            for name, fn in variants.items():
                samples[name].append(timed(fn, args.iters))
    rows_out = {name: dict(spread(v), samples=len(v), peak_memory_bytes=peaks[name]) for name, v in samples.items()}
    for name in maps:
        row = rows_out[f"fused count: {name}"]
        row.update(hbm_bytes=2 * npx, share_of_hbm_peak=round(2 * npx / (row["us_median"] * 1e-6) / HBM_PEAK, 4),
                   speedup_over_torch=round(rows_out[f"torch count (bincount): {name}"]["us_median"] / row["us_median"],
                                            2))
    for mode, (_, others) in routes.items():
        row = rows_out[f"fused {mode}"]
        row["speedup_over_torch"] = {name: round(rows_out[name]["us_median"] / row["us_median"], 2) for name in others}
    report = {
        "shape": {"batch": N, "height": H, "width": W, "classes": nc, "images": M, "images_l2": args.images_l2,
                  "groups": 2, "replicates": B, "table_bytes": int(counts.numel() * 8),
                  "torch_chunk": args.torch_chunk},
        "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
        "iters": args.iters, "rounds": args.rounds, "checks": facts, "variants": rows_out,
    }
    write_report(report, args.out)


if __name__ == "__main__":
    main()
