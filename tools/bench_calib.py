"""Calibration head on MI355X: the fused call (mdil_ss_amd.calibrate) against the dense torch route it
replaces, on the same device and in the same process: stored logits, then per temperature
``log_softmax(l / T)`` -> ``max(1)`` -> NLL, Brier score -> ``bincount`` for the reliability
histogram, at 6 x 256 x 512 x 16 features, 20 and 27 classes, 1 and 16 temperatures, 15 bins.

    python tools/bench_calib.py [--batch 6 --height 256 --width 512 --classes 20 27 --iters 10 --dense-iters 1 --rounds 5]
                                [--out FILE]

Two inputs: the random draw of the tests, and a PEAKED one -- the same draw with (8 w, 8 b) -- that
puts most pixels into the top confidence bin, where lane-wise LDS atomics would serialise.  The two
routes' outputs are compared first, and the tool fails if they disagree (labels at fp32 near-ties
only, pixel counts equal, NLL sums to 1e-5, ECE at T = 1 to 1e-4).

Timed with device events around ``--iters`` back-to-back calls after a warm-up of every variant; the
variants alternate over ``--rounds`` rounds and each reports its median and spread.  Peak memory is
the allocator's high-water mark of one call above what was allocated before it.  The report states
the two conditions of the design: the fused call at 16 temperatures is faster than the torch route
at 16, and the peaked input is not slower than the random one by more than the spread between
rounds.  No GPU: it fails, it does not fall back."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools._bench_common import peak_bytes, timed, variant_rows, write_report  # noqa: E402

MAX_LABELS_DIFFERING = 1e-3
EXP_PEAK = 256 * 4 * 8 * 2.4e9           # v_exp_f32: 64 lanes in 8 cycles per SIMD, 4 SIMDs, 256 CUs, 2.4 GHz
TEMPS16 = [0.25 * 16 ** (i / 15) for i in range(16)]
BINS = 15


def bench(nc, N, H, W, iters, dense_iters, rounds, dev, scale):
    from mdil_ss_amd.calibrate import calib_head, calibration_report, workspace_bytes
    g = torch.Generator(device=dev).manual_seed(nc)
    feat = F.relu(torch.randn(N, H, W, 16, device=dev, generator=g))
    w = torch.randn(16, nc, 2, 2, device=dev, generator=g) * 0.3 * scale
    b = torch.randn(nc, device=dev, generator=g) * 0.2 * scale
    ign = nc - 1

    def counters(K, classes=False):
        z = lambda *s: torch.zeros(s, dtype=torch.int64, device=dev)  # noqa: E731
        c = {"hist": z(K, BINS, 3), "nonfinite": z(K), "bad_targets": z(1),
             "sums": torch.zeros(K, 3, dtype=torch.float64, device=dev),
             "workspace": torch.empty(workspace_bytes(N, H, W, nc, K) // 8, dtype=torch.float64, device=dev)}
        if classes:
            c["class_hist"] = z(nc, BINS, 3)
        return c

    def dense(logits, temps, histogram=True):
        """-> per temperature (hist [bins,3] with float confidence sums, nll sum, brier sum, labels)."""
        out = []
        y = target.long().unsqueeze(1)
        for T in temps:
            z = F.log_softmax(logits / T, 1)
            p = z.exp()
            conf, label = p.max(1)
            nll = -z.gather(1, y)[:, 0]
            brier = (p * p).sum(1) - 2 * p.gather(1, y)[:, 0] + 1
            if not histogram:
                out.append((None, nll[counted].double().sum(), brier[counted].double().sum(), label))
                continue
            k = counted.view(-1)
            bins = (conf * BINS).long().clamp_(max=BINS - 1).view(-1)[k]
            correct = (label == target).view(-1)[k]
            hist = torch.stack([torch.bincount(bins, minlength=BINS).double(),
                                torch.bincount(bins, weights=correct.double(), minlength=BINS),
                                torch.bincount(bins, weights=conf.view(-1)[k].double(), minlength=BINS)], 1)
            out.append((hist, nll[counted].double().sum(), brier[counted].double().sum(), label))
        return out

    with torch.no_grad():
        stored = F.conv_transpose2d(feat.permute(0, 3, 1, 2), w, b, stride=2)
        p = F.softmax(stored / 1.7 / scale, 1).permute(0, 2, 3, 1).reshape(-1, nc)
        target = torch.multinomial(p, 1, generator=g).reshape(N, 2 * H, 2 * W).to(torch.uint8)
        del p
        counted = target != ign
        # ---- the two routes agree (at T = 1 and 2)
        c2 = counters(2)
        fused = calib_head(feat, w, b, target, [1.0, 2.0], ignore_index=ign, label=True, counters=c2)
        ref = dense(stored, [1.0, 2.0])
        share = (fused["label"].long() != ref[0][3]).float().mean().item()
        rep = calibration_report(c2["hist"].cpu(), c2["sums"].cpu(), [1.0, 2.0])["temperatures"]
        top_bin = rep[0]["reliability"][-1]["pixels"] / rep[0]["pixels"]
        apart = {}
        for k in range(2):
            hist, nll, brier, _ = ref[k]
            n = hist[:, 0].sum().item()
            ece = ((hist[:, 1] - hist[:, 2]).abs().sum() / n).item()
            apart[k] = (abs(rep[k]["ece"] - ece), abs(c2["sums"][k, 0].item() - nll.item()) / abs(nll.item()),
                        rep[k]["pixels"] == int(n))
        if share > MAX_LABELS_DIFFERING or any(a[0] > 1e-4 or a[1] > 1e-5 or not a[2] for a in apart.values()) or \
                int(c2["nonfinite"].sum()) or int(c2["bad_targets"]):
            raise SystemExit(f"bench_calib: the routes disagree at {nc} classes, scale {scale}: labels differ at "
                             f"{share:.2e} of the pixels; (ECE apart, NLL sum apart, counts equal) per temperature {apart}")
        del fused, ref
        # ---- time
        c1, c16, c16c = counters(1), counters(16), counters(16, True)
        variants = {
            "fused: 1 temperature": lambda: calib_head(feat, w, b, target, [1.0], ignore_index=ign, counters=c1),
            "fused: 16 temperatures": lambda: calib_head(feat, w, b, target, TEMPS16, ignore_index=ign, counters=c16),
            "fused: 16 temperatures + class histogram": lambda: calib_head(
                feat, w, b, target, TEMPS16, ignore_index=ign, class_temp=7, counters=c16c),
            "fused: 16 temperatures, histogram only": lambda: calib_head(
                feat, w, b, target, TEMPS16, ignore_index=ign, counters={"hist": c16["hist"]}),
            "fused: 16 temperatures, sums only": lambda: calib_head(
                feat, w, b, target, TEMPS16, ignore_index=ign, counters={"sums": c16["sums"], "workspace": c16["workspace"]}),
            "dense from stored logits: 1 temperature": lambda: dense(stored, [1.0]),
            "dense from stored logits: 16 temperatures": lambda: dense(stored, TEMPS16),
            "dense from stored logits: 16 temperatures, no histogram": lambda: dense(stored, TEMPS16, False),
        }
        samples = {k: [] for k in variants}
        for k, fn in variants.items():
            timed(fn, 1 if k.startswith("dense") else 2)
        peaks = {k: peak_bytes(fn) for k, fn in variants.items()}
        for _ in range(rounds):
            for k, fn in variants.items():
                samples[k].append(timed(fn, dense_iters if k.startswith("dense") else iters))
    npf, npl = N * H * W, N * 4 * H * W
    lg = npl * nc * 4                                     # the stored logit tensor
    # dense, per temperature: the division and log_softmax read and write the tensor (4 lg), exp and
    # the square read and write it (4 lg), max and the two sums read it (3 lg), the gathers and
    # bincounts move per-pixel maps
    per_t = 11 * lg + npl * 60
    bytes_moved = {"fused: 1 temperature": npf * 64 + npl, "fused: 16 temperatures": npf * 64 + npl,
                   "fused: 16 temperatures + class histogram": npf * 64 + npl,
                   "fused: 16 temperatures, histogram only": npf * 64 + npl,
                   "fused: 16 temperatures, sums only": npf * 64 + npl,
                   "dense from stored logits: 1 temperature": per_t, "dense from stored logits: 16 temperatures": 16 * per_t,
                   "dense from stored logits: 16 temperatures, no histogram": 16 * (11 * lg + npl * 12)}
    rows = variant_rows(samples, bytes_moved, peaks)
    med = {k: statistics.median(v) for k, v in samples.items()}
    exps = npl * 16 * (nc + 1)
    return {"variants": rows, "stored_logits_bytes": lg, "share_of_pixels_in_the_top_bin_at_T1": round(top_bin, 4),
            "labels_differing_between_routes": share,
            "fused_16_exp_per_second": round(exps / (med["fused: 16 temperatures"] * 1e-6), 0),
            "fused_16_share_of_exp_peak": round(exps / (med["fused: 16 temperatures"] * 1e-6) / EXP_PEAK, 4),
            "fused_16_over_dense_16": round(med["fused: 16 temperatures"] / med["dense from stored logits: 16 temperatures"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--height", type=int, default=256, help="feature height (half the network's)")
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--classes", type=int, nargs="+", default=[20, 27])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--dense-iters", type=int, default=1, help="calls per sample of the dense route (seconds each)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_calib needs an MI355X")
    import mdil_ss_amd  # noqa: F401
    dev = torch.device("cuda", 0)
    classes, conditions = {}, {}
    for nc in args.classes:
        r = bench(nc, args.batch, args.height, args.width, args.iters, args.dense_iters, args.rounds, dev, 1.0)
        p = bench(nc, args.batch, args.height, args.width, args.iters, args.dense_iters, args.rounds, dev, 8.0)
        classes[str(nc)] = {"random": r, "peaked": p}
        fr, fp = r["variants"]["fused: 16 temperatures"], p["variants"]["fused: 16 temperatures"]
        noise = max(fr["us_max"] - fr["us_min"], fp["us_max"] - fp["us_min"])
        conditions[str(nc)] = {
            "fused_16_faster_than_dense_16": r["fused_16_over_dense_16"] < 1 and p["fused_16_over_dense_16"] < 1,
            "peaked_minus_random_us": round(fp["us_median"] - fr["us_median"], 1), "spread_between_rounds_us": round(noise, 1),
            "peaked_not_slower_than_random_beyond_the_spread": fp["us_median"] - fr["us_median"] <= noise}
    report = {
        "shape": {"batch": args.batch, "feature_height": args.height, "feature_width": args.width},
        "device": torch.cuda.get_device_name(0), "iters": args.iters, "dense_iters": args.dense_iters,
        "rounds": args.rounds, "bins": BINS,
        "temperatures": TEMPS16, "classes": classes, "conditions": conditions,
    }
    write_report(report, args.out)


if __name__ == "__main__":
    main()
