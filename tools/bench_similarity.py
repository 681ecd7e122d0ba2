"""The moments kernel of the similarity add-on (mdil_ss_amd.similarity / libmdil_similarity.so) at
the two sizes a validation batch has -- 6 x 64 x 128 rows of 128 + 128 encoder channels and
6 x 256 x 512 rows of 16 + 16 penultimate channels, 20-class labels -- against the same moments from
torch ops on the same device: subtract the pivot, ``cat`` [onehot | x | y], one fp32 ``Z^T @ Z``, and
``index_add_`` for the class sums.

    python tools/bench_similarity.py [--rounds 7] [--iters 10] [--out FILE]

Per size: the time of one ``MomentMeter.add`` call (device events around ``--iters`` calls after a
warm-up; the variants alternate over ``--rounds`` rounds; median and spread), the input bytes and
the workspace bytes over that time, the flops of the tiles the kernel forms over that time, and the
torch route's time.  The two routes' moments are compared before anything is timed and the tool
fails when they differ by more than the fp32 rounding of the torch route allows.  No GPU: it fails,
it does not fall back."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools._bench_common import HBM_PEAK, spread, timed, write_report  # noqa: E402

SIZES = (("encoder", 6 * 64 * 128, 128), ("penultimate", 6 * 256 * 512, 16))
NC = 20
FP32_MATRIX_PEAK = 157.3e12                                           # flop / s


def features(rows, c, dev, seed):
    """20 Gaussian classes around a common offset, as a network's features of a batch roughly are."""
    g = torch.Generator(device=dev).manual_seed(seed)
    labels = torch.randint(0, NC + 1, (rows,), device=dev, generator=g).to(torch.uint8)   # NC: skipped rows
    centres = torch.randn(NC + 1, c, device=dev, generator=g)
    x = (3.0 + centres[labels.long()] + torch.randn(rows, c, device=dev, generator=g)).contiguous()
    return x, labels


def torch_moments(x, y, labels, px, py):
    """-> (n [NC], sx [NC,cx], sy [NC,cy], G [(cx+cy),(cx+cy)]) with fp32 sums."""
    keep = labels < NC
    z = torch.cat([x - px, y - py], 1) * keep[:, None]
    G = z.t() @ z
    s = torch.zeros(NC + 1, z.shape[1], device=x.device).index_add_(0, labels.long(), z)
    n = torch.bincount(labels.long(), minlength=NC + 1)
    return n[:NC], s[:NC, :x.shape[1]], s[:NC, x.shape[1]:], G


def formed_flops(rows, cx, cy):
    """2 x rows x 256 per 16 x 16 tile the kernel forms ("Similarity")."""
    gh, gx, gy = (NC + 15) // 16, (cx + 15) // 16, (cy + 15) // 16
    tiles = gh * (gx + gy) + gx * (gx + 1) // 2 + gy * (gy + 1) // 2 + gx * gy
    return tiles, 2 * rows * 256 * tiles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="calls per timed sample")
    ap.add_argument("--out", help="also write the JSON report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_similarity needs an MI355X")
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import _similarity_lib
    from mdil_ss_amd.similarity import MomentMeter
    dev = torch.device("cuda", 0)
    torch.backends.cuda.matmul.allow_tf32 = False
    report = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters, "classes": NC,
              "sizes": {}}
    with torch.no_grad():
        for name, rows, c in SIZES:
            x, labels = features(rows, c, dev, rows + c)
            y = (x + 0.3 * torch.randn(rows, c, device=dev, generator=torch.Generator(device=dev).manual_seed(5))).contiguous()
            px, py = x[:1024].mean(0), y[:1024].mean(0)
            meter = MomentMeter(c, c, NC, dev, pivot_x=px, pivot_y=py)
            meter.add(x, y, labels)
            m = meter.moments()
            n, sx, sy, G = (t.double().cpu().numpy() for t in torch_moments(x, y, labels, px, py))
            # the torch route sums `rows` fp32 terms in an order of its own: rows * 2^-24 of the entry's scale
            differ = max(float(abs(m["gxx"] - G[:c, :c]).max() / abs(G[:c, :c]).max()),
                         float(abs(m["gyy"] - G[c:, c:]).max() / abs(G[c:, c:]).max()),
                         float(abs(m["gxy"] - G[:c, c:]).max() / abs(G[:c, c:]).max()),
                         float(abs(m["sx"] - sx).max() / abs(sx).max()), float(abs(m["sy"] - sy).max() / abs(sy).max()))
            if not (m["n"] == n).all() or not differ <= rows * 2.0 ** -24:
                raise SystemExit(f"bench_similarity: {name}: the two routes differ by {differ:.3e} of the largest "
                                 f"entry (bound {rows * 2.0 ** -24:.3e})")
            variants = {"accumulate": lambda: meter.add(x, y, labels),
                        "torch": lambda: torch_moments(x, y, labels, px, py)}
            samples = {k: [] for k in variants}
            for fn in variants.values():
                timed(fn, 2)
            for _ in range(args.rounds):
                for k, fn in variants.items():
                    samples[k].append(timed(fn, args.iters))
            med = statistics.median(samples["accumulate"]) * 1e-6
            in_bytes = rows * (2 * c * 4 + 1)
            ws_bytes = _similarity_lib.load().mdil_sim_workspace_bytes(rows, c, c, NC)
            tiles, flops = formed_flops(rows, c, c)
            rows_out = {k: spread(v) for k, v in samples.items()}
            rows_out["accumulate"].update(
                input_bytes=in_bytes, workspace_bytes_written_and_read=ws_bytes,
                input_bytes_per_s=round(in_bytes / med, -9), share_of_hbm_peak=round(in_bytes / med / HBM_PEAK, 4),
                all_bytes_per_s=round((in_bytes + 2 * ws_bytes) / med, -9), tiles=tiles, formed_flops=flops,
                flops_per_s=round(flops / med, -9), share_of_fp32_matrix_peak=round(flops / med / FP32_MATRIX_PEAK, 4),
                speedup_over_torch=round(statistics.median(samples["torch"]) * 1e-6 / med, 2))
            report["sizes"][name] = {"rows": rows, "channels": [c, c], "variants_us": rows_out,
                                     "difference_between_routes": differ}
            del x, y, labels, meter
            torch.cuda.empty_cache()
    write_report(report, args.out)


if __name__ == "__main__":
    main()
