"""Density kernels on MI355X (mdil_ss_amd.density) at the evaluation shape: 6 x 256 x 512 x 16
features at 20 and 27 classes (``density_head``) and 6 x 64 x 128 rows of 128 channels (``density_rows``).

    python tools/bench_density.py [--batch 6 --height 512 --width 1024 --classes 20 27 --iters 20] [--out FILE]

Three inputs load the histogram differently: a randomly initialised network's features (with a model
fitted to them under random labels), all-zero features (every pixel in ONE code per kind: the contention
worst case) and clustered features with 5 % far rows (hundreds of occupied bins: the normal case of a
density score).  Each with and without the histogram, against ``openset_head`` (label + code + its
four histograms) and ``predict_head`` in the same run, and against the torch-op route on the same card
(``(x - p) @ A.T``, ``cdist``, ``min``, ``key16``, ``bincount``), which is asserted to give the kernel's
histograms when it is handed the kernel's code maps.  Timed with device events around ``--iters``
back-to-back calls after a warm-up of every variant; the variants alternate over ``--rounds`` rounds and
report median, min and max.  No GPU: it fails, it does not fall back."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


from tools._bench_common import HBM_PEAK, peak_bytes, spread, timed, write_report  # noqa: E402


def fit_to(rows, labels, classes):
    """A model fitted to device rows [n, C] through the moments kernel, as ``--fit`` does."""
    from mdil_ss_amd import density as D
    from mdil_ss_amd import similarity as S
    meter = S.MomentMeter(rows.shape[1], 0, classes, rows.device)
    meter.add(rows, None, labels)
    return D.fit_model(meter.moments(), min_rows=2)


def clustered(C, classes, rows, seed, dev):
    """Class means 2 N(0, I), one SPD covariance 0.25 (B B^T / C + 0.1 I), 5 % of the rows uniform in +-6."""
    g = torch.Generator().manual_seed(seed)
    means = 2.0 * torch.randn(classes, C, generator=g)
    B = torch.randn(C, C, generator=g)
    L = torch.linalg.cholesky(0.25 * (B @ B.T / C + 0.1 * torch.eye(C)))
    labels = torch.randint(0, classes, (rows,), generator=g)
    x = means[labels] + torch.randn(rows, C, generator=g) @ L.T
    far = torch.rand(rows, generator=g) < 0.05
    x[far] = torch.rand(int(far.sum()), C, generator=g) * 12.0 - 6.0
    labels[far] = classes
    return x.contiguous().to(dev), labels.to(torch.uint8).to(dev)


def torch_scores(rows, dm):
    """float32 [2, n]: the torch-op route to both scores; it stores the n x K distances."""
    C, K = dm.C, dm.K
    buf = dm.buffer
    p, A, A0 = buf[:C], buf[C:C + C * C].view(C, C), buf[C + C * C:C + 2 * C * C].view(C, C)
    m0, m = buf[C + 2 * C * C:2 * C + 2 * C * C], buf[2 * C + 2 * C * C:].view(K, C)
    w = rows - p
    z = w @ A.T
    # in chunks of at most 2^24 distances: past that, torch.cdist gave wrong distances here (seen at 786,432 rows x 26
    # means, where the share of rows in another bin than the kernel's jumped from 1e-5 to 2^24 / (rows x means))
    step = max(1, (1 << 24) // K)
    dmin = torch.cat([(torch.cdist(z[i:i + step], m, compute_mode="donot_use_mm_for_euclid_dist") ** 2).min(1)[0]
                      for i in range(0, z.shape[0], step)])
    d0 = ((w @ A0.T - m0) ** 2).sum(1)
    return torch.stack([dmin + 0.0, (dmin - d0) + 0.0])


def torch_hist(codes):
    return torch.stack([torch.bincount(c.reshape(-1), minlength=65536) for c in codes])


def torch_route(rows, dm):
    from mdil_ss_amd import openset as O
    return torch_hist(O.key16(torch_scores(rows, dm)))


def measure(variants, args):
    iters = {k: (3 if k.startswith("torch") else args.iters) for k in variants}
    samples = {k: [] for k in variants}
    with torch.no_grad():
        for fn in variants.values():
            timed(fn, 2)
        for _ in range(args.rounds):
            for k, fn in variants.items():
                samples[k].append(timed(fn, iters[k]))
    return samples, {k: statistics.median(v) for k, v in samples.items()}


def head_form(nc, args, dev):
    from mdil_ss_amd import density as D
    from mdil_ss_amd import openset as O
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    from mdil_ss_amd.predict import predict_head
    N, H, W = args.batch, args.height, args.width
    torch.manual_seed(0)
    net = Net([nc], 1, 0).to(dev).eval()
    images = torch.rand(N, 3, H, W, device=dev)
    with torch.no_grad():
        feat = net.features(images, 0).contiguous()
        w, b = (t.detach().contiguous() for t in net.head_params(0))
    rows = feat.view(-1, 16)
    labels = torch.randint(0, nc - 1, (rows.shape[0],), generator=torch.Generator().manual_seed(1)).to(torch.uint8).to(dev)
    cx, cl = clustered(16, nc - 1, rows.shape[0], 2, dev)
    net_model, cl_model = D.DeviceModel(fit_to(rows, labels, nc - 1), dev), D.DeviceModel(fit_to(cx, cl, nc - 1), dev)
    inputs = {"network features": (feat, net_model), "all-zero features": (torch.zeros_like(feat), net_model),
              "clustered features, 5 % far rows": (cx.view(feat.shape), cl_model)}
    hist = torch.zeros(2, 2, 65536, dtype=torch.int64, device=dev)
    ohist = torch.zeros(4, 2, 65536, dtype=torch.int64, device=dev)
    nonf, agree = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)

    occupied, busiest, score_gap = {}, {}, {}
    for name, (x, dm) in inputs.items():
        hist.zero_()
        D.density_head(x, w, b, dm, hist=hist, nonfinite=nonf, want_label=False)
        codes = torch.stack([O.code_values(D.density_head(x, w, b, dm, map_kind=k, want_label=False)[2]) for k in range(2)])
        assert torch.equal(hist[:, 0], torch_hist(codes)) and int(hist[:, 1].sum()) == 0, name
        assert int(nonf.item()) == 0
        occupied[name] = [int((hist[k, 0] > 0).sum()) for k in range(2)]
        busiest[name] = [round(float(hist[k, 0].max()) / float(hist[k, 0].sum()), 4) for k in range(2)]
        t32 = O.key16(torch_scores(x.view(-1, 16), dm))
        score_gap[name] = [round(float((t32[k] != codes[k, :, ::2, ::2].reshape(-1)).float().mean()), 5) for k in range(2)]

    variants = {}
    for name, (x, dm) in inputs.items():
        variants[f"density_head, {name}: label + code + 2 hists + agree"] = \
            lambda x=x, dm=dm: D.density_head(x, w, b, dm, map_kind="maha", hist=hist, nonfinite=nonf, agree=agree)
        variants[f"density_head, {name}: label + code, no hist"] = \
            lambda x=x, dm=dm: D.density_head(x, w, b, dm, map_kind="maha")
        variants[f"openset_head, {name}: label + code + 4 hists"] = \
            lambda x=x: O.openset_head(x, w, b, map_kind="energy", hist=ohist, nonfinite=nonf)
    variants["predict_head, network features: label"] = lambda: predict_head(feat, w, b, None, False)
    variants["torch route, network features: whiten, cdist, min, key16, bincount"] = lambda: torch_route(rows, net_model)
    samples, med = measure(variants, args)
    with torch.no_grad():
        fused_peak = peak_bytes(lambda: D.density_head(feat, w, b, net_model, map_kind="maha", hist=hist, nonfinite=nonf))
        torch_peak = peak_bytes(lambda: torch_route(rows, net_model))
    key = "density_head, {}: label + code + 2 hists + agree"
    okey = "openset_head, {}: label + code + 4 hists"
    base = med[key.format("network features")]
    npix = N * H * W                                              # output pixels; a quarter as many feature pixels
    moved = npix // 4 * 64 + npix * 3
    return {
        "us_per_call": {k: spread(v, 2, "") for k, v in samples.items()},
        "density_head_over_openset_head_with_histograms": {n: round(med[key.format(n)] / med[okey.format(n)], 3) for n in inputs},
        "density_head_over_openset_head_plus_predict_head": round(
            base / (med[okey.format("network features")] + med["predict_head, network features: label"]), 3),
        "histogram_cost": {n: round(med[key.format(n)] / med[f"density_head, {n}: label + code, no hist"], 3) for n in inputs},
        "all_zero_over_network_features": round(med[key.format("all-zero features")] / base, 3),
        "torch_route_over_density_head": round(
            med["torch route, network features: whiten, cdist, min, key16, bincount"] / base, 3),
        "histograms_equal_torch_bincount_of_the_code_maps": True,
        "bins_occupied_per_kind": occupied,
        "share_of_pixels_in_the_busiest_bin_per_kind": busiest,
        "share_of_pixels_where_float32_torch_scores_fall_in_another_bin": score_gap,
        "peak_memory_bytes": {"density_head (label, code)": fused_peak, "torch route (scores and histograms only)": torch_peak},
        "hbm_bytes_moved": {"features read + label + code written": moved,
                            "share_of_hbm_peak": round(moved / (base * 1e-6) / HBM_PEAK, 4)},
    }


def rows_form(args, dev):
    from mdil_ss_amd import density as D
    from mdil_ss_amd import latent
    from mdil_ss_amd import openset as O
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    N, H, W, C, classes = args.batch, args.height, args.width, 128, 19
    torch.manual_seed(0)
    net = Net([classes + 1], 1, 0).to(dev).eval()
    images = torch.rand(N, 3, H, W, device=dev)
    feat = latent.latents(net, images, 0, "encoder")
    rows = feat.view(-1, C)
    n = rows.shape[0]
    labels = torch.randint(0, classes, (n,), generator=torch.Generator().manual_seed(1)).to(torch.uint8).to(dev)
    cx, cl = clustered(C, classes, n, 3, dev)
    net_model, cl_model = D.DeviceModel(fit_to(rows, labels, classes), dev), D.DeviceModel(fit_to(cx, cl, classes), dev)
    inputs = {"network features": (rows, net_model), "all-zero features": (torch.zeros_like(rows), net_model),
              "clustered features, 5 % far rows": (cx, cl_model)}
    hist = torch.zeros(2, 2, 65536, dtype=torch.int64, device=dev)
    nonf = torch.zeros(1, dtype=torch.int64, device=dev)
    occupied, score_gap = {}, {}
    for name, (x, dm) in inputs.items():
        hist.zero_()
        D.density_rows(x, dm, hist=hist, nonfinite=nonf, want_nearest=False)
        codes = torch.stack([O.code_values(D.density_rows(x, dm, map_kind=k, want_nearest=False)[1]) for k in range(2)])
        assert torch.equal(hist[:, 0], torch_hist(codes)) and int(nonf.item()) == 0, name
        occupied[name] = [int((hist[k, 0] > 0).sum()) for k in range(2)]
        t32 = O.key16(torch_scores(x, dm))
        score_gap[name] = [round(float((t32[k] != codes[k]).float().mean()), 5) for k in range(2)]
    variants = {}
    for name, (x, dm) in inputs.items():
        variants[f"density_rows, {name}: nearest + code + 2 hists"] = \
            lambda x=x, dm=dm: D.density_rows(x, dm, map_kind="maha", hist=hist, nonfinite=nonf)
        variants[f"density_rows, {name}: nearest + code, no hist"] = lambda x=x, dm=dm: D.density_rows(x, dm, map_kind="maha")
    variants["torch route, network features: whiten, cdist, min, key16, bincount"] = lambda: torch_route(rows, net_model)
    samples, med = measure(variants, args)
    with torch.no_grad():
        fused_peak = peak_bytes(lambda: D.density_rows(rows, net_model, map_kind="maha", hist=hist, nonfinite=nonf))
        torch_peak = peak_bytes(lambda: torch_route(rows, net_model))
    key = "density_rows, {}: nearest + code + 2 hists"
    base = med[key.format("network features")]
    moved = n * C * 4 + n * 3
    return {
        "rows": n, "channels": C, "class_means": net_model.K,
        "us_per_call": {k: spread(v, 2, "") for k, v in samples.items()},
        "histogram_cost": {m: round(med[key.format(m)] / med[f"density_rows, {m}: nearest + code, no hist"], 3) for m in inputs},
        "all_zero_over_network_features": round(med[key.format("all-zero features")] / base, 3),
        "torch_route_over_density_rows": round(
            med["torch route, network features: whiten, cdist, min, key16, bincount"] / base, 3),
        "histograms_equal_torch_bincount_of_the_code_maps": True,
        "bins_occupied_per_kind": occupied,
        "share_of_rows_where_float32_torch_scores_fall_in_another_bin": score_gap,
        "peak_memory_bytes": {"density_rows (nearest, code)": fused_peak, "torch route": torch_peak},
        "hbm_bytes_moved": {"rows read + nearest + code written": moved, "model tiles staged in LDS per work-group": 2 * (C // 16) * (C // 16 + 1) // 2 * 1024,
                            "share_of_hbm_peak": round(moved / (base * 1e-6) / HBM_PEAK, 4)},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--classes", type=int, nargs="+", default=[20, 27])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_density needs an MI355X")
    import mdil_ss_amd  # noqa: F401
    dev = torch.device("cuda", 0)
    report = {"shape": {"batch": args.batch, "height": args.height, "width": args.width},
              "device": torch.cuda.get_device_name(0),
              "what": "a randomly initialised network, random labels for its fit, ridge 1e-4 untuned; timings only",
              "head_form": {str(nc): head_form(nc, args, dev) for nc in args.classes},
              "rows_form": rows_form(args, dev)}
    write_report(report, args.out)


if __name__ == "__main__":
    main()
