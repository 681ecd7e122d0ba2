"""Open-set kernels on MI355X (mdil_ss_amd.openset) at the evaluation shape: 6 x 256 x 512 x 16
features, 20 and 27 classes.

    python tools/bench_openset.py [--batch 6 --height 512 --width 1024 --classes 20 27 --iters 20] [--out FILE]

``openset_head`` with all four histograms + label + one code map, and ``openset_apply`` on the stored
maps, against two routes on the same device in the same process: (a) the torch route -- stored
logits, ``logsumexp`` / ``softmax`` / entropy, ``key16``, ``bincount`` -- which is asserted to give
the kernel's histograms when it is handed the kernel's code maps, and (b) this build's
``pseudo_head``, the nearest existing kernel (label + 16-bit confidence + a 32 x 256 histogram in
LDS).  Three inputs load the global histogram differently: the network's features (a trained-looking
spread), all-zero features (every pixel in ONE code per kind: the contention worst case for the
merged atomics) and wide noise (few lanes of a wave share a code: the merge finds nothing).  Timed
with device events around ``--iters`` back-to-back calls after a warm-up of every variant; the
variants alternate over ``--rounds`` rounds and report median, min and max.  No GPU: it fails, it does
not fall back."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


from tools._bench_common import peak_bytes, spread, timed, write_report  # noqa: E402


def torch_scores(feat, w, b):
    """Stored logits -> the four scores, float32 [4,N,2H,2W], and the label."""
    from mdil_ss_amd import ops
    logits = ops.OutFn.apply(feat, w, b).permute(0, 3, 1, 2)
    m, label = logits.max(1)
    lse = torch.logsumexp(logits, 1)
    p = torch.softmax(logits, 1)
    ent = -(p * torch.where(p > 0, p.log(), torch.zeros_like(p))).sum(1)
    return torch.stack([1.0 - p.max(1)[0], -m, -lse, ent]), label.to(torch.uint8)


def torch_hist(codes):
    """int64 codes [4,...] -> [4][65536] by bincount."""
    return torch.stack([torch.bincount(c.reshape(-1), minlength=65536) for c in codes])


def torch_route(feat, w, b):
    from mdil_ss_amd import openset as O
    scores, label = torch_scores(feat, w, b)
    return torch_hist(O.key16(scores)), label


def one_width(nc, args, dev):
    from mdil_ss_amd import openset as O
    from mdil_ss_amd import pseudo as P
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    N, H, W = args.batch, args.height, args.width
    torch.manual_seed(0)
    model = Net([nc], 1, 0).to(dev).eval()
    images = torch.rand(N, 3, H, W, device=dev)
    with torch.no_grad():
        feat = model.features(images, 0).contiguous()
        w, b = (t.detach().contiguous() for t in model.head_params(0))
    feats = {"network features": feat, "all-zero features": torch.zeros_like(feat),
             "wide noise": (torch.randn_like(feat) * 8.0).contiguous()}
    hist = torch.zeros(4, 2, 65536, dtype=torch.int64, device=dev)
    nonf = torch.zeros(1, dtype=torch.int64, device=dev)
    phist = torch.zeros(nc, 256, dtype=torch.int64, device=dev)

    # the kernel's histograms are the bincounts of its own code maps, by torch ops on the same device
    occupied, busiest, score_gap = {}, {}, {}
    for name, x in feats.items():
        hist.zero_()
        O.openset_head(x, w, b, hist=hist, nonfinite=nonf, want_label=False)
        codes = torch.stack([O.code_values(O.openset_head(x, w, b, map_kind=k, want_label=False)[1]) for k in range(4)])
        assert torch.equal(hist[:, 0], torch_hist(codes)) and int(hist[:, 1].sum()) == 0, name
        assert int(nonf.item()) == 0
        occupied[name] = [int((hist[k, 0] > 0).sum()) for k in range(4)]
        busiest[name] = [round(float(hist[k, 0].max()) / float(hist[k, 0].sum()), 4) for k in range(4)]
        # how often the float32 torch evaluation of the formulas lands in another bin than the kernel
        score_gap[name] = [round(float((O.key16(torch_scores(x, w, b)[0][k]) != codes[k]).float().mean()), 5)
                           for k in range(4)]
    label, code = O.openset_head(feat, w, b, map_kind="energy")
    thr = int(O.code_values(code).reshape(-1)[::97].median().item())
    cdf = O.cdf_lut(torch.bincount(O.code_values(code).reshape(-1), minlength=65536).cpu()).to(dev)
    counters = O.new_apply_counters(nc, dev)
    some = {k: counters[k] for k in ("seen", "rejected", "bad_labels")}

    def head(x, **kw):
        return lambda: O.openset_head(x, w, b, map_kind="energy", hist=hist, nonfinite=nonf, **kw)

    variants = {f"openset_head, {name}: label + code + 4 hists": head(x) for name, x in feats.items()}
    variants.update({
        "openset_head, network features: label + code, no hist":
            lambda: O.openset_head(feat, w, b, map_kind="energy"),
        "openset_head, network features: one hist (energy) only":
            lambda: O.openset_head(feat, w, b, kinds=["energy"], hist=hist, want_label=False),
        "openset_head, all-zero features: one hist (energy) only":
            lambda: O.openset_head(feats["all-zero features"], w, b, kinds=["energy"], hist=hist, want_label=False),
        "openset_apply: out + score + seen + rejected": lambda: O.openset_apply(label, code, nc, thr, None, 255, cdf,
                                                                                counters=some),
        "pseudo_head, network features: label + qconf + hist": lambda: P.pseudo_head(feat, w, b, phist, nonf),
        "torch route, network features: logits, logsumexp, softmax, entropy, key16, bincount":
            lambda: torch_route(feat, w, b),
    })
    iters = {k: (3 if k.startswith("torch") else args.iters) for k in variants}
    samples = {k: [] for k in variants}
    with torch.no_grad():
        for k, fn in variants.items():
            timed(fn, 2)
        for _ in range(args.rounds):
            for k, fn in variants.items():
                samples[k].append(timed(fn, iters[k]))
        fused_peak = peak_bytes(head(feat))
        torch_peak = peak_bytes(lambda: torch_route(feat, w, b))
    med = {k: statistics.median(v) for k, v in samples.items()}
    base = med["openset_head, network features: label + code + 4 hists"]
    npix = N * H * W
    return {
        "us_per_call": {k: spread(v, 2, "") for k, v in samples.items()},
        "all_zero_over_network_features": round(med["openset_head, all-zero features: label + code + 4 hists"] / base, 3),
        "wide_noise_over_network_features": round(med["openset_head, wide noise: label + code + 4 hists"] / base, 3),
        "openset_head_over_pseudo_head": round(base / med["pseudo_head, network features: label + qconf + hist"], 3),
        "torch_route_over_openset_head": round(
            med["torch route, network features: logits, logsumexp, softmax, entropy, key16, bincount"] / base, 3),
        "histograms_equal_torch_bincount_of_the_code_maps": True,
        "bins_occupied_per_kind": occupied,
        "share_of_pixels_in_the_busiest_bin_per_kind": busiest,
        "share_of_pixels_where_float32_torch_scores_fall_in_another_bin": score_gap,
        "peak_memory_bytes": {"openset_head (label, code)": fused_peak, "torch route": torch_peak},
        "algorithmic_bytes": {"features read": npix // 4 * 64, "label + code written": npix * 3,
                              "apply reads + writes": npix * 5,
                              "torch route: logits written, then read back": [npix * ((nc + 3) // 4 * 4) * 4] * 2},
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
        raise SystemExit("bench_openset needs an MI355X")
    import mdil_ss_amd  # noqa: F401
    dev = torch.device("cuda", 0)
    report = {"shape": {"batch": args.batch, "height": args.height, "width": args.width},
              "device": torch.cuda.get_device_name(0), "what": "a randomly initialised network; timings only",
              "classes": {str(nc): one_width(nc, args, dev) for nc in args.classes}}
    write_report(report, args.out)


if __name__ == "__main__":
    main()
