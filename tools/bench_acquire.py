"""Acquisition kernels on MI355X (mdil_ss_amd.acquire) at the evaluation shape: 6 x 256 x 512 x 16
features, 20 and 27 classes, tiles of 32 x 32.

    python tools/bench_acquire.py [--batch 6 --height 512 --width 1024 --classes 20 27 --tile 32 32 --iters 20] [--out FILE]

``acquire_head`` with every output (label, q map, tile table with a target) on the network's features, on
all-zero features (one label and one q: every add of a tile on one address) and on wide noise features (the
merge inside the wave finds nothing), and ``acquire_apply`` on the stored maps, against two routes on the
same device in the same process: (a) this build's ``pseudo_head`` and ``openset_head`` (both unchanged
from the parent commit), the nearest shipped kernels -- ``openset_head`` does strictly more counter work,
four histograms of 65,536 bins -- and (b) the torch route: stored logits, ``softmax``, the score, the
16-bit q and ``index_add_`` per tile and class, which is asserted to give the kernel's table when it is
handed the kernel's own maps.  Timed with device events around ``--iters`` back-to-back calls after a
warm-up of every variant; the variants alternate over ``--rounds`` rounds and report median, min and
max.  No GPU: it fails, it does not fall back."""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


from tools._bench_common import HBM_PEAK, peak_bytes, spread, timed, write_report  # noqa: E402
from tools.bench_audit import block_target, torch_logits  # noqa: E402


def tile_ids(N, Hl, Wl, tile, dev):
    Ty, Tx = -(-Hl // tile[0]), -(-Wl // tile[1])
    ty = torch.arange(Hl, device=dev) // tile[0]
    tx = torch.arange(Wl, device=dev) // tile[1]
    n = torch.arange(N, device=dev)
    return ((n[:, None, None] * Ty + ty[None, :, None]) * Tx + tx[None, None, :]).reshape(-1), N * Ty * Tx


def torch_table(label, q, target, ids, T, nc, ignore):
    """The tile table from stored maps by ``index_add_``: one per field, one for the label counts."""
    lab, qq, t = label.reshape(-1).long(), q.reshape(-1), target.reshape(-1).long()
    ok = (t < nc) & (t != ignore)
    one = torch.ones_like(lab)
    cols = [torch.zeros(T, dtype=torch.int64, device=label.device).index_add_(0, ids, v)
            for v in (one, qq, (ok & (lab != t)).long(), ok.long())]
    hist = torch.zeros(T * nc, dtype=torch.int64, device=label.device).index_add_(0, ids * nc + lab, one)
    return torch.cat([torch.stack(cols, 1), hist.reshape(T, nc)], 1)


def torch_entropy_q(logits, nc):
    logp = torch.log_softmax(logits, 1)
    u = -(logp.exp() * logp).sum(1) * float(1.0 / math.log(nc))
    return (u.clamp(min=0.0) * 65536.0).floor().clamp(max=65535.0).long()


def torch_route(feat, w, b, target, ids, T, nc, ignore):
    """label, q and the table from stored logits."""
    logits = torch_logits(feat, w, b)
    label = logits.argmax(1)
    return torch_table(label, torch_entropy_q(logits, nc), target, ids, T, nc, ignore)


def one_width(nc, args, dev):
    from mdil_ss_amd import acquire as A
    from mdil_ss_amd import openset as O
    from mdil_ss_amd import pseudo as P
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    N, H, W = args.batch, args.height, args.width
    tile, ignore = tuple(args.tile), nc - 1
    torch.manual_seed(0)
    model = Net([nc], 1, 0).to(dev).eval()
    images = torch.rand(N, 3, H, W, device=dev)
    with torch.no_grad():
        feat = model.features(images, 0).contiguous()
        w, b = (t.detach().contiguous() for t in model.head_params(0))
    feats = {"network features": feat, "all-zero features": torch.zeros_like(feat),
             "wide noise": (torch.randn_like(feat) * 8.0).contiguous()}
    target = block_target(N, H, W, nc, ignore, dev)
    ids, T = tile_ids(N, H, W, tile, dev)
    counters = {k: torch.zeros(1, dtype=torch.int64, device=dev) for k in A.HEAD_COUNTERS}
    tiles = A.new_tiles(N, (H, W), tile, nc, dev)
    hist = torch.zeros(4, 2, 65536, dtype=torch.int64, device=dev)
    nonf = torch.zeros(1, dtype=torch.int64, device=dev)
    phist = torch.zeros(nc, 256, dtype=torch.int64, device=dev)

    # the kernel's table is what torch ops count from its own maps, on the same device
    labels_per_tile, q_gap = {}, {}
    with torch.no_grad():
        for name, x in feats.items():
            for kind in A.KINDS:
                t = A.new_tiles(N, (H, W), tile, nc, dev)
                label, qmap = A.acquire_head(x, w, b, tile, kind, target, ignore, t, want_label=True, want_qmap=True)
                want = torch_table(label, A.q_values(qmap), target, ids, T, nc, ignore)
                assert torch.equal(t.reshape(T, -1), want), (name, kind)
                if kind == "entropy":
                    labels_per_tile[name] = round(float((t[..., 4:] > 0).sum(-1).double().mean()), 2)
                    q_gap[name] = round(float((torch_entropy_q(torch_logits(x, w, b), nc) != A.q_values(qmap)).float().mean()), 6)
                    if name == "network features":
                        label0 = label
    sel = (torch.rand(N, *A.tile_grid((H, W), tile), device=dev) < 0.05).to(torch.uint8)
    applied = A.new_apply_counters(nc, dev)

    def head(x, **kw):
        return lambda: A.acquire_head(x, w, b, tile, "entropy", target, ignore, tiles, counters, want_label=True,
                                      want_qmap=True, **kw)

    variants = {f"acquire_head, {name}: label + q + tiles": head(x) for name, x in feats.items()}
    variants.update({
        "acquire_head, network features: label + q, no tiles":
            lambda: A.acquire_head(feat, w, b, tile, "entropy", want_label=True, want_qmap=True),
        "acquire_head, network features: tiles only, msp, no target":
            lambda: A.acquire_head(feat, w, b, tile, "msp", tiles=tiles),
        "acquire_head, network features: label + q + tiles, tiles of 2 x 2":
            lambda: A.acquire_head(feat, w, b, (2, 2), "entropy", target, ignore, tiles2, counters, want_label=True,
                                   want_qmap=True),
        "acquire_apply: out + mask + counters": lambda: A.acquire_apply(sel, (H, W), tile, nc, target, label0, None, ignore,
                                                                        255, applied, want_mask=True),
        "pseudo_head, network features: label + qconf + hist": lambda: P.pseudo_head(feat, w, b, phist, nonf),
        "openset_head, network features: label + code + 4 hists":
            lambda: O.openset_head(feat, w, b, map_kind="energy", hist=hist, nonfinite=nonf),
        "torch route, network features: logits, log_softmax, entropy, q, argmax, index_add_":
            lambda: torch_route(feat, w, b, target, ids, T, nc, ignore),
    })
    tiles2 = A.new_tiles(N, (H, W), (2, 2), nc, dev)
    iters = {k: (3 if k.startswith("torch") else args.iters) for k in variants}
    samples = {k: [] for k in variants}
    with torch.no_grad():
        for k, fn in variants.items():
            timed(fn, 2)
        for _ in range(args.rounds):
            for k, fn in variants.items():
                samples[k].append(timed(fn, iters[k]))
        fused_peak = peak_bytes(head(feat))
        torch_peak = peak_bytes(lambda: torch_route(feat, w, b, target, ids, T, nc, ignore))
    med = {k: statistics.median(v) for k, v in samples.items()}
    mine = {name: med[f"acquire_head, {name}: label + q + tiles"] for name in feats}
    net = mine["network features"]
    npix = N * H * W
    moved = npix // 4 * 64 + npix + npix * 3 + T * (4 + nc) * 8        # features, target, label + q, the table once
    return {
        "us_per_call": {k: spread(v, 2, "") for k, v in samples.items()},
        "acquire_over_pseudo_head": round(net / med["pseudo_head, network features: label + qconf + hist"], 3),
        "acquire_over_openset_head": round(net / med["openset_head, network features: label + code + 4 hists"], 3),
        "tiles_over_maps_only": round(net / med["acquire_head, network features: label + q, no tiles"], 3),
        "all_zero_over_network": round(mine["all-zero features"] / net, 3),
        "wide_noise_over_network": round(mine["wide noise"] / net, 3),
        "torch_route_over_acquire_head": round(
            med["torch route, network features: logits, log_softmax, entropy, q, argmax, index_add_"] / net, 3),
        "tables_equal_torch_ops_on_the_kernels_own_maps": True,
        "mean_labels_per_tile": labels_per_tile,
        "share_of_q_where_float32_torch_entropy_gives_another_q": q_gap,
        "peak_memory_bytes": {"acquire_head (label, q, tiles)": fused_peak, "torch route": torch_peak},
        "algorithmic_bytes": {"acquire_head": moved, "torch route: logits written, then read back": [npix * nc * 4] * 2},
        "share_of_hbm_peak": round(moved / (net * 1e-6) / HBM_PEAK, 4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--classes", type=int, nargs="+", default=[20, 27])
    ap.add_argument("--tile", type=int, nargs=2, default=[32, 32])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_acquire needs an MI355X")
    import mdil_ss_amd  # noqa: F401
    dev = torch.device("cuda", 0)
    report = {"shape": {"batch": args.batch, "height": args.height, "width": args.width, "tile": args.tile},
              "device": torch.cuda.get_device_name(0), "what": "a randomly initialised network; timings only",
              "classes": {str(nc): one_width(nc, args, dev) for nc in args.classes}}
    write_report(report, args.out)


if __name__ == "__main__":
    main()
