"""Label-audit kernels on MI355X (mdil_ss_amd.audit) at the evaluation shape: 6 x 256 x 512 x 16
features, 20 and 27 classes.

    python tools/bench_audit.py [--batch 6 --height 512 --width 1024 --classes 20 27 --iters 20] [--out FILE]

Sweep 1 of ``audit_head`` (count + qsum), sweep 2 with all outputs (self-q map, suggest map, count,
joint, per-image counts) and ``audit_apply`` on the stored maps, against two routes on the same device
in the same process: (a) the torch route -- stored logits, ``softmax``, the 16-bit q, ``gather``,
``index_add_`` / ``bincount`` -- which is asserted to give the kernel's counters when it is handed the
kernel's q maps and suggestions, and (b) this build's ``pseudo_head``, the nearest shipped kernel (label
+ 16-bit confidence + a 32 x 256 histogram in LDS).  Three targets load the in-wave merge differently:
block-wise labels (coherent, as real annotation is), every target one class (every lane adds to one
cell) and per-pixel random targets (the merge finds nothing to merge).  Timed with device events around
``--iters`` back-to-back calls after a warm-up of every variant; the variants alternate over
``--rounds`` rounds and report median, min and max.  No GPU: it fails, it does not fall back."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


from tools._bench_common import peak_bytes, spread, timed, write_report  # noqa: E402


def block_target(N, H, W, nc, ignore, dev, block=32):
    """Labels constant over ``block`` x ``block`` pixels, a tenth of the blocks ignored."""
    g = torch.Generator().manual_seed(nc)
    coarse = torch.randint(0, nc - 1, (N, H // block, W // block), generator=g)
    coarse[torch.rand(coarse.shape, generator=g) < 0.1] = ignore
    return coarse.repeat_interleave(block, 1).repeat_interleave(block, 2).to(torch.uint8).to(dev).contiguous()


def torch_logits(feat, w, b):
    from mdil_ss_amd import ops
    return ops.OutFn.apply(feat, w, b).permute(0, 3, 1, 2)


def torch_q(logits):
    return (torch.softmax(logits, 1) * 65536.0).floor().clamp(max=65535.0).long()


def torch_sweep1(q, target, nc, ignore):
    t = target.long()
    valid = (t < nc) & (t != ignore)
    selfq = q.gather(1, t.clamp(max=nc - 1).unsqueeze(1))[:, 0]
    count = torch.bincount(t[valid], minlength=nc)
    qsum = torch.zeros(nc, dtype=torch.int64, device=q.device).index_add_(0, t[valid], selfq[valid])
    return count, qsum


def torch_suggest(q, logits, thr, nc):
    inside = q >= thr.reshape(1, -1, 1, 1)
    best = torch.where(inside, logits, torch.full_like(logits, float("-inf"))).argmax(1)
    return torch.where(inside.any(1), best, torch.full_like(best, nc))


def torch_joint(target, suggest, nc, ignore):
    t = target.long()
    valid = (t < nc) & (t != ignore)
    return torch.bincount(t[valid] * (nc + 1) + suggest[valid], minlength=nc * (nc + 1)).reshape(nc, nc + 1)


def torch_route(feat, w, b, target, thr, nc, ignore):
    """Both sweeps' counters from stored logits."""
    logits = torch_logits(feat, w, b)
    q = torch_q(logits)
    count, qsum = torch_sweep1(q, target, nc, ignore)
    return count, qsum, torch_joint(target, torch_suggest(q, logits, thr, nc), nc, ignore)


def one_width(nc, args, dev):
    from mdil_ss_amd import audit as A
    from mdil_ss_amd import pseudo as P
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    N, H, W = args.batch, args.height, args.width
    ignore = nc - 1
    torch.manual_seed(0)
    model = Net([nc], 1, 0).to(dev).eval()
    images = torch.rand(N, 3, H, W, device=dev)
    with torch.no_grad():
        feat = model.features(images, 0).contiguous()
        w, b = (t.detach().contiguous() for t in model.head_params(0))
    g = torch.Generator().manual_seed(1)
    targets = {"block-wise targets": block_target(N, H, W, nc, ignore, dev),
               "every target one class": torch.full((N, H, W), 3, dtype=torch.uint8, device=dev),
               "per-pixel random targets": torch.randint(0, nc, (N, H, W), generator=g, dtype=torch.uint8).to(dev)}
    phist = torch.zeros(nc, 256, dtype=torch.int64, device=dev)
    pnonf = torch.zeros(1, dtype=torch.int64, device=dev)

    # the kernel's counters are what torch ops count from its own q maps and suggestions, on the same device
    thrs, issue_share, suggest_gap = {}, {}, {}
    with torch.no_grad():
        q_maps = torch.stack([A.q_values(A.audit_head(feat, w, b, q_class=c)[0]) for c in range(nc)], 1)
        logits = torch_logits(feat, w, b)
        q_gap = round(float((torch_q(logits) != q_maps).float().mean()), 6)
        for name, target in targets.items():
            c1 = A.new_head_counters(nc, N, dev, ("count", "qsum", "bad_targets", "nonfinite"))
            A.audit_head(feat, w, b, target, ignore, counters=c1)
            count, qsum = torch_sweep1(q_maps, target, nc, ignore)
            assert torch.equal(c1["count"], count) and torch.equal(c1["qsum"], qsum), name
            thr = A.thresholds(c1["count"].cpu(), c1["qsum"].cpu())
            thrs[name] = torch.tensor(thr, dtype=torch.int32).to(dev)
            c2 = A.new_head_counters(nc, N, dev, ("count", "joint", "per_image", "bad_targets", "nonfinite"))
            selfq, suggest = A.audit_head(feat, w, b, target, ignore, thrs[name], "given", nc, c2, want_suggest=True)
            assert torch.equal(c2["joint"], torch_joint(target, suggest.long(), nc, ignore)), name
            assert torch.equal(c2["per_image"][:, :, 0].sum(0), count) and int(c2["nonfinite"]) == 0, name
            assert torch.equal(c2["per_image"][:, :, 1].sum(0),
                               c2["joint"][:, :nc].sum(1) - c2["joint"][:, :nc].diagonal()), name
            issue_share[name] = round(float(c2["per_image"][:, :, 1].sum()) / max(1.0, float(count.sum())), 4)
            suggest_gap[name] = round(float((torch_suggest(q_maps, logits, thrs[name].long(), nc) !=
                                             suggest.long()).float().mean()), 6)
        del logits, q_maps
    name0 = "block-wise targets"
    target0, thr0 = targets[name0], thrs[name0]
    selfq, suggest = A.audit_head(feat, w, b, target0, ignore, thr0, "given", nc, want_suggest=True)
    max_q = torch.full((nc,), 65535, dtype=torch.int32).to(dev)
    acted = A.new_apply_counters(nc, dev)
    c1 = A.new_head_counters(nc, N, dev, ("count", "qsum"))
    c2 = A.new_head_counters(nc, N, dev, ("count", "joint", "per_image", "bad_targets", "nonfinite"))

    def sweep1(target):
        return lambda: A.audit_head(feat, w, b, target, ignore, counters=c1)

    def sweep2(name, **kw):
        return lambda: A.audit_head(feat, w, b, targets[name], ignore, thrs[name], "given", nc, c2, want_suggest=True, **kw)

    variants = {f"audit_head sweep 1, {name}: count + qsum": sweep1(t) for name, t in targets.items()}
    variants.update({f"audit_head sweep 2, {name}: self-q + suggest + count + joint + per_image": sweep2(name)
                     for name in targets})
    variants.update({
        "audit_head, no target: one q map only": lambda: A.audit_head(feat, w, b, q_class=0),
        "audit_head sweep 2, block-wise targets: maps only, no counters":
            lambda: A.audit_head(feat, w, b, target0, ignore, thr0, "given", nc, want_suggest=True),
        "audit_apply: out + mask + seen + acted": lambda: A.audit_apply(target0, suggest, selfq, nc, max_q, "prune", ignore,
                                                                        nc, 255, acted, want_mask=True),
        "pseudo_head, network features: label + qconf + hist": lambda: P.pseudo_head(feat, w, b, phist, pnonf),
        "torch route, block-wise targets: logits, softmax, q, gather, index_add_, argmax, bincount":
            lambda: torch_route(feat, w, b, target0, thr0.long(), nc, ignore),
    })
    iters = {k: (3 if k.startswith("torch") else args.iters) for k in variants}
    samples = {k: [] for k in variants}
    with torch.no_grad():
        for k, fn in variants.items():
            timed(fn, 2)
        for _ in range(args.rounds):
            for k, fn in variants.items():
                samples[k].append(timed(fn, iters[k]))
        fused_peak = peak_bytes(sweep2(name0))
        torch_peak = peak_bytes(lambda: torch_route(feat, w, b, target0, thr0.long(), nc, ignore))
    med = {k: statistics.median(v) for k, v in samples.items()}
    s1 = {name: med[f"audit_head sweep 1, {name}: count + qsum"] for name in targets}
    s2 = {name: med[f"audit_head sweep 2, {name}: self-q + suggest + count + joint + per_image"] for name in targets}
    pseudo = med["pseudo_head, network features: label + qconf + hist"]
    npix = N * H * W
    return {
        "us_per_call": {k: spread(v, 2, "") for k, v in samples.items()},
        "sweep_2_over_pseudo_head": round(s2[name0] / pseudo, 3),
        "sweep_1_over_pseudo_head": round(s1[name0] / pseudo, 3),
        "sweep_2_one_class_over_block_wise": round(s2["every target one class"] / s2[name0], 3),
        "sweep_2_random_over_block_wise": round(s2["per-pixel random targets"] / s2[name0], 3),
        "sweep_2_counters_over_maps_only": round(
            s2[name0] / med["audit_head sweep 2, block-wise targets: maps only, no counters"], 3),
        "torch_route_over_both_sweeps": round(
            med["torch route, block-wise targets: logits, softmax, q, gather, index_add_, argmax, bincount"] /
            (s1[name0] + s2[name0]), 3),
        "counters_equal_torch_ops_on_the_kernels_own_maps": True,
        "issue_share_on_this_random_network": issue_share,
        "share_of_q_where_float32_torch_softmax_gives_another_q": q_gap,
        "share_of_pixels_where_torch_argmax_over_the_same_confident_set_differs": suggest_gap,
        "peak_memory_bytes": {"audit_head sweep 2 (self-q, suggest)": fused_peak, "torch route": torch_peak},
        "algorithmic_bytes": {"features read": npix // 4 * 64, "target read": npix, "self-q + suggest written": npix * 3,
                              "apply reads + writes": npix * 6,
                              "torch route: logits written, then read back": [npix * nc * 4] * 2},
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
        raise SystemExit("bench_audit needs an MI355X")
    import mdil_ss_amd  # noqa: F401
    dev = torch.device("cuda", 0)
    report = {"shape": {"batch": args.batch, "height": args.height, "width": args.width},
              "device": torch.cuda.get_device_name(0), "what": "a randomly initialised network; timings only",
              "classes": {str(nc): one_width(nc, args, dev) for nc in args.classes}}
    write_report(report, args.out)


if __name__ == "__main__":
    main()
