"""Connected components on MI355X: the fused calls (mdil_ss_amd.segments: ``label``, ``label`` +
``segment_count`` for both sides as ``SegmentMeter.add`` runs them, ``despeckle``) against a
torch-ops route on the same device and in the same process -- masked min-propagation over the
same-label neighbour pairs with pointer jumping (``r = r.gather(r)``) between sweeps, to a fixed
point -- and against the numpy reference (and scipy, where it is installed) on the host for one
image; at 6 x 1024 x 2048 by default.

    python tools/bench_segments.py [--batch 6 --height 1024 --width 2048 --classes 20 --iters 10 --rounds 5
                                    --torch-iters 1 --torch-rounds 3 --torch-budget 10]
                                    [--out FILE]

Inputs: ``ProceduralSeg`` targets with a perturbed copy as the prediction (``procedural``), one label
everywhere (every add of an image on one address), a full-size spiral (a parent chain as long as the
segment) and two-label noise (millions of segments).  Timed with device events around ``--iters``
back-to-back calls after a warm-up of every variant; the variants alternate over the rounds and each
reports its median and spread.  The torch route needs about as many sweeps as the longest path
inside a segment has pixels, so an input on which one call takes more than ``--torch-budget``
seconds is timed once.  The torch route must give the fused route's roots bit for bit, or
the run aborts.  Bytes of the label call: what its three launches must move through HBM (the map in
twice, parents out and in, the cleared areas and the roots out: 18 bytes per pixel); the atomics and
the parent chains come on top and are served by the L2.  No GPU: it fails, it does not fall back."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools._bench_common import HBM_PEAK, peak_bytes, spread, timed, write_report  # noqa: E402

HALF = {4: ((0, 1), (1, 0)), 8: ((0, 1), (1, 0), (1, 1), (1, -1))}
LABEL_BYTES_PER_PIXEL = 18


def torch_route(m, connectivity):
    """-> (roots i64 [N,H,W], sweeps): min-propagation with pointer jumping, every image on its own."""
    N, H, W = m.shape
    r = torch.arange(H * W, device=m.device).view(1, H, W).repeat(N, 1, 1)
    pairs = []
    for dy, dx in HALF[connectivity]:
        a = (slice(None), slice(0, H - dy), slice(max(0, -dx), W - max(0, dx)))
        b = (slice(None), slice(dy, H), slice(max(0, dx), W + min(0, dx)))
        pairs.append((a, b, m[a] == m[b]))
    sweeps = 0
    while True:
        before = r.clone()
        for a, b, same in pairs:
            low = torch.minimum(r[a], r[b])
            r[a] = torch.where(same, low, r[a])
            r[b] = torch.where(same, torch.minimum(low, r[b]), r[b])
        flat = r.view(N, -1)
        while True:
            nxt = flat.gather(1, flat)
            if torch.equal(nxt, flat):
                break
            flat.copy_(nxt)
        sweeps += 1
        if torch.equal(before, r):
            return r, sweeps


def perturbed(target, n_labels, seed, shift=2, share=0.01):
    g = torch.Generator().manual_seed(seed)
    pred = torch.roll(target, (shift, shift), dims=(-2, -1))
    flip = torch.rand(target.shape, generator=g) < share
    pred[flip] = torch.randint(0, n_labels, (int(flip.sum()),), generator=g, dtype=torch.uint8)
    return pred.contiguous()


def host_routes(image, connectivity):
    """Seconds of the numpy reference (and of scipy, where installed) on one image, and whether they agree."""
    from tests import segments_reference as R
    t0 = time.perf_counter()
    root = R.roots_propagate(image, connectivity)
    out = {"numpy_reference_s": round(time.perf_counter() - t0, 3)}
    try:
        from scipy import ndimage
    except ImportError:
        out["scipy_s"] = None
        return root, out
    t0 = time.perf_counter()
    own = np.arange(image.size).reshape(image.shape)
    want = np.empty(image.shape, dtype=np.int32)
    for c in np.unique(image):
        lab, n = ndimage.label(image == c, structure=np.ones((3, 3)) if connectivity == 8 else None)
        low = ndimage.minimum(own, lab, np.arange(1, n + 1)).astype(np.int32)
        want[lab > 0] = low[lab[lab > 0] - 1]
    out["scipy_s"] = round(time.perf_counter() - t0, 3)
    out["scipy_agrees"] = bool(np.array_equal(root, want))
    return root, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--height", type=int, default=1024, help="the labels' own height")
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--connectivity", type=int, choices=(4, 8), default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-iters", type=int, default=1, help="calls per timed window of the torch route")
    ap.add_argument("--torch-rounds", type=int, default=3)
    ap.add_argument("--torch-budget", type=float, default=10.0, help="an input whose first torch call takes longer "
                                                                      "than this many seconds is timed once")
    ap.add_argument("--out", help="also write the JSON report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_segments needs an MI355X")
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd import segments as S
    from mdil_ss_amd.dataset import ProceduralSeg
    from tests import segments_reference as R
    dev = torch.device("cuda", 0)
    nc, N, H, W, conn = args.classes, args.batch, args.height, args.width, args.connectivity
    ds = ProceduralSeg(N, H, W, nc, seed=12, domain=0)
    target = torch.stack([ds[i][1][0] for i in range(N)]).to(torch.uint8)
    flat = torch.full((N, H, W), 3, dtype=torch.uint8)
    spiral = torch.from_numpy(R.spiral(H, W))[None].repeat(N, 1, 1)
    noise = torch.randint(0, 2, (N, H, W), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    inputs = {"procedural": (target, perturbed(target, nc, 1)), "one label": (flat, flat.clone()),
              "spiral": (spiral, perturbed(spiral, 2, 2, shift=1)), "noise": (noise, perturbed(noise, 2, 3))}
    host_image = target[0].numpy()
    inputs = {k: tuple(t.to(dev) for t in v) for k, v in inputs.items()}
    npx = N * H * W
    ws = torch.empty(S.workspace_bytes(N, H, W), dtype=torch.uint8, device=dev)
    meter = S.SegmentMeter(nc, nc - 1, connectivity=conn)
    held = {s: S.new_counters(nc, meter.nb, dev) for s in ("target", "pred")}       # accumulated into while timing

    def both_sides(t, p):
        for side, a, b, a_ign, b_ign in (("target", t, p, nc - 1, -1), ("pred", p, t, -1, nc - 1)):
            root, area = S.label(a, conn, ws)
            S.segment_count(a, b, root, area, nc, meter.edges, map_ignore=a_ign, other_ignore=b_ign,
                            counters=held[side], workspace=ws)

    variants, facts = {}, {}
    with torch.no_grad():
        for name, (t, p) in inputs.items():
            root, area = S.label(t, conn, ws)
            want, sweeps = torch_route(t, conn)
            if not torch.equal(root.long(), want):
                raise SystemExit(f"bench_segments: the torch route and the fused route disagree on {name!r}")
            facts[name] = {"segments": int((area > 0).sum()), "largest_segment": int(area.max()),
                           "torch_route_sweeps": sweeps, "both_routes_give_the_same_roots": True}
            del want, root, area
            variants[f"fused label: {name}"] = (lambda t=t: S.label(t, conn, ws), args.iters, args.rounds)
            variants[f"fused label + count, both sides: {name}"] = (lambda t=t, p=p: both_sides(t, p), args.iters,
                                                                    args.rounds)
            variants[f"fused despeckle (label + filter): {name}"] = (lambda p=p: S.despeckle(p, 16, connectivity=conn),
                                                                     args.iters, args.rounds)
            variants[f"torch label: {name}"] = (lambda t=t: torch_route(t, conn), args.torch_iters, args.torch_rounds)
        samples, peaks = {k: [] for k in variants}, {}
        for k, (fn, _, _) in variants.items():
            if k.startswith("torch"):                       # its check above was its warm-up
                peaks[k] = peak_bytes(lambda fn=fn, k=k: samples[k].append(timed(fn, 1)))
            else:
                timed(fn, 1)
                peaks[k] = peak_bytes(fn)
        for r in range(max(args.rounds, args.torch_rounds)):
            for k, (fn, iters, rounds) in variants.items():
                slow = k.startswith("torch") and samples[k][0] > args.torch_budget * 1e6
                if len(samples[k]) < rounds and not slow:
                    samples[k].append(timed(fn, iters))
    rows = {}
    for k, v in samples.items():
        rows[k] = dict(spread(v), samples=len(v), peak_memory_bytes=peaks[k])
    for name in inputs:
        row = rows[f"fused label: {name}"]
        med = row["us_median"] * 1e-6
        row.update(hbm_bytes=LABEL_BYTES_PER_PIXEL * npx,
                   share_of_hbm_peak=round(LABEL_BYTES_PER_PIXEL * npx / med / HBM_PEAK, 4),
                   speedup_over_torch=round(rows[f"torch label: {name}"]["us_median"] / row["us_median"], 2))
    host_root, host = host_routes(host_image, conn)
    with torch.no_grad():
        one = S.label(inputs["procedural"][0][:1].contiguous(), conn)[0][0].cpu().numpy()
    host["numpy_reference_agrees_with_the_fused_route"] = bool(np.array_equal(one, host_root))
    host["image"] = f"procedural, 1 x {H} x {W}"
    report = {
        "shape": {"batch": N, "height": H, "width": W, "classes": nc, "connectivity": conn},
        "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
        "iters": args.iters, "rounds": args.rounds, "torch_iters": args.torch_iters, "torch_rounds": args.torch_rounds,
        "workspace_bytes": int(ws.numel()), "inputs": facts, "variants": rows, "host_routes_one_image": host,
    }
    write_report(report, args.out)


if __name__ == "__main__":
    main()
