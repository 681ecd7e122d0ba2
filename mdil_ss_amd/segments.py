"""Label maps as sets of objects, at the DATASET's own size on MI355X: connected components of a
predicted and a ground-truth label map by a lock-free union-find over pixels, segment recall and
precision binned by segment size, missed and hallucinated segments, and a despeckle filter for
pseudo-label maps (include/mdil_segments.h).  Every count is exact.

    python -m mdil_ss_amd.segments --state model_best_....pth.tar --num-classes 20 20 27 --task 0 \
        --dataset cityscapes [--cs-datadir ...] [--edges 64 256 1024] [--coverage 0.5] --score [--json FILE] \
        [--out DIR]
    python -m mdil_ss_amd.segments --pred MAPS --num-classes 20 20 27 --task 0 --dataset cityscapes --score
    python -m mdil_ss_amd.segments --clean MAPS --min-area 16 --out CLEANED [--min-area-class C A ...] \
        [--keep-id 255] [--fill 255] [--json FILE]

The prediction is the full-size label map of ``mdil_ss_amd.fullres`` (``--state``), or the
``<stem>_label.png`` files in train ids that ``predict`` / ``fullres`` / ``ensemble`` wrote
(``--pred DIR``).  A ground-truth segment is *covered* when at least ``--coverage`` of its judged
pixels carry its label in the prediction, and *missed* when none does; a predicted segment is judged
the same way against the ground truth (segment precision, hallucinated segments).  ``--out`` with
``--score`` writes ``<stem>_segments.png``: the ground truth's segments green where covered, amber
where partly hit, red where missed, ignored pixels grey.  ``--clean`` reads every 8-bit
single-channel PNG under MAPS, recursively, replaces the segments smaller than ``--min-area`` pixels
by ``--fill`` (``--keep-id`` is never removed) and writes the map under the same relative path in
CLEANED: a ``pseudo --out-root`` tree cleans to a tree the trainers open unchanged."""
import os
from fractions import Fraction

import numpy as np
import torch

from . import _head_common as hc
from . import _labelsize_common as ls
from . import _report_common as rc
from . import _segments_lib

_PATH = "segments"
HISTS = ("segments", "pixels", "hit_pixels", "covered", "missed", "unjudged")
COUNTERS = HISTS + ("bad_labels",)
DEFAULT_EDGES = (64, 256, 1024, 4096, 16384, 65536)
DEFAULT_COVERAGE = Fraction(1, 2)


def _chk(fn, t, name, dtype=torch.uint8):
    hc.chk(fn, _PATH, t, name, dtype)


def check_edges(edges):
    """-> the area edges as a list of ints: 1 to 8 strictly increasing integers in [1, 2^30]."""
    fn = "segments_count"
    try:
        e = [int(v) for v in edges]
    except (TypeError, ValueError):
        raise RuntimeError(f"mdil {fn}: edges must be integers, got {edges!r}") from None
    if not 1 <= len(e) <= _segments_lib.MAX_EDGES:
        raise RuntimeError(f"mdil {fn}: {len(e)} edges (supported: 1 to {_segments_lib.MAX_EDGES})")
    if any(v < 1 or v > _segments_lib.MAX_EDGE for v in e) or any(b <= a for a, b in zip(e, e[1:])):
        raise RuntimeError(f"mdil {fn}: edges must be strictly increasing within [1, {_segments_lib.MAX_EDGE}], "
                           f"got {e}")
    return e


def check_coverage(coverage):
    """-> (cover_num, cover_den) of a share in (0, 1]: a Fraction as it is, a number or a string
    through ``Fraction(str(v)).limit_denominator(1000)``."""
    try:
        f = coverage if isinstance(coverage, Fraction) else \
            Fraction(str(coverage)).limit_denominator(_segments_lib.MAX_COVER_DEN)
    except (TypeError, ValueError, ZeroDivisionError):
        raise RuntimeError(f"mdil segments_count: coverage must be a share in (0, 1], got {coverage!r}") from None
    if not 0 < f <= 1 or f.denominator > _segments_lib.MAX_COVER_DEN:
        raise RuntimeError(f"mdil segments_count: coverage {f} must be in (0, 1] with a denominator up to "
                           f"{_segments_lib.MAX_COVER_DEN}")
    return f.numerator, f.denominator


def _check_connectivity(fn, connectivity):
    if connectivity not in (4, 8):
        raise RuntimeError(f"mdil {fn}: connectivity must be 4 or 8, got {connectivity!r}")
    return int(connectivity)


def counter_shapes(nc, nb):
    return dict({k: (nc, nb) for k in HISTS}, bad_labels=(1,))


def new_counters(nc, nb, dev):
    """The seven int64 counters of ``segment_count`` for ``nc`` classes and ``nb`` bins, zeroed, on ``dev``."""
    return {k: torch.zeros(s, dtype=torch.int64, device=dev) for k, s in counter_shapes(nc, nb).items()}


def workspace_bytes(N, H, W):
    need = _segments_lib.load().mdil_segments_workspace_bytes(N, H, W)
    if need < 0:
        raise RuntimeError(f"mdil segments: maps [{N},{H},{W}] are outside the supported sizes (H, W up to "
                           f"{_segments_lib.MAX_SIZE}, 2^40 pixels)")
    return need


def _check_map(fn, t, name, like=None, dtype=torch.uint8):
    _chk(fn, t, name, dtype)
    if t.dim() != 3 or t.numel() == 0 or (like is not None and (t.shape != like.shape or t.device != like.device)):
        want = "[N,H,W]" if like is None else f"{list(like.shape)} on {like.device}"
        raise RuntimeError(f"mdil {fn}: {name} must be a {str(dtype)[6:]} map {want} (got {tuple(t.shape)} on "
                           f"{t.device})")


def _workspace(fn, workspace, like):
    need = workspace_bytes(*like.shape)
    if workspace is None:
        return torch.empty(need, dtype=torch.uint8, device=like.device)
    _chk(fn, workspace, "workspace")
    if workspace.device != like.device or workspace.numel() < need:
        raise RuntimeError(f"mdil {fn}: workspace must hold {need} bytes on {like.device} (got "
                           f"{workspace.numel()} on {workspace.device})")
    return workspace


def label(map, connectivity=8, workspace=None):  # noqa: A002  (the header's name)
    """Connected components of ``map`` (u8 [N,H,W] on the device, any byte is a label), every image
    on its own, on the current stream.  -> (root, area), i32 [N,H,W]: the smallest y*W + x of the
    pixel's segment, and the segment's pixel count at that root pixel (0 everywhere else).
    ``workspace``: u8, at least ``workspace_bytes(N, H, W)`` bytes on the device (allocated when None)."""
    fn = "segments_label"
    lib = _segments_lib.load()
    _check_map(fn, map, "map")
    connectivity = _check_connectivity(fn, connectivity)
    N, H, W = map.shape
    with torch.no_grad(), torch.cuda.device(map.device):
        workspace = _workspace(fn, workspace, map)
        root = torch.empty(N, H, W, dtype=torch.int32, device=map.device)
        area = torch.empty(N, H, W, dtype=torch.int32, device=map.device)
        _segments_lib.check(
            lib.mdil_segments_label(map.data_ptr(), N, H, W, connectivity, root.data_ptr(), area.data_ptr(),
                                    workspace.data_ptr(), workspace.numel(),
                                    torch.cuda.current_stream(map.device).cuda_stream),
            "mdil_segments_label")
    return root, area


def segment_count(map, other, root, area, nc, edges=DEFAULT_EDGES, *, map_ignore=-1, other_ignore=-1,  # noqa: A002
                  coverage=DEFAULT_COVERAGE, counters, workspace=None, overlap=False):
    """Counts the segments of ``map`` (``root``, ``area``: those of ``label(map)``) against ``other``
    INTO ``counters`` -- a dict of the seven int64 device tensors of ``new_counters(nc, len(edges) + 1,
    device)``, accumulated into, never cleared -- by class and by the bin of their area
    (include/mdil_segments.h), on the current stream.
    -> (hit, void): i32 [N,H,W] with the segment's sums at its root, or (None, None) without ``overlap``."""
    import ctypes as C
    fn = "segments_count"
    lib = _segments_lib.load()
    _check_map(fn, map, "map")
    _check_map(fn, other, "other", map)
    _check_map(fn, root, "root", map, torch.int32)
    _check_map(fn, area, "area", map, torch.int32)
    nc = int(nc)
    if not _segments_lib.MIN_CLASSES <= nc <= _segments_lib.MAX_CLASSES:
        raise RuntimeError(f"mdil {fn}: {nc} classes (supported: {_segments_lib.MIN_CLASSES} to "
                           f"{_segments_lib.MAX_CLASSES})")
    e = check_edges(edges)
    num, den = check_coverage(coverage)
    hc.check_ignore_index(fn, map_ignore)
    hc.check_ignore_index(fn, other_ignore)
    c = rc.check_counters(fn, counters, COUNTERS)
    missing = [k for k in COUNTERS if c[k] is None]
    if missing:
        raise RuntimeError(f"mdil {fn}: counters {missing} are missing; all of {list(COUNTERS)} are needed (int64, on "
                           "the device; they are accumulated into)")
    shapes = counter_shapes(nc, len(e) + 1)
    hc.check_tables(fn, _PATH, map.device, torch.int64, tuple((c[k], k, shapes[k]) for k in COUNTERS))
    N, H, W = map.shape
    with torch.no_grad(), torch.cuda.device(map.device):
        workspace = _workspace(fn, workspace, map)
        hit = torch.empty_like(root) if overlap else None
        void = torch.empty_like(root) if overlap else None
        _segments_lib.check(
            lib.mdil_segments_count(map.data_ptr(), other.data_ptr(), root.data_ptr(), area.data_ptr(), N, H, W, nc,
                                    int(map_ignore), int(other_ignore), (C.c_int * len(e))(*e), len(e), num, den,
                                    workspace.data_ptr(), workspace.numel(), hc.ptr(hit), hc.ptr(void),
                                    *(c[k].data_ptr() for k in COUNTERS),
                                    torch.cuda.current_stream(map.device).cuda_stream),
            "mdil_segments_count")
    return hit, void


def min_area_table(min_area, per_class=None):
    """-> i32 [256] on the host: ``min_area`` for every label byte (an int, or 256 of them), then
    ``per_class`` {label: area} on top."""
    fn = "segments_filter"
    try:
        if isinstance(min_area, torch.Tensor):
            min_area = min_area.tolist()
        table = [int(min_area)] * 256 if not hasattr(min_area, "__len__") else [int(v) for v in min_area]
        extra = {int(k): int(v) for k, v in dict(per_class or {}).items()}
    except (TypeError, ValueError):
        raise RuntimeError(f"mdil {fn}: min_area must be an integer or 256 of them, got {min_area!r}") from None
    if len(table) != 256:
        raise RuntimeError(f"mdil {fn}: min_area must be an integer or 256 of them, got {len(table)}")
    for k, v in extra.items():
        if not 0 <= k <= 255:
            raise RuntimeError(f"mdil {fn}: label {k} outside [0, 255]")
        table[k] = v
    if any(v < 0 or v > _segments_lib.MAX_EDGE for v in table):
        raise RuntimeError(f"mdil {fn}: areas must be within [0, {_segments_lib.MAX_EDGE}]")
    return torch.tensor(table, dtype=torch.int32)


def despeckle(map, min_area, keep_id=255, fill=255, connectivity=8):  # noqa: A002
    """``map`` (u8 [N,H,W] on the device) with every segment of fewer than ``min_area`` pixels (an int,
    or 256 of them indexed by the label byte) replaced by ``fill``; the label ``keep_id`` (-1: none) is
    never removed.  -> (out u8 [N,H,W], removed): ``removed`` = {"segments", "pixels"}, int64 [256]
    on the device, by label byte."""
    fn = "segments_filter"
    lib = _segments_lib.load()
    _check_map(fn, map, "map")
    hc.check_ignore_index(fn, keep_id)
    if not 0 <= int(fill) <= 255:
        raise RuntimeError(f"mdil {fn}: fill {fill} outside [0, 255]")
    table = min_area_table(min_area)
    N, H, W = map.shape
    with torch.no_grad(), torch.cuda.device(map.device):
        root, area = label(map, connectivity)
        least = table.to(map.device)
        out = torch.empty_like(map)
        removed = {k: torch.zeros(256, dtype=torch.int64, device=map.device) for k in ("segments", "pixels")}
        _segments_lib.check(
            lib.mdil_segments_filter(map.data_ptr(), root.data_ptr(), area.data_ptr(), N, H, W, least.data_ptr(),
                                     int(keep_id), int(fill), out.data_ptr(), removed["segments"].data_ptr(),
                                     removed["pixels"].data_ptr(), torch.cuda.current_stream(map.device).cuda_stream),
            "mdil_segments_filter")
    return out, removed


def _share(num, den):
    """num / den per cell, None where den is 0."""
    return [None if d == 0 else n / d for n, d in zip(num.reshape(-1).tolist(), den.reshape(-1).tolist())]


def _table(num, den):
    """{"total", "bins" [nb], "classes" [nc][nb]} of the ratio of two [nc,nb] counters."""
    nb = num.shape[1]
    cells = _share(num, den)
    return {"total": _share(num.sum().reshape(1), den.sum().reshape(1))[0], "bins": _share(num.sum(0), den.sum(0)),
            "classes": [cells[i:i + nb] for i in range(0, len(cells), nb)]}


def score(target_side, pred_side, edges, coverage):
    """The report of two sets of int64 host counters (the shapes of ``counter_shapes``), those of the
    ground truth's segments judged by the prediction and of the prediction's judged by the ground truth."""
    t, p = target_side, pred_side
    return {
        "edges": list(edges), "coverage": list(coverage),
        "segment_recall": _table(t["covered"], t["segments"]),
        "missed_share": _table(t["missed"], t["segments"]),
        "pixel_recall": _table(t["hit_pixels"], t["pixels"]),
        "segment_precision": _table(p["covered"], p["segments"]),
        "hallucinated_share": _table(p["missed"], p["segments"]),
        "target_segments": int(t["segments"].sum()), "pred_segments": int(p["segments"].sum()),
        "unjudged": {"target": t["unjudged"].tolist(), "pred": p["unjudged"].tolist()},
        "counters": {"target": {k: t[k].tolist() for k in COUNTERS}, "pred": {k: p[k].tolist() for k in COUNTERS}},
    }


class SegmentMeter:
    """Segment recall / precision of full-size predictions by segment size, counted on the device.
    Each ``add`` labels both maps and counts two sides: the ground truth's segments against the
    prediction (``ignore_index`` segments add to nothing) and the prediction's segments against the
    ground truth (their pixels under ``ignore_index`` are not judged)."""

    def __init__(self, nc, ignore_index, edges=DEFAULT_EDGES, coverage=DEFAULT_COVERAGE, connectivity=8):
        self.nc, self.ignore_index = int(nc), int(ignore_index)
        self.edges, self.coverage = check_edges(edges), check_coverage(coverage)
        self.connectivity = _check_connectivity("SegmentMeter", connectivity)
        self.nb = len(self.edges) + 1
        self.sides, self.workspace = {}, None

    def add(self, *source, target=None, overlap=False):
        """``add(pred, target)`` with two u8 [N,H,W] label maps in train ids on the device, or
        ``add(model, images, task, target=t)`` / ``add(features, weight, bias, target=t)``, which first
        run ``fullres.fullres_head`` for the label map of ``target``'s size.
        -> (pred, seen): ``seen`` = {"root", "area", "hit"} of the ground truth's segments (i32
        [N,H,W]) with ``overlap``, else None."""
        (pred,), target = ls.label_maps(("SegmentMeter", "segments_label", _PATH), source, target)
        if not self.sides:
            self.sides = {s: new_counters(self.nc, self.nb, pred.device) for s in ("target", "pred")}
        need = workspace_bytes(*pred.shape)
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, dtype=torch.uint8, device=pred.device)
        seen = None
        for side, a, b, a_ign, b_ign in (("target", target, pred, self.ignore_index, -1),
                                         ("pred", pred, target, -1, self.ignore_index)):
            root, area = label(a, self.connectivity, self.workspace)
            want = overlap and side == "target"
            hit, _ = segment_count(a, b, root, area, self.nc, self.edges, map_ignore=a_ign, other_ignore=b_ign,
                                   coverage=Fraction(*self.coverage), counters=self.sides[side],
                                   workspace=self.workspace, overlap=want)
            if want:
                seen = {"root": root, "area": area, "hit": hit}
        return pred, seen

    def counters(self):
        """{"target", "pred"} -> the seven counters as int64 host tensors; raises when a label outside
        [0, nc) (other than an ignored target) was met."""
        if not self.sides:
            shapes = counter_shapes(self.nc, self.nb)
            return {s: {k: torch.zeros(shapes[k], dtype=torch.int64) for k in COUNTERS} for s in ("target", "pred")}
        rc.refuse_bad_pixels("SegmentMeter", self.nc, self.ignore_index, self.sides["target"]["bad_labels"],
                             self.sides["pred"]["bad_labels"])
        return {s: {k: v.cpu() for k, v in c.items()} for s, c in self.sides.items()}

    def report(self):
        c = self.counters()
        out = score(c["target"], c["pred"], self.edges, self.coverage)
        out["connectivity"] = self.connectivity
        return out


# ------------------------------------------------------------------------------------------ CLI
GREY, COVERED, PARTLY, MISSED = (128, 128, 128), (0, 200, 0), (240, 170, 0), (220, 0, 0)


def segment_image(target, seen, coverage, ignore_index):
    """u8 [N,H,W,3] on the device: every pixel in the colour of its ground-truth segment -- covered,
    partly hit or missed --, ignored pixels grey.  From ``hit[root]`` and ``area[root]``."""
    N = target.shape[0]
    at = seen["root"].reshape(N, -1).long()
    hit = seen["hit"].reshape(N, -1).gather(1, at).reshape(target.shape).long()
    area = seen["area"].reshape(N, -1).gather(1, at).reshape(target.shape).long()
    num, den = coverage

    def colour(c):
        return torch.tensor(c, dtype=torch.uint8, device=target.device)

    img = colour(PARTLY).repeat(*target.shape, 1)
    img[hit * den >= num * area] = colour(COVERED)
    img[hit == 0] = colour(MISSED)
    img[target == ignore_index] = colour(GREY)
    return img


def _score_main(args):
    rc.refuse_task(args.task, args.num_classes)
    dev, nc, models, folders = ls.load_predictors(args)
    meter = SegmentMeter(nc, nc - 1, edges=args.edges, coverage=args.coverage, connectivity=args.connectivity)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    data = ls.open_data(args, nc)
    with hc.png_pool() as pool:
        png = hc.PngWriter(pool, args.out)
        for run in ls.label_runs(data, pool, dev, args.batch_size, models, args.task, folders, png):
            _, seen = meter.add(*run.sources, target=run.target, overlap=bool(args.out))
            if args.out:
                run.write("_segments.png",
                          segment_image(run.target, seen, meter.coverage, meter.ignore_index).cpu().numpy())
    report = ls.report_header(args, data[0], png)
    report.update(meter.report())
    if args.score:
        def pct(v):
            return "n/a" if v is None else f"{v * 100:.2f} %"
        print(f"{report['dataset']} (task {args.task}) at the labels' own size: {report['target_segments']} "
              f"ground-truth segments, recall {pct(report['segment_recall']['total'])}, missed "
              f"{pct(report['missed_share']['total'])}; {report['pred_segments']} predicted segments, precision "
              f"{pct(report['segment_precision']['total'])}, hallucinated {pct(report['hallucinated_share']['total'])}")
        lows = [0] + report["edges"]
        for k in range(meter.nb):
            span = f"{lows[k] + 1} to {report['edges'][k]}" if k < meter.nb - 1 else f"above {lows[k]}"
            print(f"area {span}: segment recall {pct(report['segment_recall']['bins'][k])}  pixel recall "
                  f"{pct(report['pixel_recall']['bins'][k])}  segment precision "
                  f"{pct(report['segment_precision']['bins'][k])}")
    return hc.score_report(report, None, args)


def read_map_png(path, name):
    """An 8-bit single-channel PNG as u8 [H,W]; anything else is refused by ``name``."""
    from PIL import Image
    with Image.open(path) as im:
        arr = np.array(im)
    if arr.ndim != 2 or arr.dtype != np.uint8:
        raise RuntimeError(f"--clean: {name} is not an 8-bit single-channel label map")
    return arr


def _clean_main(args):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pairs = args.min_area_class or []
    table = min_area_table(args.min_area, dict(zip(pairs[0::2], pairs[1::2])))
    names = sorted(os.path.relpath(os.path.join(d, f), args.clean)
                   for d, _, files in os.walk(args.clean) for f in files if f.lower().endswith(".png"))
    if not names:
        raise RuntimeError(f"--clean {args.clean}: no .png files found")
    total = {k: torch.zeros(256, dtype=torch.int64) for k in ("segments", "pixels")}
    with hc.png_pool() as pool:
        png = hc.PngWriter(pool, args.out)
        for name in names:
            arr = read_map_png(os.path.join(args.clean, name), name)
            out, removed = despeckle(torch.from_numpy(arr).to(dev)[None], table, keep_id=args.keep_id, fill=args.fill,
                                     connectivity=args.connectivity)
            for k in total:
                total[k] += removed[k].cpu()
            os.makedirs(os.path.dirname(os.path.join(args.out, name)), exist_ok=True)
            png.wait()
            png.submit(out[0].cpu().numpy(), name)
        png.wait()
    report = {"maps": len(names), "written": png.written, "min_area": table.tolist(), "keep_id": args.keep_id,
              "fill": args.fill, "connectivity": args.connectivity,
              "removed_segments": {str(c): int(v) for c, v in enumerate(total["segments"].tolist()) if v},
              "removed_pixels": {str(c): int(v) for c, v in enumerate(total["pixels"].tolist()) if v}}
    print(f"{len(names)} maps cleaned into {args.out}: {int(total['segments'].sum())} segments of "
          f"{int(total['pixels'].sum())} pixels removed")
    if args.json:
        hc.write_json(report, args.json)
    return report


def main(args):
    _refusals(args)
    return _clean_main(args) if args.clean else _score_main(args)


def _inside(inner, outer):
    inner, outer = os.path.realpath(inner), os.path.realpath(outer)
    return os.path.commonpath([inner, outer]) == outer


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused."""
    if args.clean:
        if args.score or args.pred or args.state:
            raise RuntimeError("--clean filters maps already written: it goes without --score, --pred and --state")
        if not args.out:
            raise RuntimeError("--clean needs --out DIR for the cleaned maps")
        if _inside(args.out, args.clean):
            raise RuntimeError(f"--out {args.out} is --clean {args.clean} or lies inside it: the cleaned maps would be "
                               "read as input")
        pairs = args.min_area_class or []
        if len(pairs) % 2 or any(not 0 <= c <= 255 for c in pairs[0::2]):
            raise RuntimeError("--min-area-class takes pairs of a label in [0, 255] and its smallest area")
        if args.min_area < 0 or any(a < 0 for a in pairs[1::2]):
            raise RuntimeError("--min-area and the areas of --min-area-class must not be negative")
        if not -1 <= args.keep_id <= 255 or not 0 <= args.fill <= 255:
            raise RuntimeError("--keep-id must be in [-1, 255] and --fill in [0, 255]")
        return
    ls.refuse_idle(args, ", or --clean DIR")
    ls.refuse_json_without_score(args)
    ls.refuse_sources(args)
    if args.num_classes is None or args.task is None:
        raise RuntimeError("scoring needs --num-classes and --task")
    check_edges(args.edges)
    check_coverage(args.coverage)
    ls.refuse_data(args)


def build_parser():
    p = ls.add_flags(hc.RefusingParser(_refusals, description="segment recall and precision by segment size at the "
                                                              "dataset's own size, and a despeckle filter for label "
                                                              "maps"),
                     label_maps=False, required=(), pred=True,      # --clean goes without a model
                     out_help="--score: write <stem>_segments.png at the image's own size into this folder; --clean: "
                              "the folder of the cleaned maps")
    p.add_argument("--edges", type=int, nargs="+", default=list(DEFAULT_EDGES),
                   help="area bins in pixels: 1 to 8 increasing values (default %(default)s)")
    p.add_argument("--coverage", default="0.5", help="share of a segment's judged pixels that must carry its label "
                                                     "for the segment to count as covered (default %(default)s)")
    p.add_argument("--connectivity", type=int, choices=(4, 8), default=8)
    p.add_argument("--clean", help="despeckle every 8-bit single-channel PNG under this folder into --out")
    p.add_argument("--min-area", type=int, default=16, help="--clean: segments of fewer pixels are removed "
                                                            "(default %(default)s)")
    p.add_argument("--min-area-class", type=int, nargs="+", metavar="N", help="--clean: pairs LABEL AREA that replace "
                                                                              "--min-area for single labels")
    p.add_argument("--keep-id", type=int, default=255, help="--clean: the label that is never removed, -1 for none "
                                                            "(default %(default)s)")
    p.add_argument("--fill", type=int, default=255, help="--clean: the label written in place of a removed segment "
                                                         "(default %(default)s)")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
