"""Pseudo-labels for a domain that has images but no label files, on MI355X: class-balanced
self-training (Zou et al., ECCV 2018).  The head that exists predicts the new domain's images, per
class only the most confident share of the predicted pixels is kept, and those are written as
train-id label maps with everything else 255 -- files the trainers read unchanged.

    python -m mdil_ss_amd.pseudo --state model_best_....pth.tar --num-classes 20 20 --task 1 \
        --images DIR --portion 0.2 --out-root ROOT --layout BDD --subset train [--json FILE]
    python -m mdil_ss_amd.pseudo --state model_best_....pth.tar --num-classes 20 20 --task 1 \
        --dataset BDD --subset val --portion 0.2 --json FILE            # how good would they be

The selection is exact and needs no sort (include/mdil_pseudo.h): ``pseudo_head`` writes the label
and the winner's softmax confidence as 16 bits per pixel and counts a [class][high byte] histogram;
the host finds the byte that holds rank k of each class; ``pseudo_refine`` counts the low byte
inside that byte over the stored maps; ``pseudo_apply`` writes the thresholded maps and counts
what was kept (and, with ground truth, how right it is).  The maps of a whole split stay in HBM,
3 bytes per pixel."""
import math
import os

import numpy as np
import torch

from . import _head_common as hc
from . import _pseudo_lib
from . import _report_common as rc

_PATH = "pseudo-label"
Q_ONE = 65536                                   # q = min(65535, floor(conf * Q_ONE)); thr = Q_ONE keeps nothing
QCONF = torch.uint16
APPLY_COUNTERS = ("seen", "kept", "confusion", "bad_targets", "bad_labels")
DEFAULT_PORTION = 0.2


q_values = hc.q_values                          # the stored confidences as int64


def check_nc(fn, nc):
    return hc.check_nc(fn, _pseudo_lib, nc)


def check_thr(fn, thr, nc):
    """-> the thresholds as a list of nc ints in [0, 65536]."""
    return hc.check_q_thresholds(fn, thr, nc, Q_ONE, "the pseudo-label path keeps a pixel of class c when q >= thr[c]")


def check_portion(portion, nc):
    """A scalar or one value per class, each in [0, 1] -> a list of nc floats."""
    try:
        p = [float(v) for v in portion] if isinstance(portion, (list, tuple, torch.Tensor, np.ndarray)) else \
            [float(portion)]
    except (TypeError, ValueError):
        raise RuntimeError(f"mdil pseudo-label thresholds: portion must be numbers, got {portion!r}") from None
    if len(p) == 1:
        p = p * nc
    if len(p) != nc or any(not 0.0 <= v <= 1.0 for v in p):
        raise RuntimeError(f"mdil pseudo-label thresholds: portion must be one value or {nc} values in [0, 1], got "
                           f"{portion!r}")
    return p


def _maps(fn, label, qconf):
    hc.chk(fn, _PATH, label, "label", torch.uint8)
    hc.chk(fn, _PATH, qconf, "qconf", QCONF)
    if label.numel() == 0 or label.shape != qconf.shape or label.device != qconf.device:
        raise RuntimeError(f"mdil {fn}: expects a uint8 label map and a uint16 qconf map of one shape on one device "
                           f"(got label {tuple(label.shape)} on {label.device}, qconf {tuple(qconf.shape)} on "
                           f"{qconf.device})")


# --------------------------------------------------------------------------------- entry points
def pseudo_head(features, weight, bias, hist=None, nonfinite=None, want_label=True, want_qconf=True):
    """``output_conv`` + argmax + 16-bit confidence on NHWC decoder features [N,H,W,16] and the
    ``ConvTranspose2d(16, nc, 2, 2)`` parameters, 2 <= nc <= 32, on the current stream.
    -> (label u8 [N,2H,2W] or None, qconf u16 [N,2H,2W] or None); ``hist`` (int64 [nc,256], device)
    gains one count per pixel at [label][q >> 8] and ``nonfinite`` (int64 [1]) one per NaN
    confidence; both are accumulated into, never cleared."""
    fn = "pseudo_head"
    lib = _pseudo_lib.load()
    for t, name in ((features, "features"), (weight, "weight"), (bias, "bias")):
        hc.chk(fn, _PATH, t, name)
    x, w, b = features, weight, bias
    nc = hc.check_params(fn, w, b, x)
    N, H, W = x.shape[0], x.shape[1], x.shape[2]
    hc.check_classes(fn, _pseudo_lib, nc, x, w, b)
    hc.check_tables(fn, _PATH, x.device, torch.int64, ((hist, "hist", (nc, 256)), (nonfinite, "nonfinite", (1,))))
    if not want_label and not want_qconf and hist is None:
        raise RuntimeError(f"mdil {fn}: nothing to do (no label, no qconf, no hist)")
    with torch.no_grad(), torch.cuda.device(x.device):
        label = torch.empty(N, 2 * H, 2 * W, dtype=torch.uint8, device=x.device) if want_label else None
        qconf = torch.empty(N, 2 * H, 2 * W, dtype=QCONF, device=x.device) if want_qconf else None
        _pseudo_lib.check(
            lib.mdil_pseudo_head(x.data_ptr(), w.data_ptr(), b.data_ptr(), N, H, W, nc, hc.ptr(label), hc.ptr(qconf),
                                 hc.ptr(hist), hc.ptr(nonfinite), torch.cuda.current_stream(x.device).cuda_stream),
            "mdil_pseudo_head")
    return label, qconf


def pseudo_refine(label, qconf, nc, sel, hist2, bad_labels):
    """Level 2 over stored maps (any shape, one size): ``hist2`` (int64 [nc,256], device) gains one
    count at [label][q & 255] for every pixel with (q >> 8) == sel[label]; ``sel``: nc ints (-1 skips
    the class) or an int32 device tensor.  Labels >= nc are counted in ``bad_labels`` (int64 [1])."""
    fn = "pseudo_refine"
    lib = _pseudo_lib.load()
    nc = check_nc(fn, nc)
    _maps(fn, label, qconf)
    dev = label.device
    if not isinstance(sel, torch.Tensor):
        s = [int(v) for v in sel]
        if len(s) != nc or any(v < -1 or v > 255 for v in s):
            raise RuntimeError(f"mdil {fn}: sel must be {nc} high bytes in [-1, 255], got {s}")
        sel = torch.tensor(s, dtype=torch.int32).to(dev)
    hc.check_tables(fn, _PATH, dev, torch.int32, ((sel, "sel", (nc,)),))
    if hist2 is None or bad_labels is None:
        raise RuntimeError(f"mdil {fn}: hist2 (int64 [nc,256]) and bad_labels (int64 [1]) are needed on the device; "
                           "they are accumulated into")
    hc.check_tables(fn, _PATH, dev, torch.int64, ((hist2, "hist2", (nc, 256)), (bad_labels, "bad_labels", (1,))))
    with torch.no_grad(), torch.cuda.device(dev):
        _pseudo_lib.check(
            lib.mdil_pseudo_refine(label.data_ptr(), qconf.data_ptr(), label.numel(), nc, sel.data_ptr(),
                                   hist2.data_ptr(), bad_labels.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
            "mdil_pseudo_refine")


def new_apply_counters(nc, dev):
    """The five int64 counters of ``pseudo_apply`` for ``nc`` classes, zeroed, on ``dev``."""
    return hc.zero_counters(apply_counter_shapes(nc), dev)


def apply_counter_shapes(nc):
    return {"seen": (nc,), "kept": (nc,), "confusion": (nc, nc), "bad_targets": (1,), "bad_labels": (1,)}


def pseudo_apply(label, qconf, nc, thr, id_map=None, drop_id=255, target=None, ignore_index=-1, counters=None,
                 want_out=True):
    """The thresholded map of stored maps (any shape, one size), on the current stream:
    ``q >= thr[label] ? id_map[label] : drop_id`` -> out u8 of ``label``'s shape (None without
    ``want_out``).  ``thr``: nc ints in [0, 65536], or an int32 [nc] device tensor, which is not
    read back (the kernel compares q with any int); ``id_map``: u8 [nc] on the device or None
    (identity).  ``counters``: any of ``APPLY_COUNTERS`` as int64 device tensors (the shapes of
    ``apply_counter_shapes``), accumulated into; a ``target`` (u8, ``label``'s shape) needs
    "confusion" and "bad_targets"."""
    fn = "pseudo_apply"
    lib = _pseudo_lib.load()
    nc = check_nc(fn, nc)
    on_device = isinstance(thr, torch.Tensor) and thr.is_cuda
    if not on_device:
        thr = check_thr(fn, thr, nc)
    hc.check_id(fn, "drop_id", drop_id)
    hc.check_ignore_index(fn, ignore_index)
    _maps(fn, label, qconf)
    dev = label.device
    hc.check_tables(fn, _PATH, dev, torch.uint8, ((id_map, "id_map", (nc,)), (target, "target", tuple(label.shape))))
    if on_device:                                      # taken as it is: reading it back would stall the stream
        hc.check_tables(fn, _PATH, dev, torch.int32, ((thr, "thr", (nc,)),))
    c = rc.check_counters(fn, counters, APPLY_COUNTERS)
    shapes = apply_counter_shapes(nc)
    hc.check_tables(fn, _PATH, dev, torch.int64, tuple((c[k], k, shapes[k]) for k in APPLY_COUNTERS))
    if target is not None and (c["confusion"] is None or c["bad_targets"] is None):
        raise RuntimeError(f"mdil {fn}: a target needs the counters confusion (int64 [nc,nc]) and bad_targets "
                           "(int64 [1]) on the device; they are accumulated into")
    if not want_out and all(v is None for v in c.values()):
        raise RuntimeError(f"mdil {fn}: nothing to do (no out map, no counters)")
    with torch.no_grad(), torch.cuda.device(dev):
        thr_d = thr if on_device else torch.tensor(thr, dtype=torch.int32).to(dev)
        out = torch.empty_like(label) if want_out else None
        _pseudo_lib.check(
            lib.mdil_pseudo_apply(label.data_ptr(), qconf.data_ptr(), label.numel(), nc, thr_d.data_ptr(),
                                  hc.ptr(id_map), int(drop_id), hc.ptr(target), int(ignore_index), hc.ptr(out),
                                  *(hc.ptr(c[k]) for k in APPLY_COUNTERS), torch.cuda.current_stream(dev).cuda_stream),
            "mdil_pseudo_apply")
    return out


# ------------------------------------------------------------------------------------- selection
def ranks(hist, portion):
    """k_c = floor(p_c * n_c) with n_c = hist[c].sum(): how many pixels of class c the portion asks for."""
    nc = hist.shape[0]
    p = check_portion(portion, nc)
    return [math.floor(p[c] * int(hist[c].sum())) for c in range(nc)]


def floor_q(floor):
    if not 0.0 <= float(floor) <= 1.0:
        raise RuntimeError(f"mdil pseudo-label thresholds: floor {floor} outside [0, 1]")
    return min(Q_ONE, math.ceil(float(floor) * Q_ONE))


def _walk_down(counts, rank):
    """-> (the highest bin b with sum(counts[b:]) >= rank, the count above b); rank >= 1."""
    above = 0
    for b in range(255, -1, -1):
        if above + counts[b] >= rank:
            return b, above
        above += counts[b]
    raise RuntimeError(f"mdil pseudo-label thresholds: rank {rank} is beyond the {above} pixels counted")


def thresholds(hist, refine, portion, floor=0.0):
    """The class-balanced thresholds, on the host (torch on CPU only).  ``hist``: int64 [nc,256], the
    level-1 histogram [class][q >> 8]; ``refine(sel)``: given nc high bytes (-1: skip), returns the
    level-2 histogram int64 [nc,256] of q & 255 over the pixels of class c with q >> 8 == sel[c].
    -> thr, nc ints: thr_c is the k_c-th largest q among the pixels predicted as c, k_c =
    floor(p_c * n_c), so every pixel tied with it is kept (kept_c >= k_c); k_c = 0 gives 65536
    (nothing kept); finally thr_c = max(thr_c, ceil(floor * 65536)).

    Exact: rank k_c lies in the high byte sel_c where the count walked down from 255 first reaches
    k_c; it is rank r_c = k_c - count(high > sel_c) inside that byte, and the low byte where the
    level-2 count walked down first reaches r_c completes the 16 bits."""
    hist = torch.as_tensor(hist)
    if hist.is_cuda or hist.dim() != 2 or hist.shape[1] != 256 or hist.dtype != torch.int64:
        raise RuntimeError(f"mdil pseudo-label thresholds: hist must be a host int64 [nc,256] tensor (got "
                           f"{tuple(hist.shape)} {hist.dtype} on {hist.device})")
    nc = hist.shape[0]
    k = ranks(hist, portion)
    fq = floor_q(floor)
    rows = hist.tolist()
    sel, left = [-1] * nc, [0] * nc
    for c in range(nc):
        if k[c] > 0:
            sel[c], above = _walk_down(rows[c], k[c])
            left[c] = k[c] - above
    thr = [Q_ONE] * nc
    if any(s >= 0 for s in sel):
        hist2 = torch.as_tensor(refine(list(sel))).cpu()
        if tuple(hist2.shape) != (nc, 256):
            raise RuntimeError(f"mdil pseudo-label thresholds: refine returned {tuple(hist2.shape)}, not [{nc},256]")
        rows2 = hist2.tolist()
        for c in range(nc):
            if sel[c] < 0:
                continue
            if sum(rows2[c]) != rows[c][sel[c]]:
                raise RuntimeError(f"mdil pseudo-label thresholds: class {c}: level 2 counted {sum(rows2[c])} pixels "
                                   f"in high byte {sel[c]}, level 1 {rows[c][sel[c]]}; the maps are not the ones the "
                                   "histogram was counted from")
            thr[c] = sel[c] * 256 + _walk_down(rows2[c], left[c])[0]
    return [max(v, fq) for v in thr]


class PseudoLabeller:
    """The meter of this add-on: ``add`` predicts a batch and keeps its label and confidence maps in
    HBM (3 bytes per pixel: Cityscapes train is 4.7 GB, BDD train 11 GB) while the level-1 histogram
    accumulates; ``thresholds`` is one ``pseudo_refine`` pass over what is stored; ``apply`` yields
    the thresholded maps chunk by chunk and fills ``seen`` / ``kept`` / ``confusion``."""

    def __init__(self, nc, store_gb=64.0):
        self.nc = check_nc("PseudoLabeller", nc)
        self.store_bytes = float(store_gb) * 1e9
        self.chunks, self.stored, self.tensors, self.counters = [], 0, {}, None

    def _head(self, x, w, b):
        return pseudo_head(x, w, b, self.tensors["hist"], self.tensors["nonfinite"])

    def _predict(self, model, images, task):
        model.eval()
        with torch.no_grad():
            feat = model.features(images, task).contiguous()
            w, b = model.head_params(task)
            return self._head(feat, w.detach(), b.detach())

    def add(self, *source):
        """``add(model, images, task)`` or ``add(features, weight, bias)`` -> (label, qconf) of the
        batch, which are also stored."""
        if len(source) != 3:
            raise RuntimeError("mdil PseudoLabeller.add: expects (model, images, task) or (features, weight, bias)")
        fn, dev, N, H, W = rc.meter_source("PseudoLabeller", _PATH, source, 1, self._predict, self._head, "features")
        need = 3 * N * 2 * H * 2 * W
        if self.stored + need > self.store_bytes:
            raise RuntimeError(f"mdil PseudoLabeller.add: the stored maps would take {(self.stored + need) / 1e9:.3f} "
                               f"GB of device memory, above store_gb = {self.store_bytes / 1e9:g}; raise store_gb or "
                               "label the split in parts")
        if not self.tensors:
            self.tensors = {"hist": torch.zeros(self.nc, 256, dtype=torch.int64, device=dev),
                            "nonfinite": torch.zeros(1, dtype=torch.int64, device=dev)}
        label, qconf = fn(*source)
        self.chunks.append((label, qconf))
        self.stored += need
        return label, qconf

    def hist(self):
        """The level-1 histogram as a host int64 [nc,256] tensor."""
        return self.tensors["hist"].cpu() if self.tensors else torch.zeros(self.nc, 256, dtype=torch.int64)

    def nonfinite(self):
        return int(self.tensors["nonfinite"].item()) if self.tensors else 0

    def refine(self, sel):
        """Level 2 over every stored chunk -> host int64 [nc,256]."""
        if not self.chunks:
            return torch.zeros(self.nc, 256, dtype=torch.int64)
        dev = self.chunks[0][0].device
        hist2 = torch.zeros(self.nc, 256, dtype=torch.int64, device=dev)
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        sel_d = torch.tensor([int(v) for v in sel], dtype=torch.int32).to(dev)
        for label, qconf in self.chunks:
            pseudo_refine(label, qconf, self.nc, sel_d, hist2, bad)
        if int(bad.item()):
            raise RuntimeError(f"mdil PseudoLabeller: {int(bad.item())} stored labels are outside [0, {self.nc})")
        return hist2.cpu()

    def thresholds(self, portion=DEFAULT_PORTION, floor=0.0):
        return thresholds(self.hist(), self.refine, portion, floor)

    def apply(self, thr, id_map=None, drop_id=255, targets=None, ignore_index=-1, want_out=True):
        """Yields the thresholded map (u8, the chunk's shape; None without ``want_out``) of every
        stored chunk, in the order of ``add``.  ``targets``: one u8 device tensor per chunk.
        ``self.counters`` (host int64 tensors) hold seen / kept / confusion once the iteration has
        ended; it ends with a RuntimeError when a target outside [0, nc) that is not
        ``ignore_index`` was met."""
        thr = check_thr("PseudoLabeller.apply", thr, self.nc)
        if targets is not None:
            targets = list(targets)
            if len(targets) != len(self.chunks):
                raise RuntimeError(f"mdil PseudoLabeller.apply: {len(targets)} targets for {len(self.chunks)} chunks")
        self.counters = None
        if not self.chunks:
            self.counters = {k: torch.zeros(s, dtype=torch.int64) for k, s in apply_counter_shapes(self.nc).items()}
            return
        dev = self.chunks[0][0].device
        if id_map is not None:
            id_map = torch.as_tensor(id_map, dtype=torch.uint8).contiguous().to(dev)
        tensors = new_apply_counters(self.nc, dev)
        given = {k: v for k, v in tensors.items() if targets is not None or k not in ("confusion", "bad_targets")}
        thr_d = torch.tensor(thr, dtype=torch.int32).to(dev)
        for i, (label, qconf) in enumerate(self.chunks):
            yield pseudo_apply(label, qconf, self.nc, thr_d, id_map, drop_id,
                               None if targets is None else targets[i], ignore_index, given, want_out)
        rc.refuse_bad_targets("PseudoLabeller", tensors, self.nc, ignore_index)
        bad = int(tensors["bad_labels"].item())
        if bad:
            raise RuntimeError(f"mdil PseudoLabeller: {bad} stored labels are outside [0, {self.nc})")
        self.counters = {k: v.cpu() for k, v in tensors.items()}


def precision(confusion):
    """Per predicted class: the share of the counted pixels whose target is that class (float64;
    0 where the class was never predicted)."""
    m = torch.as_tensor(confusion).double()
    return (m.diagonal() / m.sum(0).clamp(min=1.0)).tolist()


# ------------------------------------------------------------------------------------------ CLI
LAYOUTS = {"cityscapes": ("leftImg8bit", "gtFine"), "BDD": ("images", "labels")}


def label_name(layout, stem):
    """The label file the ``layout``'s loader pairs with the image ``stem``."""
    if layout == "BDD":
        return f"{stem}_train_id.png"
    if stem.endswith("_leftImg8bit"):
        stem = stem[:-len("_leftImg8bit")]
    return f"{stem}_gtFine_labelTrainIds.png"


def plan_tree(args, files):
    """The label paths (relative to the labels' folder) of ``files`` under ``--out-root`` and the
    image link; refuses names whose sorted label list would not pair with the sorted image list."""
    img_dir, lab_dir = LAYOUTS[args.layout]
    root = os.path.abspath(args.images)
    rel = [os.path.relpath(os.path.abspath(f), root) for f in files]
    names = [os.path.join(os.path.dirname(r), label_name(args.layout, os.path.splitext(os.path.basename(r))[0]))
             for r in rel]
    if len(set(names)) != len(names):
        raise RuntimeError(f"--out-root: two images under {args.images} would share one label file")
    if [names[i] for i in sorted(range(len(rel)), key=lambda i: rel[i])] != sorted(names):
        raise RuntimeError(f"--out-root: the {args.layout} loader pairs the sorted image list with the sorted label "
                           f"list, and the image names under {args.images} sort differently from their label names; "
                           "rename the images")
    link = os.path.join(args.out_root, img_dir, args.subset)
    labels = os.path.join(args.out_root, lab_dir, args.subset)
    os.makedirs(os.path.dirname(link), exist_ok=True)
    if os.path.lexists(link):                          # the images' own folder, or the link of an earlier run
        if os.path.realpath(link) != os.path.realpath(root):
            raise RuntimeError(f"--out-root: {link} exists and is not the folder of --images ({root})")
    else:
        os.symlink(root, link, target_is_directory=True)
    for d in sorted({os.path.dirname(n) for n in names}):
        os.makedirs(os.path.join(labels, d), exist_ok=True)
    return labels, names


def main(args):
    _refusals(args)
    rc.refuse_task(args.task, args.num_classes)
    nc = args.num_classes[args.task]
    portion = check_portion(args.portion if len(args.portion) > 1 else args.portion[0], nc)
    dev, nc, model = hc.load_model(args.state, args.num_classes, args.task)
    out_dir, names = args.out, None
    if args.out_root:
        from . import predict as P
        out_dir, names = plan_tree(args, P._image_files(args.images)[0])
    elif args.out:
        os.makedirs(args.out, exist_ok=True)
    meter = PseudoLabeller(nc, args.store_gb)
    stems, targets = [], []
    with hc.png_pool() as pool:
        for s, images, target in rc.image_or_dataset_batches(args, nc, pool, dev, unique_stems=bool(args.out)):
            meter.add(model, images, args.task)
            stems.extend(s)
            if target is not None:
                targets.append(target)
        scored = bool(targets)
        hist = meter.hist()
        k = ranks(hist, portion)
        thr = meter.thresholds(portion, args.floor)
        id_map = torch.arange(nc, dtype=torch.uint8)
        if not args.keep_void:
            id_map[nc - 1] = 255                       # the trainers' relabelled ignore class
        if names is None:
            names = [f"{s}_pseudo.png" for s in stems]
        png = hc.PngWriter(pool, out_dir)
        i0 = 0
        for out in meter.apply(thr, id_map, 255, targets if scored else None, nc - 1, want_out=bool(out_dir)):
            if out_dir:
                host = out.cpu().numpy()
                png.wait()                             # the batch before this one: bounds what is in flight
                for j in range(host.shape[0]):
                    png.submit(host[j], names[i0 + j])
                i0 += host.shape[0]
        png.wait()
        counters = meter.counters
        if scored:                                     # the same figures for every pixel: threshold 0
            for _ in meter.apply([0] * nc, id_map, 255, targets, nc - 1, want_out=False):
                pass
            everything = meter.counters
    seen, kept = counters["seen"].tolist(), counters["kept"].tolist()
    report = {"dataset": rc.source_name(args), "task": args.task, "images": len(stems), "written": png.written, "portion": portion, "floor": args.floor,
              "seen": seen, "kept": kept, "thr": thr, "thr_probability": [t / Q_ONE for t in thr], "k": k,
              "kept_share": sum(kept) / max(1, sum(seen)), "nonfinite": meter.nonfinite(),
              "hist": hist.tolist()}
    print(f"{report['dataset']} (task {args.task}): {len(stems)} images, kept {report['kept_share'] * 100:.2f} % of "
          f"{sum(seen)} pixels; {report['nonfinite']} non-finite confidences")
    print("thresholds: " + " ".join(f"{t / Q_ONE:.4f}" for t in thr))
    if scored:
        report.update(precision_kept=precision(counters["confusion"]), confusion_kept=counters["confusion"].tolist(),
                      precision_all=precision(everything["confusion"]),
                      confusion_all=everything["confusion"].tolist())
        print("precision of the kept pixels: " + " ".join(f"{v * 100:.2f}" for v in report["precision_kept"]))
        print("precision of all pixels:      " + " ".join(f"{v * 100:.2f}" for v in report["precision_all"]))
    if out_dir:
        print(f"{len(png.written)} maps written to {out_dir}")
    if args.json:
        hc.write_json(report, args.json)
    return report


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused."""
    if sum(bool(v) for v in (args.images, args.dataset, args.synthetic)) != 1:
        raise RuntimeError("give one source of images: --images DIR, --dataset cityscapes|BDD|IDD or --synthetic N")
    if args.layout == "IDD":
        raise RuntimeError("--layout IDD is not supported: the IDD loaders remap level-3 ids, so the label files would "
                           "need the inverse map; write --layout cityscapes or BDD")
    if args.out_root and not args.images:
        raise RuntimeError("--out-root writes a tree beside the images: it needs --images DIR")
    if bool(args.out_root) != bool(args.layout):
        raise RuntimeError("--out-root and --layout cityscapes|BDD go together")
    if args.out_root and args.out:
        raise RuntimeError("--out and --out-root exclude each other")
    if not args.out and not args.out_root and not args.json:
        raise RuntimeError("nothing to do: give --out DIR, --out-root DIR or --json FILE")
    if min(args.height, args.width, args.batch_size) < 1 or args.synthetic < 0:
        raise RuntimeError("sizes and --batch-size must be positive")
    if any(not 0.0 <= p <= 1.0 for p in args.portion):
        raise RuntimeError(f"--portion {args.portion}: every value must be in [0, 1]")
    if 0 <= args.task < len(args.num_classes) and len(args.portion) not in (1, args.num_classes[args.task]):
        raise RuntimeError(f"--portion: one value or {args.num_classes[args.task]} (one per class), got "
                           f"{len(args.portion)}")
    if not 0.0 <= args.floor <= 1.0:
        raise RuntimeError(f"--floor {args.floor} outside [0, 1]")
    if not args.store_gb > 0:
        raise RuntimeError("--store-gb must be positive")


def build_parser():
    p = hc.RefusingParser(_refusals, description="class-balanced pseudo-labels from a checkpoint: train-id label "
                                                 "maps of the most confident pixels per class")
    p.add_argument("--state", required=True, help="checkpoint written by the trainers (or by the reference)")
    p.add_argument("--num-classes", type=int, nargs="+", required=True)
    p.add_argument("--task", type=int, required=True, help="which task's decoder predicts")
    p.add_argument("--images", help="folder of unlabelled .jpg / .png images (searched recursively)")
    rc.add_data_flags(p, dataset_help="a labelled dataset instead: the report also says how right the pseudo-labels "
                                      "are", synthetic_help="N procedural images instead (labelled)")
    p.set_defaults(subset="train")
    p.add_argument("--portion", type=float, nargs="+", default=[DEFAULT_PORTION],
                   help="share of each class's predicted pixels to keep: one value or one per class (default "
                        "%(default)s)")
    p.add_argument("--floor", type=float, default=0.0, help="never keep a pixel below this confidence")
    p.add_argument("--keep-void", action="store_true",
                   help="write the last class (the trainers' relabelled ignore class) as itself, not as 255")
    p.add_argument("--out", help="write <stem>_pseudo.png here: 8-bit train ids, 255 = unlabelled")
    p.add_argument("--out-root", help="with --images: write a dataset tree the trainers open as --cs-datadir / "
                                      "--bdd-datadir")
    p.add_argument("--layout", choices=("cityscapes", "BDD", "IDD"), help="the tree --out-root writes")
    p.add_argument("--json", help="write the report here")
    p.add_argument("--store-gb", type=float, default=64.0, help="device memory the stored maps may take")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
