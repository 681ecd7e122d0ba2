"""Open-set report on MI355X: which pixels of a domain does the current head not know?  Per pixel
four scores (maximum softmax probability, max logit, free energy, entropy; higher = more likely
unknown), judged by AUROC, AUPR and FPR at 95 % TPR against pixels known to lie outside the head's
label set, and label maps with a reject id that ``boundary --pred``, ``segments --pred`` and
``segments --clean`` read.

    python -m mdil_ss_amd.openset --state CKPT --num-classes 20 20 27 --task 0 --dataset IDD --data-task 2 \
        --unknown-ids 18 25 --score --json FILE                  # head 0 on IDD, IDD's own ids as the unknowns
    python -m mdil_ss_amd.openset --state CKPT --num-classes 20 20 --task 0 --dataset cityscapes \
        --foreign-dataset BDD --foreign-task 1 --score --json FILE
    python -m mdil_ss_amd.openset --state CKPT --num-classes 20 20 --task 0 --dataset cityscapes \
        --fit THRESHOLDS.json --known-fpr 0.05
    python -m mdil_ss_amd.openset --state CKPT --num-classes 20 20 --task 0 --images DIR \
        --threshold THRESHOLDS.json --kind energy --out DIR [--unknown-id 255] [--colour]

Everything is counted, nothing is sorted (include/mdil_openset.h): ``openset_head`` forms the scores
in the head's registers, turns each into a 16-bit order-preserving code and adds to a
[kind][group][code] histogram of exact integers; the metrics below are integer prefix sums over that
table and go to fp64 at the last division.  ``tie_mass`` says how much the 16 bits can matter: the
AUROC of the codes is within half of it of the AUROC of the unquantised scores."""
import math
import os
from argparse import Namespace
from fractions import Fraction

import numpy as np
import torch

from . import _head_common as hc
from . import _openset_lib
from . import _report_common as rc

_PATH = "open-set"
KINDS = ("msp", "maxlogit", "energy", "entropy")
CODES = 65536
NONFINITE_CODE = 65535
FINITE_CODES = (128, 65407)                     # what a finite score can give; -inf 127, +inf 65408
CODE = torch.uint16
APPLY_COUNTERS = ("seen", "rejected", "detect", "confusion", "bad_targets", "bad_labels")
KNOWN, UNKNOWN, IGNORED = 0, 1, 2
DEFAULT_TPR = 0.95
DEFAULT_KNOWN_FPR = 0.05


# ------------------------------------------------------------------------------------- the key
def key16(t):
    """The 16-bit code of float32 scores (any device) as int64: the high half of the order-preserving
    key of ``t + 0.0`` (so -0 and +0 share a code).  u <= v implies key16(u) <= key16(v)."""
    t = torch.as_tensor(t, dtype=torch.float32) + 0.0
    bits = t.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    key = torch.where((bits & 0x80000000) != 0, ~bits & 0xffffffff, bits | 0x80000000)
    return key >> 16


def code_floor(code):
    """The smallest float32 of a code's bin: an int -> a float, a tensor / array -> a float32 tensor."""
    single = isinstance(code, int)
    c = np.asarray(code.cpu() if isinstance(code, torch.Tensor) else code, dtype=np.int64)
    shape, c = c.shape, c.reshape(-1)
    if ((c < 0) | (c >= CODES)).any():
        raise RuntimeError(f"mdil code_floor: codes lie in [0, {CODES}), got {code!r}")
    key = (c << 16).astype(np.uint32)
    bits = np.where(key & np.uint32(0x80000000), key & np.uint32(0x7fffffff), ~key).astype(np.uint32)
    f = bits.view(np.float32)
    return float(f[0]) if single else torch.from_numpy(f.copy()).reshape(shape)


def threshold_score(t):
    """A threshold code as a score for a report: ``code_floor`` inside the finite codes, else None."""
    return code_floor(int(t)) if FINITE_CODES[0] <= t <= FINITE_CODES[1] else None


code_values = hc.q_values                       # a stored code map as int64


def group_lut(unknown_ids=(), ignore_ids=()):
    """u8 [256] on the host: the group of every target byte -- 0 known, 1 for ``unknown_ids``, 2
    (ignored) for ``ignore_ids``."""
    lut = torch.zeros(256, dtype=torch.uint8)
    u, i = [int(v) for v in unknown_ids], [int(v) for v in ignore_ids]
    if any(not 0 <= v <= 255 for v in u + i):
        raise RuntimeError(f"mdil group_lut: ids lie in [0, 255], got unknown {u} ignore {i}")
    if set(u) & set(i):
        raise RuntimeError(f"mdil group_lut: {sorted(set(u) & set(i))} are both unknown and ignored")
    lut[u] = UNKNOWN
    lut[i] = IGNORED
    return lut


def kinds_mask(kinds):
    """Kind names or numbers -> the bit mask of ``openset_head`` (1..15)."""
    mask = 0
    for k in kinds:
        if isinstance(k, str) and k in KINDS:
            k = KINDS.index(k)
        if not isinstance(k, int) or not 0 <= k < len(KINDS):
            raise RuntimeError(f"mdil open-set: unknown score kind {k!r} (known: {list(KINDS)})")
        mask |= 1 << k
    if not mask:
        raise RuntimeError(f"mdil open-set: no score kind given (known: {list(KINDS)})")
    return mask


def check_nc(fn, nc):
    return hc.check_nc(fn, _openset_lib, nc)


# --------------------------------------------------------------------------------- entry points
def openset_head(features, weight, bias, target=None, lut=None, const_group=KNOWN, kinds=KINDS, map_kind=None,
                 hist=None, nonfinite=None, want_label=True):
    """``output_conv`` + argmax + the four scores on NHWC decoder features [N,H,W,16] and the
    ``ConvTranspose2d(16, nc, 2, 2)`` parameters, 2 <= nc <= 32, on the current stream.
    -> (label u8 [N,2H,2W] or None, code u16 [N,2H,2W] of kind ``map_kind`` or None).  ``hist``
    (int64 [4,2,65536], device) gains one count per kind of ``kinds`` and pixel at
    [kind][group][code], the group being ``lut[target]`` (u8 [256] and u8 [N,2H,2W] on the device) or
    ``const_group``; ``nonfinite`` (int64 [1]) one per pixel whose softmax sum or maximum is not
    finite.  Both are accumulated into, never cleared."""
    fn = "openset_head"
    lib = _openset_lib.load()
    for t, name in ((features, "features"), (weight, "weight"), (bias, "bias")):
        hc.chk(fn, _PATH, t, name)
    x, w, b = features, weight, bias
    nc = hc.check_params(fn, w, b, x)
    N, H, W = x.shape[0], x.shape[1], x.shape[2]
    hc.check_classes(fn, _openset_lib, nc, x, w, b)
    mask = kinds_mask(kinds)
    if map_kind is not None:
        map_kind = kinds_mask([map_kind]).bit_length() - 1
    if int(const_group) not in (KNOWN, UNKNOWN, IGNORED):
        raise RuntimeError(f"mdil {fn}: const_group {const_group} outside [0, 2]")
    if target is not None and lut is None:
        raise RuntimeError(f"mdil {fn}: a target needs its group look-up table (uint8 [256]) on the device")
    hc.check_tables(fn, _PATH, x.device, torch.uint8, ((target, "target", (N, 2 * H, 2 * W)), (lut, "lut", (256,))))
    hc.check_tables(fn, _PATH, x.device, torch.int64,
                    ((hist, "hist", (len(KINDS), 2, CODES)), (nonfinite, "nonfinite", (1,))))
    if not want_label and map_kind is None and hist is None and nonfinite is None:
        raise RuntimeError(f"mdil {fn}: nothing to do (no label, no code map, no hist, no nonfinite)")
    with torch.no_grad(), torch.cuda.device(x.device):
        label = torch.empty(N, 2 * H, 2 * W, dtype=torch.uint8, device=x.device) if want_label else None
        code = torch.empty(N, 2 * H, 2 * W, dtype=CODE, device=x.device) if map_kind is not None else None
        _openset_lib.check(
            lib.mdil_openset_head(x.data_ptr(), w.data_ptr(), b.data_ptr(), N, H, W, nc, hc.ptr(target),
                                  hc.ptr(lut if target is not None else None), int(const_group), mask,
                                  -1 if map_kind is None else map_kind, hc.ptr(label), hc.ptr(code), hc.ptr(hist),
                                  hc.ptr(nonfinite), torch.cuda.current_stream(x.device).cuda_stream),
            "mdil_openset_head")
    return label, code


def apply_counter_shapes(nc):
    return {"seen": (nc,), "rejected": (nc,), "detect": (2, 2), "confusion": (nc, nc), "bad_targets": (1,),
            "bad_labels": (1,)}


def new_apply_counters(nc, dev):
    """The six int64 counters of ``openset_apply`` for ``nc`` classes, zeroed, on ``dev``."""
    return hc.zero_counters(apply_counter_shapes(nc), dev)


def check_thr(fn, thr):
    try:
        t = int(thr)
    except (TypeError, ValueError):
        raise RuntimeError(f"mdil {fn}: thr must be an integer in [0, {CODES}], got {thr!r}") from None
    if not 0 <= t <= CODES:
        raise RuntimeError(f"mdil {fn}: thr must be an integer in [0, {CODES}] (a pixel is rejected when its code "
                           f">= thr), got {t}")
    return t


def openset_apply(label, code, nc, thr, id_map=None, unknown_id=255, cdf=None, target=None, lut=None, counters=None,
                  want_out=True):
    """The reject map of stored maps (any shape, one size), on the current stream:
    ``code >= thr ? unknown_id : id_map[label]`` -> (out u8 of ``label``'s shape or None without
    ``want_out``, score u8 = ``cdf[code]`` or None without ``cdf``).  ``thr``: an int in [0, 65536];
    ``id_map``: u8 [nc] on the device or None (identity); ``cdf``: u8 [65536] on the device
    (``cdf_lut``).  ``counters``: any of ``APPLY_COUNTERS`` as int64 device tensors (the shapes of
    ``apply_counter_shapes``), accumulated into; a ``target`` (u8, ``label``'s shape) needs its
    ``lut`` and "detect", "confusion" and "bad_targets"."""
    fn = "openset_apply"
    lib = _openset_lib.load()
    nc = check_nc(fn, nc)
    thr = check_thr(fn, thr)
    hc.check_id(fn, "unknown_id", unknown_id)
    hc.chk(fn, _PATH, label, "label", torch.uint8)
    hc.chk(fn, _PATH, code, "code", CODE)
    if label.numel() == 0 or label.shape != code.shape or label.device != code.device:
        raise RuntimeError(f"mdil {fn}: expects a uint8 label map and a uint16 code map of one shape on one device "
                           f"(got label {tuple(label.shape)} on {label.device}, code {tuple(code.shape)} on "
                           f"{code.device})")
    dev = label.device
    hc.check_tables(fn, _PATH, dev, torch.uint8, ((id_map, "id_map", (nc,)), (cdf, "cdf", (CODES,)),
                                                  (target, "target", tuple(label.shape)), (lut, "lut", (256,))))
    c = rc.check_counters(fn, counters, APPLY_COUNTERS)
    shapes = apply_counter_shapes(nc)
    hc.check_tables(fn, _PATH, dev, torch.int64, tuple((c[k], k, shapes[k]) for k in APPLY_COUNTERS))
    if target is not None and (lut is None or any(c[k] is None for k in ("detect", "confusion", "bad_targets"))):
        raise RuntimeError(f"mdil {fn}: a target needs its group look-up table (uint8 [256]) and the counters detect "
                           "(int64 [2,2]), confusion (int64 [nc,nc]) and bad_targets (int64 [1]) on the device; they "
                           "are accumulated into")
    if not want_out and cdf is None and all(v is None for v in c.values()):
        raise RuntimeError(f"mdil {fn}: nothing to do (no out map, no score map, no counters)")
    with torch.no_grad(), torch.cuda.device(dev):
        out = torch.empty_like(label) if want_out else None
        score = torch.empty_like(label) if cdf is not None else None
        _openset_lib.check(
            lib.mdil_openset_apply(label.data_ptr(), code.data_ptr(), label.numel(), nc, thr, hc.ptr(id_map),
                                   int(unknown_id), hc.ptr(cdf), hc.ptr(target),
                                   hc.ptr(lut if target is not None else None), hc.ptr(out), hc.ptr(score),
                                   *(hc.ptr(c[k]) for k in APPLY_COUNTERS),
                                   torch.cuda.current_stream(dev).cuda_stream),
            "mdil_openset_apply")
    return out, score


# ------------------------------------------------------------------------- the report arithmetic
def _rows(hist_kind, who):
    """One kind's [2][65536] table -> (known counts, unknown counts) as lists of Python ints."""
    h = torch.as_tensor(hist_kind)
    if h.is_cuda or tuple(h.shape) != (2, CODES) or h.dtype != torch.int64:
        raise RuntimeError(f"mdil {who}: expects a host int64 [2,{CODES}] table (got {tuple(h.shape)} {h.dtype} on "
                           f"{h.device})")
    return h[KNOWN].tolist(), h[UNKNOWN].tolist()


def _known_row(hist_known, who):
    h = torch.as_tensor(hist_known)
    if h.is_cuda or tuple(h.shape) != (CODES,) or h.dtype != torch.int64:
        raise RuntimeError(f"mdil {who}: expects a host int64 [{CODES}] table of the known pixels (got "
                           f"{tuple(h.shape)} {h.dtype} on {h.device})")
    n = int(h.sum())
    if n == 0:
        raise RuntimeError(f"mdil {who}: the known group is empty")
    return h, n


def _share(value, name):
    """A share given as a float, taken as the decimal it prints as -> an exact Fraction in [0, 1]."""
    f = Fraction(str(float(value)))
    if not 0 <= f <= 1:
        raise RuntimeError(f"mdil open-set: {name} {value} outside [0, 1]")
    return f


def metrics(hist_kind, tpr=DEFAULT_TPR):
    """AUROC, AUPR (unknown = positive), FPR at TPR ``tpr`` and the tie mass of one kind's
    [2][65536] table; N_b known and P_b unknown pixels in bin b, a pixel called unknown when its
    code >= t.  Integer prefix sums throughout, fp64 at the last division:
        auroc    = sum_b P_b (2 N_<b + N_b) / (2 P N)              ties count half
        aupr     = (1 / P) sum_b P_b TP_>=b / (TP_>=b + FP_>=b)     the step form
        fpr      = FP_>=t / N at the largest code t with TP_>=t >= ceil(tpr P)
        tie_mass = sum_b P_b N_b / (P N); |auroc of the codes - auroc of the scores| <= tie_mass / 2
    An empty group is refused by name."""
    known, unknown = _rows(hist_kind, "open-set metrics")
    N, P = sum(known), sum(unknown)
    for n, name in ((N, "known"), (P, "unknown")):
        if n == 0:
            raise RuntimeError(f"mdil open-set metrics: the {name} group is empty: there is nothing to rank against")
    need = math.ceil(_share(tpr, "tpr") * P)
    auroc_num = ties = 0
    below = 0
    for b in range(CODES):
        if unknown[b]:
            auroc_num += unknown[b] * (2 * below + known[b])
            ties += unknown[b] * known[b]
        below += known[b]
    tp = fp = 0
    terms, at = [], None
    for b in range(CODES - 1, -1, -1):
        tp += unknown[b]
        fp += known[b]
        if unknown[b]:
            terms.append(unknown[b] * tp / (tp + fp))
        if at is None and tp >= need:
            at = (b, fp)
    t, fp_t = at
    return {"auroc": auroc_num / (2 * P * N), "aupr": math.fsum(terms) / P, "fpr_at_tpr": fp_t / N, "tpr": float(tpr),
            "threshold_code": t, "threshold_score": threshold_score(t), "tie_mass": ties / (P * N), "P": P, "N": N}


def threshold_at_known_fpr(hist_known, fpr):
    """The smallest t in [0, 65536] with sum_{b >= t} N_b <= fpr N: rejecting code >= t rejects at
    most the share ``fpr`` of the known pixels.  Needs no unknown pixel."""
    h, n = _known_row(hist_known, "threshold_at_known_fpr")
    f = _share(fpr, "fpr")
    rows = h.tolist()
    t, tail = CODES, 0
    while t > 0 and (tail + rows[t - 1]) * f.denominator <= f.numerator * n:
        t -= 1
        tail += rows[t]
    return t


def cdf_lut(hist_known):
    """u8 [65536] on the host: floor(255 N_<=b / N), the share of the known pixels at or below a code."""
    h, n = _known_row(hist_known, "cdf_lut")
    return ((255 * h.cumsum(0)) // n).to(torch.uint8)


def cdf_starts(lut):
    """A ``cdf_lut`` as 256 ints: the first code at which it reaches v (65536: never)."""
    return torch.searchsorted(lut.to(torch.int64).contiguous(), torch.arange(256)).tolist()


def cdf_from_starts(starts):
    s = torch.as_tensor(starts, dtype=torch.int64)
    if tuple(s.shape) != (256,) or int(s[0]) != 0 or bool((s[1:] < s[:-1]).any()) or int(s.max()) > CODES:
        raise RuntimeError("mdil open-set: cdf_starts must be 256 ascending codes that begin at 0")
    return (torch.searchsorted(s, torch.arange(CODES), right=True) - 1).to(torch.uint8)


class OpenSetMeter:
    """The meter of this add-on: ``add`` runs the fused head on a batch and adds to the
    [kind][group][code] histogram on the device; ``report`` reads it back once and gives the metrics of
    every kind.  Groups come from ``lut`` (u8 [256], ``group_lut``) applied to the batch's target, or
    from ``const_group`` for batches without one."""

    def __init__(self, nc, kinds=KINDS, lut=None, const_group=KNOWN):
        self.nc = check_nc("OpenSetMeter", nc)
        self.mask = kinds_mask(kinds)
        self.kinds = tuple(k for i, k in enumerate(KINDS) if self.mask >> i & 1)
        if lut is not None and (not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint8 or lut.numel() != 256):
            raise RuntimeError("mdil OpenSetMeter: lut must be a uint8 [256] tensor (group_lut)")
        if int(const_group) not in (KNOWN, UNKNOWN, IGNORED):
            raise RuntimeError(f"mdil OpenSetMeter: const_group {const_group} outside [0, 2]")
        self.lut, self.const_group, self.tensors, self.pixels = lut, int(const_group), {}, 0

    def _head(self, x, w, b, **kw):
        return openset_head(x, w, b, kinds=self.kinds, hist=self.tensors["hist"], nonfinite=self.tensors["nonfinite"],
                            **kw)

    def _predict(self, model, images, task, **kw):
        model.eval()
        with torch.no_grad():
            feat = model.features(images, task).contiguous()
            w, b = model.head_params(task)
            return self._head(feat, w.detach(), b.detach(), **kw)

    def add(self, *source, target=None, const_group=None, map_kind=None, want_label=False):
        """``add(model, images, task)`` or ``add(features, weight, bias)``; ``target`` u8 [N,2H,2W] on
        the device (grouped by the meter's lut) or None (``const_group``, default the meter's).
        -> (label or None, code map of ``map_kind`` or None)."""
        if len(source) != 3:
            raise RuntimeError("mdil OpenSetMeter.add: expects (model, images, task) or (features, weight, bias)")
        fn, dev, N, H, W = rc.meter_source("OpenSetMeter", _PATH, source, 1, self._predict, self._head, "features")
        if target is not None and self.lut is None:
            raise RuntimeError("mdil OpenSetMeter.add: a target needs the meter's lut (group_lut)")
        if not self.tensors:
            self.tensors = {"hist": torch.zeros(len(KINDS), 2, CODES, dtype=torch.int64, device=dev),
                            "nonfinite": torch.zeros(1, dtype=torch.int64, device=dev)}
            if self.lut is not None:
                self.lut = self.lut.contiguous().to(dev)
        out = fn(*source, target=target, lut=self.lut if target is not None else None,
                 const_group=self.const_group if const_group is None else const_group, map_kind=map_kind,
                 want_label=want_label)
        self.pixels += N * 2 * H * 2 * W
        return out

    def hist(self):
        """The histogram as a host int64 [4,2,65536] tensor."""
        return self.tensors["hist"].cpu() if self.tensors else torch.zeros(len(KINDS), 2, CODES, dtype=torch.int64)

    def nonfinite(self):
        return int(self.tensors["nonfinite"].item()) if self.tensors else 0

    def report(self, tpr=DEFAULT_TPR):
        """-> {"pixels", "nonfinite", "kinds": {name: metrics(...)}}"""
        hist = self.hist()
        return {"pixels": self.pixels, "nonfinite": self.nonfinite(),
                "kinds": {k: metrics(hist[KINDS.index(k)], tpr) for k in self.kinds}}


# ------------------------------------------------------------------------------------------ CLI
def _data_args(args, dataset, task, synthetic):
    """``args`` as ``_report_common.batches`` reads them, for another dataset / label space."""
    d = Namespace(**vars(args))
    d.dataset, d.task, d.synthetic = dataset, task, synthetic
    return d


def _score(args, model, dev, nc_data):
    foreign = bool(args.foreign_dataset or args.foreign_synthetic)
    void = nc_data - 1
    if foreign:                                        # every non-void pixel of the set is known
        lut = group_lut((), sorted({void, *args.ignore_ids}))
        unknown_ids = []
    else:
        unknown_ids = list(args.unknown_ids) if args.unknown_ids else [void]
        lut = group_lut(unknown_ids, args.ignore_ids)
    meter = OpenSetMeter(args.num_classes[args.task], args.kinds, lut)
    images_seen = 0
    for _, images, target in rc.batches(_data_args(args, args.dataset, args.data_task, args.synthetic), nc_data, dev):
        meter.add(model, images, args.task, target=target)
        images_seen += images.shape[0]
    foreign_seen = 0
    if foreign:
        f_task = args.foreign_task
        f_args = _data_args(args, args.foreign_dataset, f_task, args.foreign_synthetic)
        for _, images, _ in rc.batches(f_args, args.num_classes[f_task], dev, score=False):
            meter.add(model, images, args.task, const_group=UNKNOWN)
            foreign_seen += images.shape[0]
    report = {"mode": "score", "dataset": rc.source_name(args), "task": args.task, "data_task": args.data_task,
              "images": images_seen, "unknown_ids": unknown_ids, "ignore_ids": list(args.ignore_ids)}
    if foreign:
        report.update(foreign_dataset="synthetic" if args.foreign_synthetic else args.foreign_dataset,
                      foreign_task=args.foreign_task, foreign_images=foreign_seen)
    report.update(meter.report(args.tpr))
    hist = meter.hist()
    for k, m in report["kinds"].items():               # the occupied bins: the metrics can be formed again from them
        m["hist"] = {name: [[int(b), int(hist[KINDS.index(k), g, b])] for b in hist[KINDS.index(k), g].nonzero().reshape(-1)]
                     for g, name in ((KNOWN, "known"), (UNKNOWN, "unknown"))}
    for k, m in report["kinds"].items():
        print(f"{k:9s} AUROC {m['auroc'] * 100:6.2f} %  AUPR {m['aupr'] * 100:6.2f} %  FPR at {args.tpr * 100:g} % TPR "
              f"{m['fpr_at_tpr'] * 100:6.2f} % (code >= {m['threshold_code']})  tie mass {m['tie_mass']:.3g}  "
              f"P {m['P']}  N {m['N']}")
    print(f"{report['nonfinite']} non-finite pixels")
    return report, meter


def _fit(args, model, dev, nc_data):
    unknown_ids = list(args.unknown_ids) if args.unknown_ids else [nc_data - 1]
    meter = OpenSetMeter(args.num_classes[args.task], args.kinds, group_lut(unknown_ids, args.ignore_ids))
    n = 0
    for _, images, target in rc.batches(_data_args(args, args.dataset, args.data_task, args.synthetic), nc_data, dev):
        meter.add(model, images, args.task, target=target)
        n += images.shape[0]
    hist = meter.hist()
    fitted = {}
    for k in meter.kinds:
        known = hist[KINDS.index(k), KNOWN]
        t = threshold_at_known_fpr(known, args.known_fpr)
        fitted[k] = {"threshold_code": t, "threshold_score": threshold_score(t), "known_pixels": int(known.sum()),
                     "rejected_known": int(known[t:].sum()), "cdf_starts": cdf_starts(cdf_lut(known))}
        print(f"{k:9s} reject code >= {t} (score >= {fitted[k]['threshold_score']}): "
              f"{fitted[k]['rejected_known']} of {fitted[k]['known_pixels']} known pixels")
    report = {"mode": "fit", "dataset": rc.source_name(args), "task": args.task, "data_task": args.data_task, "images": n,
              "known_fpr": args.known_fpr, "unknown_ids": unknown_ids, "ignore_ids": list(args.ignore_ids),
              "num_classes": args.num_classes[args.task], "nonfinite": meter.nonfinite(), "kinds": fitted}
    hc.write_json(report, args.fit)
    return report, meter


def read_threshold(path, kind, nc):
    """The fit of ``kind`` in a ``--fit`` file -> (threshold code, cdf u8 [65536] on the host)."""
    import json
    with open(path) as f:
        saved = json.load(f)
    if saved.get("mode") != "fit" or kind not in saved.get("kinds", {}):
        raise RuntimeError(f"--threshold {path}: not a --fit file that holds the kind {kind}")
    if saved.get("num_classes") != nc:
        raise RuntimeError(f"--threshold {path}: fitted on a head of {saved.get('num_classes')} classes, this one has {nc}")
    k = saved["kinds"][kind]
    return check_thr("--threshold", k["threshold_code"]), cdf_from_starts(k["cdf_starts"])


def _write_maps(args, model, dev, nc):
    from . import predict as P
    thr, cdf = read_threshold(args.threshold, args.kind, nc)
    cdf = cdf.to(dev)
    os.makedirs(args.out, exist_ok=True)
    palette = None
    if args.colour:                                    # the classes' colours; white for the reject id
        palette = torch.full((256, 3), 255, dtype=torch.uint8)
        palette[:nc] = P.default_palette(nc)
        palette = palette.to(dev)
    meter = OpenSetMeter(nc, [args.kind])
    counters = new_apply_counters(nc, dev)
    some = {k: counters[k] for k in ("seen", "rejected", "bad_labels")}
    n = 0
    with hc.png_pool() as pool:
        png = hc.PngWriter(pool, args.out)
        nc_data = None if args.images else args.num_classes[args.data_task]
        for stems, images, _ in rc.image_or_dataset_batches(_data_args(args, None, args.data_task, args.synthetic), nc_data,
                                                            pool, dev, score=False):
            label, code = meter.add(model, images, args.task, const_group=IGNORED, map_kind=args.kind, want_label=True)
            out, score = openset_apply(label, code, nc, thr, None, args.unknown_id, cdf, counters=some)
            planes = [out.unsqueeze(3), score.unsqueeze(3)]
            if palette is not None:
                planes.append(palette[out.long()])
            host = torch.cat(planes, 3).cpu().numpy()
            png.wait()                                 # the batch before this one: bounds what is in flight
            for j, stem in enumerate(stems):
                png.submit(host[j, :, :, 0], f"{stem}_label.png")
                png.submit(host[j, :, :, 1], f"{stem}_unknown.png")
                if palette is not None:
                    png.submit(host[j, :, :, 2:5], f"{stem}_colour.png")
            n += len(stems)
        png.wait()
    seen, rejected = counters["seen"].tolist(), counters["rejected"].tolist()
    report = {"mode": "maps", "dataset": rc.source_name(args), "task": args.task, "images": n, "kind": args.kind,
              "threshold_code": thr, "unknown_id": args.unknown_id, "seen": seen, "rejected": rejected,
              "rejected_share": sum(rejected) / max(1, sum(seen)), "nonfinite": meter.nonfinite(),
              "written": png.written}
    print(f"{n} images: {report['rejected_share'] * 100:.2f} % of {sum(seen)} pixels rejected ({args.kind} code >= {thr}); "
          f"{len(png.written)} maps written to {args.out}")
    return report, meter


def main(args):
    _refusals(args)
    rc.refuse_task(args.task, args.num_classes)
    if args.data_task is None:
        args.data_task = args.task
    if args.foreign_task is None:
        args.foreign_task = args.task
    for name, t in (("--data-task", args.data_task), ("--foreign-task", args.foreign_task)):
        if not 0 <= t < len(args.num_classes):
            raise RuntimeError(f"{name} {t}: the model has tasks 0 to {len(args.num_classes) - 1}")
    if args.foreign_synthetic and args.foreign_task == args.data_task:
        raise RuntimeError("--foreign-synthetic draws the domain of --foreign-task, which is --data-task's: the same "
                           "images; give another --foreign-task")
    nc_data = args.num_classes[args.data_task]
    for name, ids in (("--unknown-ids", args.unknown_ids), ("--ignore-ids", args.ignore_ids)):
        if any(not 0 <= v < nc_data for v in ids):
            raise RuntimeError(f"{name} {ids}: task {args.data_task}'s labels lie in [0, {nc_data})")
    if args.threshold and not os.path.isfile(args.threshold):
        raise RuntimeError(f"--threshold {args.threshold}: no such file")
    dev, nc, model = hc.load_model(args.state, args.num_classes, args.task)
    if args.score:
        report, meter = _score(args, model, dev, nc_data)
    elif args.fit:
        report, meter = _fit(args, model, dev, nc_data)
    else:
        report, meter = _write_maps(args, model, dev, nc)
    if args.json:
        hc.write_json(report, args.json)
    return report


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused."""
    modes = [bool(args.score), bool(args.fit), bool(args.out)]
    if sum(modes) != 1:
        raise RuntimeError("give one of --score (with --json FILE), --fit FILE or --out DIR (with --threshold FILE)")
    if args.score and not args.json:
        raise RuntimeError("--score writes its report to --json FILE")
    if args.out and not args.threshold:
        raise RuntimeError("--out DIR needs --threshold FILE (written by --fit)")
    if args.threshold and not args.out:
        raise RuntimeError("--threshold FILE goes with --out DIR")
    if args.out:
        if sum(bool(v) for v in (args.images, args.synthetic)) != 1 or args.dataset:
            raise RuntimeError("--out DIR needs one source of images: --images DIR or --synthetic N")
    else:
        if args.images:
            raise RuntimeError("--images DIR has no labels: it goes with --threshold FILE and --out DIR")
        if sum(bool(v) for v in (args.dataset, args.synthetic)) != 1:
            raise RuntimeError("give --dataset cityscapes|BDD|IDD or --synthetic N (not both)")
    if (args.foreign_dataset or args.foreign_synthetic) and not args.score:
        raise RuntimeError("--foreign-dataset goes with --score")
    if args.foreign_dataset and args.foreign_synthetic:
        raise RuntimeError("--foreign-dataset and --foreign-synthetic exclude each other")
    if (args.foreign_dataset or args.foreign_synthetic) and args.unknown_ids:
        raise RuntimeError("--foreign-dataset makes every pixel of the foreign images the unknowns: --unknown-ids does "
                           "not go with it")
    if min(args.height, args.width, args.batch_size) < 1 or args.synthetic < 0 or args.foreign_synthetic < 0:
        raise RuntimeError("sizes and --batch-size must be positive")
    if not 0.0 < args.tpr <= 1.0:
        raise RuntimeError(f"--tpr {args.tpr} outside (0, 1]")
    if not 0.0 <= args.known_fpr <= 1.0:
        raise RuntimeError(f"--known-fpr {args.known_fpr} outside [0, 1]")
    if not 0 <= args.unknown_id <= 255:
        raise RuntimeError(f"--unknown-id {args.unknown_id} outside [0, 255]")
    if set(args.unknown_ids) & set(args.ignore_ids):
        raise RuntimeError("--unknown-ids and --ignore-ids share an id")
    if args.out and args.kind not in KINDS:
        raise RuntimeError(f"--kind {args.kind}: one of {list(KINDS)}")


def build_parser():
    p = hc.RefusingParser(_refusals, description="open-set report of a checkpoint: unknown-pixel scores, AUROC / AUPR / "
                                                 "FPR at 95 % TPR, reject thresholds and label maps with a reject id")
    p.add_argument("--state", required=True, help="checkpoint written by the trainers (or by the reference)")
    p.add_argument("--num-classes", type=int, nargs="+", required=True)
    p.add_argument("--task", type=int, required=True, help="which task's decoder is judged")
    rc.add_data_flags(p, dataset_help="a labelled dataset", synthetic_help="N procedural images instead (labelled)")
    p.add_argument("--data-task", type=int, help="open the dataset in this task's label space (default --task)")
    p.add_argument("--score", action="store_true", help="judge the scores against the unknown pixels; needs --json")
    p.add_argument("--unknown-ids", type=int, nargs="+", default=[],
                   help="target ids that count as unknown (default: the void class of --data-task)")
    p.add_argument("--ignore-ids", type=int, nargs="+", default=[], help="target ids left out of both groups")
    p.add_argument("--kinds", nargs="+", choices=KINDS, default=list(KINDS))
    p.add_argument("--tpr", type=float, default=DEFAULT_TPR, help="the TPR at which the FPR is read (default %(default)s)")
    p.add_argument("--foreign-dataset", choices=("cityscapes", "BDD", "IDD"),
                   help="with --score: every pixel of this dataset's images is unknown, every non-void pixel of "
                        "--dataset known")
    p.add_argument("--foreign-synthetic", type=int, default=0, help="N procedural images of --foreign-task's domain instead")
    p.add_argument("--foreign-task", type=int, help="the label space / domain of the foreign images (default --task)")
    p.add_argument("--fit", help="write per kind the reject threshold at --known-fpr and the known pixels' CDF here")
    p.add_argument("--known-fpr", type=float, default=DEFAULT_KNOWN_FPR,
                   help="share of the known pixels that the fitted threshold may reject (default %(default)s)")
    p.add_argument("--images", help="folder of unlabelled .jpg / .png images (searched recursively)")
    p.add_argument("--threshold", help="a file written by --fit")
    p.add_argument("--kind", default="energy", help="the score that rejects (default %(default)s)")
    p.add_argument("--out", help="write <stem>_label.png (train ids, --unknown-id where rejected) and <stem>_unknown.png here")
    p.add_argument("--unknown-id", type=int, default=255)
    p.add_argument("--colour", action="store_true", help="also write <stem>_colour.png (white where rejected)")
    p.add_argument("--json", help="write the report here")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
