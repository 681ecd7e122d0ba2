"""How far an mIoU would move on another validation set of the same size, on MI355X: per-image class
counts of full-size label maps, and the image-level bootstrap, the jackknife and -- for two
predictors on the same images -- the paired bootstrap and the label-swap randomisation test of the
difference of their mIoUs (include/mdil_signif.h).  The image is the sampling unit; the counts and
the replicate sums are exact integers, a replicate is a function of (seed, replicate index) alone.

    python -m mdil_ss_amd.significance --state model_best_....pth.tar --num-classes 20 20 27 --task 0 \
        --dataset cityscapes [--cs-datadir ...] [--replicates 10000] [--seed 0] [--level 0.95] [--influence 10] \
        [--json FILE]
    python -m mdil_ss_amd.significance --before STEP1.pth.tar --before-num-classes 20 --after STEP2.pth.tar \
        --after-num-classes 20 20 --task 0 --dataset cityscapes --json FILE
    python -m mdil_ss_amd.significance --pred MAPS_A [--pred-b MAPS_B] --num-classes 20 20 27 --task 0 \
        --dataset cityscapes

``--state`` scores one checkpoint at the labels' own size (the label maps of ``mdil_ss_amd.fullres``);
``--before`` / ``--after`` compare two checkpoints on the same images; ``--pred`` reads the
``<stem>_label.png`` files in train ids that ``predict`` / ``fullres`` / ``ensemble`` wrote, and with
``--pred-b`` compares two such folders.  The report gives the mIoU and every class IoU with the
bootstrap standard error, the percentile and the BCa interval, how many replicates lacked a class,
the images whose removal moves the mIoU most and, for a pair, the difference B - A with its
intervals, the paired-bootstrap and the label-swap p-values."""
import os
from statistics import NormalDist

import numpy as np
import torch

from . import _head_common as hc
from . import _labelsize_common as ls
from . import _report_common as rc
from . import _signif_lib

_PATH = "significance"
MODES = {"bootstrap": _signif_lib.BOOTSTRAP, "jackknife": _signif_lib.JACKKNIFE, "swap": _signif_lib.SWAP}


def _chk(fn, t, name, dtype=torch.uint8):
    hc.chk(fn, _PATH, t, name, dtype)


def _check_classes(fn, nc):
    nc = int(nc)
    if not _signif_lib.MIN_CLASSES <= nc <= _signif_lib.MAX_CLASSES:
        raise RuntimeError(f"mdil {fn}: {nc} classes (supported: {_signif_lib.MIN_CLASSES} to "
                           f"{_signif_lib.MAX_CLASSES})")
    return nc


def scored_classes(nc, ignore_index):
    """-> k, the classes that enter the mean: nc - 1 when the last class is ignored, nc when
    ``ignore_index`` is no class; any other class is refused (iouEval's rule)."""
    if 0 <= ignore_index < nc - 1:
        raise RuntimeError(f"mdil significance: ignore_index {ignore_index}: the ignore class must be the last one, "
                           f"{nc - 1}, or outside [0, {nc})")
    return nc - 1 if ignore_index == nc - 1 else nc


def new_counts(M, G, nc, dev):
    """A zeroed count table int64 [M,G,3,nc] on ``dev``: tp, predicted and labelled pixels per image,
    group (predictor) and class."""
    return torch.zeros(M, G, 3, nc, dtype=torch.int64, device=dev)


def _check_table(fn, counts, nc):
    _chk(fn, counts, "counts", torch.int64)
    if counts.dim() != 4 or tuple(counts.shape[2:]) != (3, nc) or not 1 <= counts.shape[1] <= _signif_lib.MAX_GROUPS \
            or not 1 <= counts.shape[0] <= _signif_lib.MAX_IMAGES:
        raise RuntimeError(f"mdil {fn}: counts must be int64 [M,G,3,{nc}] with 1 <= M <= {_signif_lib.MAX_IMAGES} and "
                           f"G in 1..{_signif_lib.MAX_GROUPS} (got {tuple(counts.shape)})")
    return counts.shape[0], counts.shape[1]


def image_counts(pred, target, nc, *, ignore_index, counts, first_image, group=0, stray=None):
    """Counts the pixels of ``pred`` against ``target`` (u8 [N,H,W] label maps in train ids on the
    device) INTO the rows ``first_image`` .. ``first_image + N - 1`` of group ``group`` of ``counts``
    (int64 [M,G,3,nc] on the device, accumulated into, never cleared), on the current stream.
    -> ``stray``: int64 [2] on the device, accumulated into (allocated when None): targets outside
    [0, nc) other than ``ignore_index``, and counted pixels whose prediction is outside [0, nc)."""
    fn = "signif_count"
    lib = _signif_lib.load()
    _chk(fn, pred, "pred")
    _chk(fn, target, "target")
    if pred.dim() != 3 or pred.numel() == 0 or pred.shape != target.shape or pred.device != target.device:
        raise RuntimeError(f"mdil {fn}: pred {tuple(pred.shape)} on {pred.device} and target {tuple(target.shape)} on "
                           f"{target.device} must be uint8 [N,H,W] maps of one size on one device")
    nc = _check_classes(fn, nc)
    hc.check_ignore_index(fn, ignore_index)
    M, G = _check_table(fn, counts, nc)
    N, H, W = pred.shape
    first_image, group = int(first_image), int(group)
    if counts.device != pred.device or not 0 <= group < G or not 0 <= first_image <= M - N:
        raise RuntimeError(f"mdil {fn}: rows {first_image} .. {first_image + N - 1} of group {group} are outside the "
                           f"table {tuple(counts.shape)} on {counts.device} (maps on {pred.device})")
    with torch.no_grad(), torch.cuda.device(pred.device):
        if stray is None:
            stray = torch.zeros(2, dtype=torch.int64, device=pred.device)
        hc.check_tables(fn, _PATH, pred.device, torch.int64, ((stray, "stray", (2,)),))
        _signif_lib.check(
            lib.mdil_signif_count(pred.data_ptr(), target.data_ptr(), N, H, W, nc, int(ignore_index), first_image, M, G,
                                  group, counts.data_ptr(), stray.data_ptr(), stray.data_ptr() + 8,
                                  torch.cuda.current_stream(pred.device).cuda_stream),
            "mdil_signif_count")
    return stray


def resample(counts, nc, ignore_index, mode, replicates, seed, first_replicate=0, *, sums=False, iou=True,
             empty=True, check_entries=True):
    """Replicates ``first_replicate`` .. ``first_replicate + replicates - 1`` of the summed table
    ``counts`` (int64 [M,G,3,nc] on the device, entries in [0, 2^31)), ``mode`` "bootstrap",
    "jackknife" or "swap", scored by the iouEval rule, on the current stream.
    -> {"miou" f64 [B,G], "iou" f64 [B,G,k], "empty" int64 [B,G] (bit c: class c absent), "sums" int64
    [B,G,3,nc]}, on the device; the last three only where asked for.  ``check_entries`` reads the
    table's range back first (one synchronisation)."""
    fn = "signif_resample"
    lib = _signif_lib.load()
    nc = _check_classes(fn, nc)
    M, G = _check_table(fn, counts, nc)
    hc.check_ignore_index(fn, ignore_index)
    k = scored_classes(nc, int(ignore_index))
    if mode not in MODES:
        raise RuntimeError(f"mdil {fn}: mode must be one of {sorted(MODES)}, got {mode!r}")
    if mode == "swap" and G != 2:
        raise RuntimeError(f"mdil {fn}: the swap mode exchanges two predictors: it needs a table of two groups "
                           f"(got {G})")
    B, first, seed = int(replicates), int(first_replicate), int(seed)
    if B < 1 or first < 0 or first + B > _signif_lib.MAX_REPLICATES:
        raise RuntimeError(f"mdil {fn}: replicates {first} .. {first + B - 1} are outside [0, 2^32)")
    if mode == "jackknife" and first + B > M:
        raise RuntimeError(f"mdil {fn}: the jackknife of {M} images has {M} replicates (asked for {first} .. "
                           f"{first + B - 1})")
    if not 0 <= seed < 1 << 64:
        raise RuntimeError(f"mdil {fn}: seed {seed} outside [0, 2^64)")
    dev = counts.device
    with torch.no_grad(), torch.cuda.device(dev):
        if check_entries:
            lo, hi = int(counts.min().item()), int(counts.max().item())
            if lo < 0 or hi >= _signif_lib.MAX_ENTRY:
                raise RuntimeError(f"mdil {fn}: the entries of counts must be in [0, 2^31) (got {lo} .. {hi})")
        out = {"miou": torch.empty(B, G, dtype=torch.float64, device=dev)}
        if iou:
            out["iou"] = torch.empty(B, G, k, dtype=torch.float64, device=dev)
        mask = torch.empty(B, G, dtype=torch.int32, device=dev) if empty else None
        if sums:
            out["sums"] = torch.empty(B, G, 3, nc, dtype=torch.int64, device=dev)
        _signif_lib.check(
            lib.mdil_signif_resample(counts.data_ptr(), M, G, nc, int(ignore_index), MODES[mode], first, B, seed,
                                     hc.ptr(out.get("sums")), out["miou"].data_ptr(), hc.ptr(out.get("iou")),
                                     hc.ptr(mask), torch.cuda.current_stream(dev).cuda_stream),
            "mdil_signif_resample")
        if empty:
            out["empty"] = mask.to(torch.int64) & 0xffffffff
    return out


# ------------------------------------------------------------------------- host side, float64
def score_counts(total, nc, ignore_index):
    """The iouEval rule on an integer table [..., 3, nc] (tp, predicted, labelled), as the kernel
    spells it: tp / (tp + (predicted - tp) + (labelled - tp) + 1e-15) on float64, the mean added in
    class order.  -> (miou [...], iou [..., k], empty [...]: bit c set where class c is absent)."""
    k = scored_classes(nc, int(ignore_index))
    t = np.asarray(total, dtype=np.int64)
    both, pr, lb = (t[..., p, :].astype(np.float64) for p in range(3))
    iou = (both / (both + (pr - both) + (lb - both) + 1e-15))[..., :k]
    s = np.zeros(iou.shape[:-1])
    for c in range(k):
        s = s + iou[..., c]
    empty = (((t[..., 1, :] + t[..., 2, :]) == 0).astype(np.int64) << np.arange(nc)).sum(-1)
    return s / float(k), iou, empty


def intervals(theta_hat, boot, jack, level):
    """``boot``: the bootstrap replicates of a statistic, ``jack``: its leave-one-image-out values,
    ``theta_hat``: its value on the whole set.  -> {"se": the bootstrap standard error (ddof = 1),
    "percentile": [lo, hi] by ``numpy.quantile`` (linear), "bca": [lo, hi] or None, "bca_reason": why
    not, "z0", "acceleration"}.  BCa: z0 = Phi^-1((#{boot < theta_hat} + #{boot == theta_hat} / 2) / B);
    a = sum d^3 / (6 (sum d^2)^1.5) over d = mean(jack) - jack (0 where the jackknife values are all
    equal); the quantiles are taken at Phi(z0 + (z0 + z) / (1 - a (z0 + z))), z = Phi^-1 of the
    percentile interval's two levels."""
    boot, jack, theta_hat = np.asarray(boot, dtype=np.float64), np.asarray(jack, dtype=np.float64), float(theta_hat)
    if boot.ndim != 1 or boot.size < 2 or jack.ndim != 1 or jack.size < 1:
        raise RuntimeError("mdil significance: intervals need at least 2 bootstrap replicates and 1 jackknife value")
    if not 0.0 < level < 1.0:
        raise RuntimeError(f"mdil significance: level {level} outside (0, 1)")
    lo, hi = (1.0 - level) / 2.0, 1.0 - (1.0 - level) / 2.0
    out = {"se": float(boot.std(ddof=1)), "percentile": [float(v) for v in np.quantile(boot, [lo, hi])],
           "bca": None, "bca_reason": None, "z0": None, "acceleration": None}
    share = (np.count_nonzero(boot < theta_hat) + 0.5 * np.count_nonzero(boot == theta_hat)) / boot.size
    d = jack.mean() - jack
    den = float((d * d).sum())
    a = float((d ** 3).sum() / (6.0 * den ** 1.5)) if den > 0.0 else 0.0
    out["acceleration"] = a
    if share <= 0.0 or share >= 1.0:
        out["bca_reason"] = (f"z0 is infinite: {'no' if share <= 0.0 else 'every'} bootstrap replicate lies below the "
                             "estimate")
        return out
    normal = NormalDist()
    z0 = normal.inv_cdf(share)
    out["z0"] = z0
    at = []
    for q in (lo, hi):
        z = z0 + normal.inv_cdf(q)
        if 1.0 - a * z <= 0.0:
            out["bca_reason"] = f"the acceleration {a:.3g} puts the adjusted level outside the normal range"
            return out
        at.append(normal.cdf(z0 + z / (1.0 - a * z)))
    out["bca"] = [float(v) for v in np.quantile(boot, at)]
    return out


def _influence(theta_hat, jack, stems, n):
    """The ``n`` images whose removal moves the statistic most: |theta_hat - theta(-i)| descending,
    the image index ascending among equals."""
    change = np.asarray(jack, dtype=np.float64) - theta_hat
    order = sorted(range(change.size), key=lambda i: (-abs(change[i]), i))[:max(0, int(n))]
    return [{"image": i, "stem": stems[i], "without": float(jack[i]), "change": float(change[i])} for i in order]


def build_report(total, boot, jack, swap, nc, ignore_index, stems, *, level=0.95, influence=10, seed=0):
    """The report from the whole set's integer table ``total`` [G,3,nc] and the replicates as host
    arrays: ``boot`` and ``jack`` = {"miou" [B,G], "iou" [B,G,k], "empty" [B,G] (boot only)},
    ``swap`` = {"miou" [B,2]} or None.  Everything here is host float64."""
    total = np.asarray(total, dtype=np.int64)
    G, k = total.shape[0], scored_classes(nc, int(ignore_index))
    miou, iou, _ = score_counts(total, nc, ignore_index)
    bm, bi, be = (np.asarray(boot[key]) for key in ("miou", "iou", "empty"))
    jm, ji = np.asarray(jack["miou"]), np.asarray(jack["iou"])
    B = bm.shape[0]
    report = {"images": int(jm.shape[0]), "classes": k, "replicates": int(B), "seed": int(seed), "level": float(level),
              "paired": G == 2, "predictors": []}
    for g in range(G):
        row = {"mIoU": dict(value=float(miou[g]), **intervals(miou[g], bm[:, g], jm[:, g], level)),
               "iou_classes": [dict(value=float(iou[g, c]), **intervals(iou[g, c], bi[:, g, c], ji[:, g, c], level))
                               for c in range(k)],
               "empty_replicates": [int(((be[:, g].astype(np.int64) >> c) & 1).sum()) for c in range(k)],
               "influence": _influence(float(miou[g]), jm[:, g], stems, influence),
               "counts": total[g].tolist()}
        report["predictors"].append(row)
    if G == 2:
        delta, d_boot, d_jack = float(miou[1] - miou[0]), bm[:, 1] - bm[:, 0], jm[:, 1] - jm[:, 0]
        d_swap = np.asarray(swap["miou"])[:, 1] - np.asarray(swap["miou"])[:, 0]
        below, above = int(np.count_nonzero(d_boot <= 0.0)), int(np.count_nonzero(d_boot >= 0.0))
        report["delta"] = dict(
            value=delta, **intervals(delta, d_boot, d_jack, level),
            p_boot=min(1.0, 2.0 * min(below + 1, above + 1) / (B + 1)),
            p_swap=(1 + int(np.count_nonzero(np.abs(d_swap) >= abs(delta)))) / (d_swap.size + 1),
            classes=[{"value": float(iou[1, c] - iou[0, c]),
                      "percentile": [float(v) for v in np.quantile(bi[:, 1, c] - bi[:, 0, c],
                                                                    [(1.0 - level) / 2.0, 1.0 - (1.0 - level) / 2.0])]}
                     for c in range(k)],
            influence=_influence(delta, d_jack, stems, influence))
    return report


class SignificanceMeter:
    """Per-image class counts of full-size predictions, kept on the device, and their resampling.
    ``paired``: two predictors on the same images (groups 0 = A and 1 = B of the table)."""

    def __init__(self, nc, ignore_index, paired=False):
        self.nc, self.ignore_index = _check_classes("SignificanceMeter", nc), int(ignore_index)
        hc.check_ignore_index("SignificanceMeter", self.ignore_index)
        self.k = scored_classes(self.nc, self.ignore_index)
        self.paired, self.G = bool(paired), 2 if paired else 1
        self.counts = self.stray = None
        self.images, self.stems = 0, []

    def add(self, *source, target=None, stems=None):
        """Unpaired: ``add(pred, target)`` with two u8 [N,H,W] label maps in train ids on the device,
        ``add(model, images, task, target=t)`` or ``add(features, weight, bias, target=t)``, which first
        run ``fullres.fullres_head`` for the label map of ``target``'s size.  Paired: ``add(a, b,
        target=t)``, each of ``a`` and ``b`` a label map or such a triple.  ``stems``: the images'
        names for the influence list.  -> the label maps, one per predictor."""
        who = "SignificanceMeter.add"
        preds, target = ls.label_maps(("SignificanceMeter", "signif_count", _PATH), source, target, self.paired)
        N = target.shape[0]
        stems = [f"image_{self.images + i:06d}" for i in range(N)] if stems is None else [str(s) for s in stems]
        if len(stems) != N:
            raise RuntimeError(f"mdil {who}: {len(stems)} stems for {N} images")
        if self.images + N > _signif_lib.MAX_IMAGES:
            raise RuntimeError(f"mdil {who}: more than {_signif_lib.MAX_IMAGES} images")
        if self.counts is None or self.images + N > self.counts.shape[0]:
            rows = min(_signif_lib.MAX_IMAGES, max(64, 2 * (self.images + N)))
            grown = new_counts(rows, self.G, self.nc, target.device)
            if self.counts is not None:
                grown[:self.images] = self.counts[:self.images]
            self.counts = grown
        for g, p in enumerate(preds):
            self.stray = image_counts(p, target, self.nc, ignore_index=self.ignore_index, counts=self.counts,
                                      first_image=self.images, group=g, stray=self.stray)
        self.images += N
        self.stems += stems
        return preds

    def table(self):
        """int64 [M,G,3,nc] on the device: the rows counted so far; raises when a target outside
        [0, nc) (other than the ignore index) was met."""
        if not self.images:
            raise RuntimeError("mdil SignificanceMeter: no image was added")
        rc.refuse_bad_pixels("SignificanceMeter", self.nc, self.ignore_index, self.stray[0])
        return self.counts[:self.images].contiguous()

    def report(self, replicates=10000, seed=0, level=0.95, influence=10):
        check_settings(replicates, seed, level, influence)
        table = self.table()
        args = (table, self.nc, self.ignore_index)
        boot = resample(*args, "bootstrap", replicates, seed)
        jack = resample(*args, "jackknife", self.images, seed, empty=False, check_entries=False)
        swap = resample(*args, "swap", replicates, seed, iou=False, empty=False, check_entries=False) \
            if self.paired else None

        def host(d):
            return None if d is None else {key: v.cpu().numpy() for key, v in d.items()}

        out = build_report(table.sum(0).cpu().numpy(), host(boot), host(jack), host(swap), self.nc, self.ignore_index,
                           self.stems, level=level, influence=influence, seed=seed)
        out["unpredicted_pixels"] = int(self.stray[1].item())
        return out


def check_settings(replicates, seed, level, influence, flags=False):
    """``flags``: word the refusals by the command line's flags."""
    names = ("--replicates", "--seed", "--level", "--influence") if flags else \
        ("replicates", "seed", "level", "influence")
    if not 2 <= int(replicates) <= _signif_lib.MAX_REPLICATES:
        raise RuntimeError(f"{names[0]} {replicates}: the standard error needs 2 replicates, and there are at most "
                           "2^32")
    if not 0 <= int(seed) < 1 << 64:
        raise RuntimeError(f"{names[1]} {seed} outside [0, 2^64)")
    if not 0.0 < float(level) < 1.0:
        raise RuntimeError(f"{names[2]} {level} outside (0, 1)")
    if int(influence) < 0:
        raise RuntimeError(f"{names[3]} {influence} must not be negative")


# ------------------------------------------------------------------------------------------ CLI
def _pct(v):
    return f"{v * 100:.2f}"


def _interval(row):
    lo, hi = row["bca"] if row["bca"] is not None else row["percentile"]
    return f"[{_pct(lo)}, {_pct(hi)}] ({'BCa' if row['bca'] is not None else 'percentile'})"


def main(args):
    _refusals(args)
    if args.before:
        dev, nc, before = hc.load_model(args.before, args.before_num_classes, args.task)
        models, folders = [before, hc.load_model(args.after, args.after_num_classes, args.task)[2]], []
    else:
        dev, nc, models, folders = ls.load_predictors(args)
        folders += [args.pred_b] if args.pred_b else []
    paired = len(models) + len(folders) == 2
    meter = SignificanceMeter(nc, nc - 1, paired=paired)
    data = ls.open_data(args, nc)
    with hc.png_pool() as pool:
        for run in ls.label_runs(data, pool, dev, args.batch_size, models, args.task, folders):
            meter.add(*run.sources, target=run.target, stems=run.stems)
    report = {"dataset": "synthetic" if args.synthetic else args.dataset, "task": args.task}
    report.update(meter.report(replicates=args.replicates, seed=args.seed, level=args.level,
                               influence=args.influence))
    names = ("A", "B") if paired else ("",)
    print(f"{report['dataset']} (task {args.task}) at the labels' own size: {report['images']} images, "
          f"{report['replicates']} replicates, level {report['level']}")
    for name, row in zip(names, report["predictors"]):
        m = row["mIoU"]
        print(f"mIoU {name + ' ' if name else ''}{_pct(m['value'])} %  se {_pct(m['se'])}  {_interval(m)}")
    if paired:
        d = report["delta"]
        print(f"B - A {_pct(d['value'])} points  se {_pct(d['se'])}  {_interval(d)}  p (paired bootstrap) "
              f"{d['p_boot']:.4f}  p (label swap) {d['p_swap']:.4f}")
    if args.json:
        hc.write_json(report, args.json)
    return report


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused."""
    pair = bool(args.before or args.after or args.before_num_classes or args.after_num_classes)
    given = [name for name, on in (("--state", bool(args.state)), ("--before / --after", pair),
                                   ("--pred", bool(args.pred))) if on]
    if len(given) != 1:
        raise RuntimeError("give one source: --state CHECKPOINT, --before CHECKPOINT --after CHECKPOINT or --pred DIR "
                           f"(got {', '.join(given) or 'none'})")
    if args.task is None:
        raise RuntimeError("--task is needed: which task's decoder and labels are scored")
    if pair:
        if not (args.before and args.after and args.before_num_classes and args.after_num_classes):
            raise RuntimeError("a pair needs --before, --before-num-classes, --after and --after-num-classes")
        if args.num_classes:
            raise RuntimeError("--num-classes goes with --state or --pred; a pair takes --before-num-classes and "
                               "--after-num-classes")
        rc.refuse_pair(args)
    else:
        if not args.num_classes:
            raise RuntimeError(f"{given[0]} needs --num-classes")
        rc.refuse_task(args.task, args.num_classes)
    if args.pred_b and not args.pred:
        raise RuntimeError("--pred-b is the second folder of a pair: it needs --pred")
    if args.pred_b and os.path.realpath(args.pred_b) == os.path.realpath(args.pred):
        raise RuntimeError("--pred-b is --pred: a folder compared with itself has no difference to test")
    check_settings(args.replicates, args.seed, args.level, args.influence, flags=True)
    rc.refuse_data(args)
    if min(args.native_height, args.native_width) < 1:
        raise RuntimeError("--native-height and --native-width must be positive")


def build_parser():
    p = hc.RefusingParser(_refusals, description="bootstrap intervals and paired tests for the mIoU at the dataset's "
                                                 "own size")
    p.add_argument("--state", help="one checkpoint written by the trainers (or by the reference)")
    p.add_argument("--num-classes", type=int, nargs="+", help="with --state or --pred")
    p.add_argument("--before", help="pair: the checkpoint before the incremental step (predictor A)")
    p.add_argument("--before-num-classes", type=int, nargs="+")
    p.add_argument("--after", help="pair: the checkpoint after it (predictor B)")
    p.add_argument("--after-num-classes", type=int, nargs="+")
    p.add_argument("--pred", help="score the <stem>_label.png files (train ids) of this folder (predictor A)")
    p.add_argument("--pred-b", help="pair: a second folder of such files (predictor B)")
    p.add_argument("--task", type=int, help="which task's decoder predicts; both models of a pair have it")
    p.add_argument("--replicates", type=int, default=10000, help="bootstrap and label-swap replicates "
                                                                 "(default %(default)s)")
    p.add_argument("--seed", type=int, default=0, help="of the counter-based generator (default %(default)s)")
    p.add_argument("--level", type=float, default=0.95, help="of the intervals (default %(default)s)")
    p.add_argument("--influence", type=int, default=10, help="how many of the most influential images to list "
                                                             "(default %(default)s)")
    p.add_argument("--json", help="write the report here")
    p.add_argument("--native-height", type=int, default=1024, help="--synthetic: the labels' own height")
    p.add_argument("--native-width", type=int, default=2048, help="--synthetic: the labels' own width")
    rc.add_data_flags(p)
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
