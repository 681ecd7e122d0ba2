"""Calibration report on MI355X: can a head's confidence be trusted, and which softmax temperature
makes it so.  ``output_conv``, the softmax at up to 16 temperatures at once, and per temperature
the top-class confidence, NLL, Brier score, entropy and the reliability histogram come from one
fused kernel straight from the decoder's 16-channel features, so the logit tensor is never stored
(include/mdil_calib.h).  The histogram is integer (counts, correct counts and confidences quantised
to 2^-24), so ECE is computed on the host from exact, order-independent numbers.

    python -m mdil_ss_amd.calibrate --state CKPT --num-classes 20 20 --task 0 \
        (--dataset cityscapes|BDD|IDD [--subset val] | --synthetic N) [--bins 15] \
        [--temperature T ... | --fit [--fit-rounds 4]] [--feature-cache-gb 16] --json FILE [--out DIR] \
        [--height 512 --width 1024 --batch-size 6]

The network runs once per image; its features (about 8 MB per 1024 x 512 image) and the u8 targets
stay on the device up to ``--feature-cache-gb``, so a temperature fit is a few sweeps of the head
kernel over them.  Beyond that budget the forward is run again per sweep; the JSON says which
happened.  ``--out`` writes ``reliability.png``: per bin the gap between accuracy and confidence,
at T = 1 and at the fitted (or first given) temperature."""
import ctypes as C
import functools
import math
import os

import torch

from . import _calib_lib
from . import _head_common as hc
from . import _report_common as rc

_FN, _PATH = "calib_head", "calibration"
_chk = functools.partial(hc.chk, _FN, _PATH)
_COUNTERS = ("hist", "class_hist", "sums", "nonfinite", "bad_targets", "workspace")
Q_ONE = 1 << 24                              # the confidence 1.0 in the histogram's integer sums


def workspace_bytes(N, H, W, nc, K):
    """Bytes of workspace ``calib_head`` needs to fill ``sums`` for features [N,H,W,16] and K temperatures."""
    n = _calib_lib.load().mdil_calib_workspace_bytes(int(N), int(H), int(W), int(nc), int(K))
    if n < 0:
        raise RuntimeError(f"mdil {_FN}: no workspace size for N {N}, H {H}, W {W}, {nc} classes, {K} temperatures")
    return n


def _temperatures(temps):
    try:
        temps = [float(t) for t in temps]
    except (TypeError, ValueError):
        raise RuntimeError(f"mdil {_FN}: temps must be a sequence of numbers, got {temps!r}") from None
    if not 1 <= len(temps) <= _calib_lib.MAX_TEMPS:
        raise RuntimeError(f"mdil {_FN}: {len(temps)} temperatures (supported: 1 to {_calib_lib.MAX_TEMPS})")
    if not all(math.isfinite(t) and t > 0 for t in temps):
        raise RuntimeError(f"mdil {_FN}: every temperature must be finite and > 0 (got {temps})")
    return temps


def calib_head(feat, w, b, target, temps, *, bins=15, ignore_index=-1, class_temp=None, label=False, maps=False,
               counters=None):
    """The head at ``temps`` (1 to 16 temperatures, host numbers) on NHWC decoder features
    [N,H,W,16] and their ``ConvTranspose2d(16, nc, 2, 2)`` parameters, 2 <= nc <= 32, against
    ``target`` (u8 [N,2H,2W], device, train ids), on the current stream.  A pixel is counted when its
    target is < nc and is not ``ignore_index``.  -> dict with ``label`` (u8 [N,2H,2W], with ``label``),
    ``conf`` and ``nll`` (f32 [K,N,2H,2W], with ``maps``); what was not asked for is None.

    ``counters``: a dict of device tensors that are ADDED to, never cleared, any of ``hist`` (i64
    [K,bins,3]: pixels, correct pixels, sum of ``int(conf * 2^24)`` per confidence bin),
    ``class_hist`` (i64 [nc,bins,3], the same at temperature index ``class_temp``, row = predicted
    class), ``nonfinite`` (i64 [K]), ``bad_targets`` (i64 [1]) and ``sums`` (f64 [K,3]: NLL, Brier,
    entropy), the last with ``workspace`` (f64, at least ``workspace_bytes(N, H, W, nc, K)`` bytes)."""
    lib = _calib_lib.load()
    for t, name in ((feat, "feat"), (w, "w"), (b, "b")):
        _chk(t, name)
    nc = hc.check_params(_FN, w, b, feat)
    hc.check_classes(_FN, _calib_lib, nc, feat, w, b)
    dev = feat.device
    N, H, W = feat.shape[0], feat.shape[1], feat.shape[2]
    if target is None:
        raise RuntimeError(f"mdil {_FN}: a target (uint8 [N,2H,2W] on the device) is required")
    hc.check_tables(_FN, _PATH, dev, torch.uint8, ((target, "target", (N, 2 * H, 2 * W)),))
    hc.check_ignore_index(_FN, ignore_index)
    temps = _temperatures(temps)
    K, bins = len(temps), int(bins)
    if not 1 <= bins <= _calib_lib.MAX_BINS:
        raise RuntimeError(f"mdil {_FN}: {bins} bins (supported: 1 to {_calib_lib.MAX_BINS})")
    ct = -1 if class_temp is None else int(class_temp)
    if not -1 <= ct < K:
        raise RuntimeError(f"mdil {_FN}: class_temp {class_temp} is not an index into the {K} temperatures")
    c = rc.check_counters(_FN, counters, _COUNTERS)
    hc.check_tables(_FN, _PATH, dev, torch.int64,
                    ((c["hist"], "hist", (K, bins, 3)), (c["class_hist"], "class_hist", (nc, bins, 3)),
                     (c["nonfinite"], "nonfinite", (K,)), (c["bad_targets"], "bad_targets", (1,))))
    hc.check_tables(_FN, _PATH, dev, torch.float64, ((c["sums"], "sums", (K, 3)),))
    if c["class_hist"] is not None and ct < 0:
        raise RuntimeError(f"mdil {_FN}: class_hist needs class_temp, the index of the temperature it is taken at")
    ws, ws_bytes = rc.check_workspace(_FN, _PATH, dev, c, lambda: workspace_bytes(N, H, W, nc, K))
    host_temps = (C.c_float * K)(*temps)
    with torch.no_grad(), torch.cuda.device(dev):
        out = {"label": torch.empty(N, 2 * H, 2 * W, dtype=torch.uint8, device=dev) if label else None,
               "conf": torch.empty(K, N, 2 * H, 2 * W, dtype=torch.float32, device=dev) if maps else None,
               "nll": torch.empty(K, N, 2 * H, 2 * W, dtype=torch.float32, device=dev) if maps else None}
        _calib_lib.check(
            lib.mdil_calib_head(feat.data_ptr(), w.data_ptr(), b.data_ptr(), N, H, W, nc, target.data_ptr(),
                                int(ignore_index), host_temps, K, bins, ct, hc.ptr(out["label"]), hc.ptr(out["conf"]),
                                hc.ptr(out["nll"]), hc.ptr(c["hist"]), hc.ptr(c["class_hist"]), hc.ptr(c["sums"]),
                                hc.ptr(c["nonfinite"]), hc.ptr(c["bad_targets"]), ws, ws_bytes,
                                torch.cuda.current_stream(dev).cuda_stream),
            "mdil_calib_head")
    return out


def calibrate(model, images, task, target, temps, **kw):
    """``calib_head`` on ``images`` [N,3,H,W] for ``task``: the decoder features and that task's
    ``output_conv`` parameters of ``model`` in eval mode."""
    if not isinstance(images, torch.Tensor) or not images.is_cuda:
        raise RuntimeError("mdil calibrate: images must be a device tensor; there is no CPU fallback in the "
                           "calibration path")
    model.eval()
    with torch.no_grad():
        feat = model.features(images, task)
        w, b = model.head_params(task)
        return calib_head(feat.contiguous(), w.detach(), b.detach(), target, temps, **kw)


class CalibrationMeter:
    """Owns the histograms, the sums and the workspace of a calibration run over many batches at a
    fixed list of temperatures."""

    def __init__(self, nc, temps, bins=15, ignore_index=-1, class_temp=None):
        self.nc, self.temps, self.bins = int(nc), _temperatures(temps), int(bins)
        self.ignore_index, self.class_temp = int(ignore_index), class_temp
        self.tensors = None

    def _counters(self, dev, N, H, W):
        K = len(self.temps)
        if self.tensors is None:
            z = functools.partial(torch.zeros, dtype=torch.int64, device=dev)
            self.tensors = {"hist": z(K, self.bins, 3), "nonfinite": z(K), "bad_targets": z(1),
                            "sums": torch.zeros(K, 3, dtype=torch.float64, device=dev)}
            if self.class_temp is not None:
                self.tensors["class_hist"] = z(self.nc, self.bins, 3)
        rc.grow_workspace(self.tensors, workspace_bytes(N, H, W, self.nc, K), dev)
        return self.tensors

    def add(self, *source, target=None, **kw):
        """``add(model, images, task, target=t)`` or ``add(feat, w, b, target=t)``, ``t`` u8 [N,2H,2W]
        train ids on the device.  -> ``calib_head``'s dict."""
        fn, dev, N, H, W = rc.meter_source("CalibrationMeter", _PATH, source, 1, calibrate, calib_head, "feat")
        if target is None:
            raise RuntimeError("mdil CalibrationMeter.add: a target is required")
        return fn(*source, target, self.temps, bins=self.bins, ignore_index=self.ignore_index,
                  class_temp=self.class_temp, counters=self._counters(dev, N, H, W), **kw)

    def host(self):
        """The counters on the host (int64 histograms, float64 sums); raises when a target outside
        [0, nc) other than the ignore index was met, or a counted pixel had a non-finite NLL."""
        K = len(self.temps)
        if self.tensors is None:
            out = {"hist": torch.zeros(K, self.bins, 3, dtype=torch.int64), "sums": torch.zeros(K, 3, dtype=torch.float64)}
            if self.class_temp is not None:
                out["class_hist"] = torch.zeros(self.nc, self.bins, 3, dtype=torch.int64)
            return out
        rc.refuse_bad_targets("CalibrationMeter", self.tensors, self.nc, self.ignore_index)
        nonfinite = self.tensors["nonfinite"].cpu().tolist()
        if any(nonfinite):
            raise RuntimeError(f"mdil CalibrationMeter: counted pixels with a non-finite NLL per temperature: "
                               f"{nonfinite} (NaN or inf logits)")
        return {k: v.cpu() for k, v in self.tensors.items() if k in ("hist", "class_hist", "sums")}

    def report(self, names=None):
        return calibration_report(temps=self.temps, names=names, **self.host())


# ------------------------------------------------------------------------------- host arithmetic
def _bins_report(cells):
    """``cells``: [bins][3] Python ints -> (pixels, correct, ece, mce, table)."""
    n = sum(c[0] for c in cells)
    correct = sum(c[1] for c in cells)
    gaps = [abs(c[1] * Q_ONE - c[2]) for c in cells]                       # exact integers
    ece = sum(gaps) / (Q_ONE * n) if n else None
    mce = max((g / (Q_ONE * c[0]) for g, c in zip(gaps, cells) if c[0]), default=None)
    table = [{"pixels": c[0], "accuracy": c[1] / c[0] if c[0] else None,
              "confidence": c[2] / (Q_ONE * c[0]) if c[0] else None} for c in cells]
    return n, correct, ece, mce, table


def calibration_report(hist, sums, temps, class_hist=None, names=None):
    """From the integer histograms and the sums to the report; runs on the host alone, in fp64.

    ``hist`` i64 [K,bins,3] (pixels, correct pixels, sum of ``int(conf * 2^24)`` per bin), ``sums`` f64
    [K,3] (NLL, Brier, entropy), ``temps`` the K temperatures.  -> dict: ``bins`` and per
    temperature (``temperatures``) ``pixels``, ``accuracy``, ``ece`` = sum_b |correct_b - confsum_b| / n,
    ``mce`` the largest |correct_b - confsum_b| / n_b over the non-empty bins, ``nll``, ``brier``,
    ``entropy`` (means) and the ``reliability`` table (per bin: pixels, accuracy, mean confidence;
    None in an empty bin).  With ``class_hist`` (i64 [nc,bins,3], row = predicted class) also
    ``class_ece`` (None for a class that was never predicted), their mean ``classwise_ece`` and,
    with ``names``, ``class_names``."""
    h = torch.as_tensor(hist, dtype=torch.int64)
    s = torch.as_tensor(sums, dtype=torch.float64)
    temps = [float(t) for t in temps]
    K = len(temps)
    if h.dim() != 3 or h.shape[0] != K or h.shape[2] != 3 or tuple(s.shape) != (K, 3):
        raise RuntimeError(f"mdil calibration_report: expected hist [{K},bins,3] and sums [{K},3] "
                           f"(got {tuple(h.shape)} and {tuple(s.shape)})")
    rows = []
    for k, cells in enumerate(h.tolist()):
        n, correct, ece, mce, table = _bins_report(cells)
        mean = [float(v) / n if n else None for v in s[k].tolist()]
        rows.append({"temperature": temps[k], "pixels": n, "accuracy": correct / n if n else None, "ece": ece,
                     "mce": mce, "nll": mean[0], "brier": mean[1], "entropy": mean[2], "reliability": table})
    report = {"bins": int(h.shape[1]), "temperatures": rows}
    if class_hist is not None:
        ch = torch.as_tensor(class_hist, dtype=torch.int64)
        if ch.dim() != 3 or tuple(ch.shape[1:]) != (h.shape[1], 3):
            raise RuntimeError(f"mdil calibration_report: expected class_hist [nc,{h.shape[1]},3] (got {tuple(ch.shape)})")
        per_class = [_bins_report(cells)[2] for cells in ch.tolist()]
        seen = [v for v in per_class if v is not None]
        report.update(class_ece=per_class, classwise_ece=sum(seen) / len(seen) if seen else None)
        if names is not None:
            report["class_names"] = list(names)
    return report


def fit_temperature(nll_of, lo=0.25, hi=4.0, points=16, rounds=4):
    """The temperature that minimises the NLL; runs on the host alone.  ``nll_of(temps)`` -> the NLL
    sums (or means) at ``len(temps)`` temperatures.

    Each round evaluates a geometric grid of ``points`` temperatures on [lo, hi], takes the argmin
    and narrows to its two neighbours; at an end point the range is lengthened by one cell on that
    side instead (the minimum may lie outside), so [lo, hi] is a bracket once a round has found its
    argmin inside.  The NLL is convex in 1/T, so from then on it holds the minimiser, and hi/lo shrinks as
    r -> r^(2 / (points - 1)) per round: 16 -> 1.447 -> 1.0505 -> 1.0066 -> 1.0009.  -> dict:
    ``temperature`` (the last round's argmin), ``bracket`` [lo, hi] around it, ``cell`` (the ratio of
    neighbouring temperatures in the last grid) and ``trace``, every [T, NLL] evaluated."""
    lo, hi, points, rounds = float(lo), float(hi), int(points), int(rounds)
    if not (0 < lo < hi and math.isfinite(hi)) or points < 3 or rounds < 1:
        raise RuntimeError(f"mdil fit_temperature: needs 0 < lo < hi, at least 3 points and 1 round "
                           f"(got lo {lo}, hi {hi}, {points} points, {rounds} rounds)")
    trace, best, cell = [], None, None
    for _ in range(rounds):
        cell = (hi / lo) ** (1.0 / (points - 1))
        grid = [lo * cell ** i for i in range(points)]
        grid[-1] = hi
        values = [float(v) for v in nll_of(grid)]
        if len(values) != points or not all(math.isfinite(v) for v in values):
            raise RuntimeError(f"mdil fit_temperature: nll_of returned {values} for {points} temperatures")
        trace += [[t, v] for t, v in zip(grid, values)]
        i = min(range(points), key=lambda j: (values[j], j))
        best = grid[i]
        if i == 0:
            lo = lo / cell
        elif i == points - 1:
            hi = hi * cell
        else:
            lo, hi = grid[i - 1], grid[i + 1]
    return {"temperature": best, "bracket": [lo, hi], "cell": cell, "trace": trace}


# ------------------------------------------------------------------------------------------ CLI
def reliability_image(before, after, size=(640, 360)):
    """The gap bars of two reliability tables (``calibration_report``'s rows) side by side -> PIL image.
    Per bin: the accuracy as a grey bar and the gap to the mean confidence on top of it, red where
    the model is over-confident and blue where it is under-confident; the diagonal is perfect calibration."""
    from PIL import Image, ImageDraw
    Wd, Ht = size
    im = Image.new("RGB", size, (255, 255, 255))
    draw = ImageDraw.Draw(im)
    margin, gap = 24, 24
    side = min((Wd - 2 * margin - gap) // 2, Ht - 2 * margin - 16)
    for j, row in enumerate((before, after)):
        x0, y0 = margin + j * (side + gap), margin + 16
        table = row["reliability"]
        n = len(table)
        draw.rectangle([x0, y0, x0 + side, y0 + side], outline=(0, 0, 0))
        draw.line([x0, y0 + side, x0 + side, y0], fill=(150, 150, 150))
        draw.text((x0, margin - 8), f"T = {row['temperature']:.4g}   ECE {row['ece']:.4f}", fill=(0, 0, 0))
        for i, cell in enumerate(table):
            if not cell["pixels"]:
                continue
            xa, xb = x0 + side * i // n + 1, x0 + side * (i + 1) // n - 1
            ya, yc = y0 + side - round(side * cell["accuracy"]), y0 + side - round(side * cell["confidence"])
            draw.rectangle([xa, ya, xb, y0 + side], fill=(110, 110, 110))
            if yc != ya:
                draw.rectangle([xa, min(ya, yc), xb, max(ya, yc)],
                               fill=(220, 50, 47) if cell["confidence"] > cell["accuracy"] else (38, 110, 200))
    return im


class _Features:
    """The validation set as (features, target) batches on the device: kept up to ``budget`` bytes,
    beyond it the forward is run again on every sweep."""

    def __init__(self, args, nc, dev, model, budget):
        self.args, self.nc, self.dev, self.model, self.budget = args, nc, dev, model, budget
        self.w, self.b = (t.detach() for t in model.head_params(args.task))
        self.kept, self.bytes, self.images, self.sweeps = None, 0, 0, 0

    def __iter__(self):
        self.sweeps += 1
        if self.kept is not None:
            yield from self.kept
            return
        kept, size, images = [], 0, 0
        with torch.no_grad():
            for _, batch, target in rc.batches(self.args, self.nc, self.dev):
                feat = self.model.features(batch, self.args.task).contiguous()
                images += batch.shape[0]
                if kept is not None:
                    size += feat.numel() * 4 + target.numel()
                    if size <= self.budget:
                        kept.append((feat, target))
                    else:
                        kept, size = None, 0
                yield feat, target
        self.images = images
        if kept is not None:
            self.kept, self.bytes = kept, size

    def meter(self, temps, bins, class_temp=None):
        meter = CalibrationMeter(self.nc, temps, bins, self.nc - 1, class_temp)
        for feat, target in self:
            meter.add(feat, self.w, self.b, target=target)
        return meter


def main(args):
    _refusals(args)
    dev, nc, model = hc.load_model(args.state, args.num_classes, args.task)
    source = _Features(args, nc, dev, model, int(args.feature_cache_gb * 2 ** 30))
    base = source.meter([1.0], args.bins, 0).report()
    report = {"dataset": "synthetic" if args.synthetic else args.dataset, "task": args.task, "classes": nc,
              "bins": args.bins, "report_t1": base}
    fit = None
    if args.fit:
        def nll_of(temps):
            return source.meter(temps, args.bins).host()["sums"][:, 0].tolist()
        fit = fit_temperature(nll_of, rounds=args.fit_rounds)
        temps = [fit["temperature"]]
    else:
        temps = list(args.temperature or [])
    report["fit"] = fit
    scaled = source.meter(temps, args.bins, 0).report() if temps else None
    report["report_scaled"] = scaled
    report["images"] = source.images
    report["cache"] = {"mode": "features" if source.kept is not None else "recompute", "bytes": source.bytes,
                       "budget_bytes": source.budget, "sweeps": source.sweeps}
    t1 = base["temperatures"][0]
    print(f"{report['dataset']} (task {args.task}) at T = 1: accuracy {t1['accuracy'] * 100:.2f} %  ECE {t1['ece']:.5f}  "
          f"MCE {t1['mce']:.5f}  NLL {t1['nll']:.6f}  Brier {t1['brier']:.6f}  class-wise ECE "
          f"{base['classwise_ece']:.5f}  over {t1['pixels']} pixels")
    for row in scaled["temperatures"] if scaled else ():
        print(f"  at T = {row['temperature']:.5g}{' (fitted)' if fit else ''}: ECE {row['ece']:.5f}  MCE {row['mce']:.5f}  "
              f"NLL {row['nll']:.6f}  Brier {row['brier']:.6f}")
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        path = os.path.join(args.out, "reliability.png")
        reliability_image(t1, scaled["temperatures"][0] if scaled else t1).save(path)
        report["written"] = [path]
        print(f"reliability diagram written to {path}")
    hc.write_json(report, args.json)
    return report


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused."""
    rc.refuse_task(args.task, args.num_classes)
    rc.refuse_data(args)
    if not 1 <= args.bins <= _calib_lib.MAX_BINS:
        raise RuntimeError(f"--bins must lie in [1, {_calib_lib.MAX_BINS}]")
    if args.fit and args.temperature:
        raise RuntimeError("--fit and --temperature exclude each other")
    if args.temperature and len(args.temperature) > _calib_lib.MAX_TEMPS:
        raise RuntimeError(f"at most {_calib_lib.MAX_TEMPS} temperatures in one run")
    if args.temperature and not all(math.isfinite(t) and t > 0 for t in args.temperature):
        raise RuntimeError("every --temperature must be finite and > 0")
    if args.fit_rounds < 1:
        raise RuntimeError("--fit-rounds must be at least 1")
    if not args.feature_cache_gb >= 0:
        raise RuntimeError("--feature-cache-gb must not be negative")


def build_parser():
    p = hc.RefusingParser(_refusals, description="calibration report: ECE, reliability and the fitted temperature")
    p.add_argument("--state", required=True, help="checkpoint of the model")
    p.add_argument("--num-classes", type=int, nargs="+", required=True)
    p.add_argument("--task", type=int, required=True, help="which task's decoder is calibrated")
    p.add_argument("--bins", type=int, default=15, help="equal-width confidence bins")
    p.add_argument("--temperature", type=float, nargs="+", help="also report at these temperatures")
    p.add_argument("--fit", action="store_true", help="fit the temperature that minimises the NLL and report at it")
    p.add_argument("--fit-rounds", type=int, default=4, help="rounds of 16 temperatures; 4 bracket T* to 0.09 %%")
    p.add_argument("--feature-cache-gb", type=float, default=16.0,
                   help="features kept on the device between sweeps; beyond it the forward runs again per sweep")
    p.add_argument("--json", required=True, help="write the report here")
    p.add_argument("--out", help="write reliability.png into this folder")
    rc.add_data_flags(p)
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
