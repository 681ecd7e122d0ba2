"""Density report on MI355X: open-set scores in FEATURE space.  ``openset``'s four scores are functions
of the head's nc logits; what the 16 -> nc projection discards is invisible to them.  Here every
feature row is scored against class-conditional Gaussians with one tied covariance (Lee et al.,
NeurIPS 2018; Fishyscapes' "embedding density"), also in the relative form of Ren et al. (2021), and
the nearest class mean that comes out of the same distances is reported as a classifier (iCaRL).

    python -m mdil_ss_amd.density --fit MODEL.npz --state CKPT --num-classes 20 20 27 --task 0 --dataset cityscapes \
        --subset train --layer penultimate|encoder [--ridge R --min-rows M]
    python -m mdil_ss_amd.density --model MODEL.npz --state CKPT --num-classes 20 20 27 --task 0 --dataset IDD \
        --data-task 2 --unknown-ids 18 25 --score --json FILE [--with-logit-scores]
    python -m mdil_ss_amd.density --model MODEL.npz --state CKPT --num-classes 20 20 --task 0 --dataset cityscapes \
        --fit-threshold THR.json --known-fpr 0.05
    python -m mdil_ss_amd.density --model MODEL.npz --state CKPT --num-classes 20 20 --task 0 --images DIR \
        --threshold THR.json --kind maha|rmaha --out DIR2 [--unknown-id 255 --colour --nearest]

The fit is host algebra in fp64 on the moments that ``similarity.MomentMeter`` accumulates (class
counts, class sums, the Gram matrix).  The scores are one fused kernel (include/mdil_density.h):
``density_head`` for the penultimate layer, fused with ``output_conv`` + argmax, ``density_rows`` for
any layer of up to 128 channels.  Everything after the 16-bit code is ``openset``'s: ``metrics``,
``threshold_at_known_fpr``, ``cdf_lut`` and ``openset_apply`` read these histograms and maps unchanged.

``ridge`` (default 1e-4 of the mean variance) is UNTUNED.  The penultimate features are post-ReLU and
far from Gaussian; a channel can be constant over a whole split, and only the ridge keeps the
factorisation defined there."""
import os
from argparse import Namespace

import numpy as np
import torch

from . import _density_lib
from . import _head_common as hc
from . import _report_common as rc
from . import openset as OS

_PATH = "density"
KINDS = ("maha", "rmaha")
CODES = OS.CODES
NONFINITE_CODE = OS.NONFINITE_CODE
NO_CLASS = 255
CODE = OS.CODE
KNOWN, UNKNOWN, IGNORED = OS.KNOWN, OS.UNKNOWN, OS.IGNORED
DEFAULT_RIDGE = 1e-4
FIT_LAYERS = ("penultimate", "encoder")
MODEL_FORMAT = 1
_ARRAYS = ("pivot", "cls", "dropped", "counts", "means", "mean_total", "cov_within", "cov_total", "buffer")
_SETTINGS = ("format", "layer", "task", "C", "nc", "ridge", "min_rows", "rows")


def model_floats(C, K):
    """MDIL_DENSITY_MODEL_FLOATS: pivot [C] | A [C][C] | A0 [C][C] | m0 [C] | m [K][C]."""
    return 2 * C + 2 * C * C + K * C


def kinds_mask(kinds):
    """Kind names or numbers -> the bit mask of the kernels (1..3)."""
    mask = 0
    for k in kinds:
        if isinstance(k, str) and k in KINDS:
            k = KINDS.index(k)
        if not isinstance(k, int) or not 0 <= k < len(KINDS):
            raise RuntimeError(f"mdil density: unknown score kind {k!r} (known: {list(KINDS)})")
        mask |= 1 << k
    if not mask:
        raise RuntimeError(f"mdil density: no score kind given (known: {list(KINDS)})")
    return mask


# ------------------------------------------------------------------------------------- the fit
def _inverse_factor(cov, what):
    """cov = L L^T (fp64) -> A = L^-1, lower triangular: A cov A^T = I."""
    try:
        L = np.linalg.cholesky(cov)
    except np.linalg.LinAlgError:
        raise RuntimeError(f"mdil fit_model: the {what} covariance is not positive definite (every channel constant, "
                           "or ridge 0 with a constant channel); give a larger ridge") from None
    A = torch.linalg.solve_triangular(torch.from_numpy(L), torch.eye(L.shape[0], dtype=torch.float64), upper=False)
    return np.tril(A.numpy())


def fit_model(moments, ridge=DEFAULT_RIDGE, min_rows=None, layer=None, task=None, nc=None):
    """The Gaussians of one population from ``similarity.MomentMeter(...).moments()`` (x alone, the
    meter's ``nc`` = the head's classes without the void class), in fp64 on the host:
        mu_k   = pivot + sx_k / n_k                       for every class with n_k >= ``min_rows`` (default 2 C);
                                                          the others leave ``cls`` and are named in ``dropped``
        S_w    = G - sum_k n_k mu'_k mu'_k^T              over EVERY class with rows (mu' = sx_k / n_k, pivoted)
        tied   = S_w / (n - K') + ridge tr(S_w / (n - K')) / C I       K' classes with rows, n rows
        total  = (G - n mu' mu'^T) / (n - 1) + ridge tr(.) / C I       the background Gaussian
        A      = chol(tied)^-1,  m_k = A (mu_k - pivot);  A0, m0 likewise from ``total``
    then rounded to the fp32 ``buffer`` the kernels read.  -> a dict of host arrays and settings."""
    if moments.get("cy"):
        raise RuntimeError("mdil fit_model: expects the moments of one population (cy 0)")
    C = int(moments["cx"])
    if C % 16 or not 16 <= C <= _density_lib.MAX_CHANNELS:
        raise RuntimeError(f"mdil fit_model: {C} channels (supported: multiples of 16 up to {_density_lib.MAX_CHANNELS})")
    ridge = float(ridge)
    if not np.isfinite(ridge) or ridge < 0:
        raise RuntimeError(f"mdil fit_model: ridge {ridge} must be a finite number >= 0")
    min_rows = 2 * C if min_rows is None else int(min_rows)
    if min_rows < 1:
        raise RuntimeError(f"mdil fit_model: min_rows {min_rows} must be at least 1")
    n = np.asarray(moments["n"], dtype=np.float64)
    sx = np.asarray(moments["sx"], dtype=np.float64)
    G = np.asarray(moments["gxx"], dtype=np.float64)
    pivot = np.asarray(moments["pivot_x"], dtype=np.float64).reshape(C)
    if len(n) > _density_lib.MAX_CLASSES:
        raise RuntimeError(f"mdil fit_model: {len(n)} classes (at most {_density_lib.MAX_CLASSES})")
    have = n > 0
    rows, present = float(n.sum()), int(have.sum())
    if rows - present < 1:
        raise RuntimeError(f"mdil fit_model: {int(rows)} rows in {present} classes leave no degree of freedom")
    mu = np.zeros_like(sx)
    mu[have] = sx[have] / n[have, None]                              # pivoted class means
    keep = [k for k in range(len(n)) if n[k] >= min_rows]
    dropped = [k for k in range(len(n)) if k not in keep]
    if not keep:
        raise RuntimeError(f"mdil fit_model: no class has min_rows = {min_rows} rows (rows per class: "
                           f"{[int(v) for v in n]})")
    if len(keep) > _density_lib.MAX_MEANS:
        raise RuntimeError(f"mdil fit_model: {len(keep)} class means (at most {_density_lib.MAX_MEANS})")
    S_w = G - (n[have, None, None] * mu[have, :, None] * mu[have, None, :]).sum(0)
    S_w = (S_w + S_w.T) / 2
    within = S_w / (rows - present)
    within = within + ridge * np.trace(within) / C * np.eye(C)
    mt = sx.sum(0) / rows                                          # pivoted mean of all rows
    S_t = G - rows * np.outer(mt, mt)
    S_t = (S_t + S_t.T) / 2
    total = S_t / (rows - 1)
    total = total + ridge * np.trace(total) / C * np.eye(C)
    A, A0 = _inverse_factor(within, "tied"), _inverse_factor(total, "total")
    m = mu[keep] @ A.T
    m0 = A0 @ mt
    buffer = np.concatenate([pivot, A.reshape(-1), A0.reshape(-1), m0, m.reshape(-1)]).astype(np.float32)
    if not np.isfinite(buffer).all():
        raise RuntimeError("mdil fit_model: the fp32 model is not finite; give a larger ridge")
    return {"format": MODEL_FORMAT, "layer": "" if layer is None else str(layer), "task": -1 if task is None else int(task),
            "C": C, "nc": len(n) + 1 if nc is None else int(nc), "ridge": ridge, "min_rows": min_rows, "rows": int(rows),
            "pivot": pivot, "cls": np.asarray(keep, dtype=np.uint8), "dropped": np.asarray(dropped, dtype=np.int64),
            "counts": n.astype(np.int64), "means": pivot + mu[keep], "mean_total": pivot + mt, "cov_within": within,
            "cov_total": total, "buffer": buffer}


def save_model(model, path):
    """One ``.npz`` of arrays and settings only (no pickled objects)."""
    arrays = {k: np.asarray(model[k]) for k in _ARRAYS + _SETTINGS}
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def load_model(path, layer=None, nc=None, C=None, task=None):
    """-> the model dict of ``save_model``; refuses a model whose layer, task width ``nc``, task or channel
    count ``C`` (each checked when given) does not fit the run."""
    if not os.path.isfile(path):
        raise RuntimeError(f"--model {path}: no such file")
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in _ARRAYS + _SETTINGS if k not in z.files]
        if missing:
            raise RuntimeError(f"--model {path}: not a density model (missing {missing})")
        model = {k: z[k] for k in _ARRAYS}
        model.update({k: z[k].item() for k in _SETTINGS})
    if model["format"] != MODEL_FORMAT:
        raise RuntimeError(f"--model {path}: format {model['format']}, this build reads format {MODEL_FORMAT}")
    K = len(model["cls"])
    if model["buffer"].dtype != np.float32 or model["buffer"].size != model_floats(model["C"], K):
        raise RuntimeError(f"--model {path}: the fp32 buffer does not fit C {model['C']} and {K} class means")
    for name, want, got in (("layer", layer, model["layer"]), ("num-classes of the task", nc, model["nc"]),
                            ("channels", C, model["C"]), ("task", task, model["task"])):
        if want is not None and want != got:
            raise RuntimeError(f"--model {path}: fitted for {name} {got}, this run has {want}")
    return model


class DeviceModel:
    """A fitted model on the device: ``buffer`` f32 and ``cls`` u8 as the kernels read them."""

    def __init__(self, model, device):
        self.C, self.K = int(model["C"]), len(model["cls"])
        buf = torch.as_tensor(np.asarray(model["buffer"], dtype=np.float32))
        if buf.numel() != model_floats(self.C, self.K) or not 1 <= self.K <= _density_lib.MAX_MEANS:
            raise RuntimeError(f"mdil density: a model of {buf.numel()} floats does not fit C {self.C} and {self.K} means")
        self.buffer = buf.contiguous().to(device)
        self.cls = torch.as_tensor(np.asarray(model["cls"], dtype=np.uint8)).contiguous().to(device)
        self.device = self.buffer.device


def _device_model(fn, model, dev, C):
    if not isinstance(model, DeviceModel):
        model = DeviceModel(model, dev)
    if model.device != dev or model.C != C:
        raise RuntimeError(f"mdil {fn}: the model is for {model.C} channels on {model.device}, the features have {C} on {dev}")
    return model


def _common(fn, const_group, kinds, map_kind):
    mask = kinds_mask(kinds)
    if map_kind is not None:
        map_kind = kinds_mask([map_kind]).bit_length() - 1
    if int(const_group) not in (KNOWN, UNKNOWN, IGNORED):
        raise RuntimeError(f"mdil {fn}: const_group {const_group} outside [0, 2]")
    return mask, map_kind


# --------------------------------------------------------------------------------- entry points
def density_head(features, weight, bias, model, target=None, lut=None, const_group=KNOWN, kinds=KINDS, map_kind=None,
                 hist=None, nonfinite=None, agree=None, want_label=True, want_nearest=False):
    """``output_conv`` + argmax + both density scores on NHWC decoder features [N,H,W,16], on the
    current stream.  ``model``: a fitted model (dict or ``DeviceModel``) for 16 channels.
    -> (label u8 [N,2H,2W] or None, nearest u8 [N,2H,2W] or None, code u16 [N,2H,2W] of ``map_kind`` or
    None).  ``hist`` (int64 [2,2,65536], device) gains one count per kind of ``kinds`` and OUTPUT pixel
    at [kind][group][code], the group being ``lut[target]`` or ``const_group``; ``nonfinite`` (int64 [1])
    four per feature pixel that is not finite; ``agree`` (int64 [2]) the pixels of group 0 and those of
    them whose nearest class mean is the head's label.  All three are accumulated into."""
    fn = "density_head"
    lib = _density_lib.load()
    for t, name in ((features, "features"), (weight, "weight"), (bias, "bias")):
        hc.chk(fn, _PATH, t, name)
    x, w, b = features, weight, bias
    nc = hc.check_params(fn, w, b, x)
    N, H, W = x.shape[0], x.shape[1], x.shape[2]
    hc.check_classes(fn, _density_lib, nc, x, w, b)
    mask, map_kind = _common(fn, const_group, kinds, map_kind)
    dm = _device_model(fn, model, x.device, 16)
    if target is not None and lut is None:
        raise RuntimeError(f"mdil {fn}: a target needs its group look-up table (uint8 [256]) on the device")
    hc.check_tables(fn, _PATH, x.device, torch.uint8, ((target, "target", (N, 2 * H, 2 * W)), (lut, "lut", (256,))))
    hc.check_tables(fn, _PATH, x.device, torch.int64, ((hist, "hist", (len(KINDS), 2, CODES)),
                                                       (nonfinite, "nonfinite", (1,)), (agree, "agree", (2,))))
    if not want_label and not want_nearest and map_kind is None and hist is None and nonfinite is None and agree is None:
        raise RuntimeError(f"mdil {fn}: nothing to do (no label, no nearest, no code map, no counters)")
    with torch.no_grad(), torch.cuda.device(x.device):
        size = (N, 2 * H, 2 * W)
        label = torch.empty(size, dtype=torch.uint8, device=x.device) if want_label else None
        nearest = torch.empty(size, dtype=torch.uint8, device=x.device) if want_nearest else None
        code = torch.empty(size, dtype=CODE, device=x.device) if map_kind is not None else None
        _density_lib.check(
            lib.mdil_density_head(x.data_ptr(), w.data_ptr(), b.data_ptr(), N, H, W, nc, dm.buffer.data_ptr(),
                                  dm.cls.data_ptr(), dm.K, hc.ptr(target), hc.ptr(lut if target is not None else None),
                                  int(const_group), mask, -1 if map_kind is None else map_kind, hc.ptr(label),
                                  hc.ptr(nearest), hc.ptr(code), hc.ptr(hist), hc.ptr(nonfinite), hc.ptr(agree),
                                  torch.cuda.current_stream(x.device).cuda_stream),
            "mdil_density_head")
    return label, nearest, code


def density_rows(x, model, group=None, const_group=KNOWN, kinds=KINDS, map_kind=None, hist=None, nonfinite=None,
                 want_nearest=True):
    """Both scores of feature rows ``x`` f32 [..., C] (contiguous, C a multiple of 16 up to 128, at most
    2^24 rows), on the current stream.  ``group``: u8, one entry per row (0 known, 1 unknown, else
    ignored), or None with ``const_group``.  -> (nearest u8 [rows] or None, code u16 [rows] of
    ``map_kind`` or None); ``hist`` and ``nonfinite`` as in ``density_head``, one count per row."""
    fn = "density_rows"
    lib = _density_lib.load()
    hc.chk(fn, _PATH, x, "x")
    C = x.shape[-1] if x.dim() >= 2 else 0
    if C % 16 or not 16 <= C <= _density_lib.MAX_CHANNELS or x.numel() == 0:
        raise RuntimeError(f"mdil {fn}: x must be float32 [rows,C], C a multiple of 16 in [16, "
                           f"{_density_lib.MAX_CHANNELS}] (got {tuple(x.shape)})")
    rows = x.numel() // C
    if rows > _density_lib.MAX_ROWS:
        raise RuntimeError(f"mdil {fn}: {rows} rows (at most {_density_lib.MAX_ROWS} per call)")
    mask, map_kind = _common(fn, const_group, kinds, map_kind)
    dm = _device_model(fn, model, x.device, C)
    if group is not None:
        hc.chk(fn, _PATH, group, "group", torch.uint8)
        if group.numel() != rows or group.device != x.device:
            raise RuntimeError(f"mdil {fn}: group must be uint8 [{rows}] on {x.device} (got {tuple(group.shape)} on "
                               f"{group.device})")
    hc.check_tables(fn, _PATH, x.device, torch.int64, ((hist, "hist", (len(KINDS), 2, CODES)),
                                                       (nonfinite, "nonfinite", (1,))))
    if not want_nearest and map_kind is None and hist is None and nonfinite is None:
        raise RuntimeError(f"mdil {fn}: nothing to do (no nearest, no code map, no hist, no nonfinite)")
    with torch.no_grad(), torch.cuda.device(x.device):
        nearest = torch.empty(rows, dtype=torch.uint8, device=x.device) if want_nearest else None
        code = torch.empty(rows, dtype=CODE, device=x.device) if map_kind is not None else None
        _density_lib.check(
            lib.mdil_density_rows(x.data_ptr(), rows, C, dm.buffer.data_ptr(), dm.cls.data_ptr(), dm.K, hc.ptr(group),
                                  int(const_group), mask, -1 if map_kind is None else map_kind, hc.ptr(nearest),
                                  hc.ptr(code), hc.ptr(hist), hc.ptr(nonfinite),
                                  torch.cuda.current_stream(x.device).cuda_stream),
            "mdil_density_rows")
    return nearest, code


class DensityMeter:
    """Accumulates ``hist``, ``nonfinite`` and ``agree`` over a split.  ``add`` runs the fused head on a
    batch (``layer`` "penultimate") or ``density_rows`` on the layer's own grid with the labels resized
    to it ("encoder"); ``report`` gives per-kind metrics through ``openset.metrics`` unchanged."""

    def __init__(self, nc, model, kinds=KINDS, lut=None, const_group=KNOWN, layer="penultimate"):
        self.nc = hc.check_nc("DensityMeter", _density_lib, nc)
        self.mask = kinds_mask(kinds)
        self.kinds = tuple(k for i, k in enumerate(KINDS) if self.mask >> i & 1)
        if lut is not None and (not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint8 or lut.numel() != 256):
            raise RuntimeError("mdil DensityMeter: lut must be a uint8 [256] tensor (openset.group_lut)")
        if int(const_group) not in (KNOWN, UNKNOWN, IGNORED):
            raise RuntimeError(f"mdil DensityMeter: const_group {const_group} outside [0, 2]")
        if layer not in FIT_LAYERS:
            raise RuntimeError(f"mdil DensityMeter: layer must be one of {FIT_LAYERS}, got {layer!r}")
        self.model, self.layer = model, layer
        self.lut, self.const_group, self.tensors, self.pixels, self.grid = lut, int(const_group), {}, 0, None

    def _ready(self, dev):
        if not self.tensors:
            self.tensors = {"hist": torch.zeros(len(KINDS), 2, CODES, dtype=torch.int64, device=dev),
                            "nonfinite": torch.zeros(1, dtype=torch.int64, device=dev),
                            "agree": torch.zeros(2, dtype=torch.int64, device=dev)}
            if self.lut is not None:
                self.lut = self.lut.contiguous().to(dev)
            if not isinstance(self.model, DeviceModel):
                self.model = DeviceModel(self.model, dev)

    def _head(self, x, w, b, **kw):
        t = self.tensors
        return density_head(x, w, b, self.model, kinds=self.kinds, hist=t["hist"], nonfinite=t["nonfinite"],
                            agree=t["agree"], **kw)

    def _predict(self, model, images, task, **kw):
        model.eval()
        with torch.no_grad():
            feat = model.features(images, task).contiguous()
            w, b = model.head_params(task)
            return self._head(feat, w.detach(), b.detach(), **kw)

    def add(self, *source, target=None, const_group=None, map_kind=None, want_label=False, want_nearest=False):
        """``add(model, images, task)`` or, for the penultimate layer, ``add(features, weight, bias)``;
        ``target`` u8 [N,2H,2W] on the device (grouped by the meter's lut) or None (``const_group``,
        default the meter's).  -> (label, nearest, code map of ``map_kind``), None where not asked for; on
        the encoder layer the maps are flat, one entry per row of the layer's grid, and there is no label."""
        if len(source) != 3:
            raise RuntimeError("mdil DensityMeter.add: expects (model, images, task) or (features, weight, bias)")
        if target is not None and self.lut is None:
            raise RuntimeError("mdil DensityMeter.add: a target needs the meter's lut (openset.group_lut)")
        group = self.const_group if const_group is None else const_group
        if self.layer == "encoder":
            return self._add_rows(*source, target=target, const_group=group, map_kind=map_kind, want_nearest=want_nearest)
        fn, dev, N, H, W = rc.meter_source("DensityMeter", _PATH, source, 1, self._predict, self._head, "features")
        self._ready(dev)
        out = fn(*source, target=target, lut=self.lut if target is not None else None, const_group=group,
                 map_kind=map_kind, want_label=want_label, want_nearest=want_nearest)
        self.pixels += N * 2 * H * 2 * W
        return out

    def _add_rows(self, model, images, task, target, const_group, map_kind, want_nearest):
        from . import latent
        if not isinstance(model, torch.nn.Module):
            raise RuntimeError("mdil DensityMeter.add: the encoder layer takes (model, images, task)")
        feat = latent.latents(model, images, task, "encoder")
        self._ready(feat.device)
        group = None
        if target is not None:
            small = latent.resize_labels(target, feat.shape[1], feat.shape[2]).to(device=feat.device, dtype=torch.uint8)
            group = self.lut[small.reshape(-1).long()].contiguous()
        t = self.tensors
        nearest, code = density_rows(feat, self.model, group, const_group, self.kinds, map_kind, t["hist"],
                                     t["nonfinite"], want_nearest)
        self.pixels += feat.shape[0] * feat.shape[1] * feat.shape[2]
        self.grid = [int(feat.shape[1]), int(feat.shape[2])]
        return None, nearest, code

    def hist(self):
        """The histogram as a host int64 [2,2,65536] tensor."""
        return self.tensors["hist"].cpu() if self.tensors else torch.zeros(len(KINDS), 2, CODES, dtype=torch.int64)

    def nonfinite(self):
        return int(self.tensors["nonfinite"].item()) if self.tensors else 0

    def agree(self):
        """-> (pixels of group 0, those of them whose nearest class mean is the head's label)."""
        return tuple(self.tensors["agree"].tolist()) if self.tensors else (0, 0)

    def report(self, tpr=OS.DEFAULT_TPR):
        """-> {"pixels", "nonfinite", "known_pixels", "nearest_agrees", "kinds": {name: openset.metrics(...)}}"""
        hist = self.hist()
        known, same = self.agree()
        kinds = {}
        for k in self.kinds:
            kinds[k] = OS.metrics(hist[KINDS.index(k)], tpr)
            kinds[k]["occupied_bins"] = int((hist[KINDS.index(k)].sum(0) > 0).sum())
        return {"pixels": self.pixels, "nonfinite": self.nonfinite(), "known_pixels": known, "nearest_agrees": same,
                "kinds": kinds}


# ------------------------------------------------------------------------------------------ CLI
def _data_args(args, dataset, task, synthetic, subset=None):
    d = Namespace(**vars(args))
    d.dataset, d.task, d.synthetic = dataset, task, synthetic
    if subset is not None:
        d.subset = subset
    return d


def _fit(args, dev, nc, net):
    from . import similarity as S
    meter, n = None, 0
    for _, images, target in rc.batches(_data_args(args, args.dataset, args.task, args.synthetic), nc, dev):
        meter = S.population(net, images, args.task, args.layer, labels=target, meter=meter, classes=nc - 1)
        n += images.shape[0]
    if meter is None:
        raise RuntimeError("--fit: the split holds no image")
    model = fit_model(meter.moments(), args.ridge, args.min_rows, layer=args.layer, task=args.task, nc=nc)
    save_model(model, args.fit)
    report = {"mode": "fit", "dataset": rc.source_name(args), "subset": args.subset, "task": args.task, "layer": args.layer,
              "images": n, "rows": model["rows"], "channels": model["C"], "num_classes": nc, "ridge": model["ridge"],
              "ridge_note": "untuned", "min_rows": model["min_rows"], "classes": model["cls"].tolist(),
              "dropped_classes": model["dropped"].tolist(), "rows_per_class": model["counts"].tolist(), "model": args.fit}
    print(f"{args.layer}: {model['rows']} rows of {model['C']} channels from {n} images; {len(model['cls'])} class means, "
          f"classes below {model['min_rows']} rows left out: {report['dropped_classes']}; ridge {model['ridge']:g} (untuned) "
          f"-> {args.fit}")
    return report


def _lut(args, nc_data, foreign):
    void = nc_data - 1
    if foreign:                                        # every non-void pixel of the set is known
        return OS.group_lut((), sorted({void, *args.ignore_ids})), []
    unknown_ids = list(args.unknown_ids) if args.unknown_ids else [void]
    return OS.group_lut(unknown_ids, args.ignore_ids), unknown_ids


def _score(args, dev, nc, net, fitted):
    from . import route
    from .fullres import iou_rule
    nc_data = args.num_classes[args.data_task]
    foreign = bool(args.foreign_dataset or args.foreign_synthetic)
    lut, unknown_ids = _lut(args, nc_data, foreign)
    meter = DensityMeter(nc, fitted, KINDS, lut, layer=args.layer)
    head = args.layer == "penultimate"
    logit = OS.OpenSetMeter(nc, OS.KINDS, lut) if args.with_logit_scores else None
    same_space = head and args.data_task == args.task
    conf = {"head": torch.zeros(nc, nc, dtype=torch.int64, device=dev), "nearest": torch.zeros(nc, nc, dtype=torch.int64, device=dev)}
    seen = 0
    for _, images, target in rc.batches(_data_args(args, args.dataset, args.data_task, args.synthetic), nc_data, dev):
        label, nearest, _ = meter.add(net, images, args.task, target=target, want_label=same_space, want_nearest=same_space)
        if same_space:
            conf["head"] += route.confusion(label, target, nc, nc - 1)[0]
            conf["nearest"] += route.confusion(nearest, target, nc, nc - 1)[0]
        if logit is not None:
            logit.add(net, images, args.task, target=target)
        seen += images.shape[0]
    foreign_seen = 0
    if foreign:
        f_args = _data_args(args, args.foreign_dataset, args.foreign_task, args.foreign_synthetic)
        for _, images, _ in rc.batches(f_args, args.num_classes[args.foreign_task], dev, score=False):
            meter.add(net, images, args.task, const_group=UNKNOWN)
            if logit is not None:
                logit.add(net, images, args.task, const_group=UNKNOWN)
            foreign_seen += images.shape[0]
    report = {"mode": "score", "dataset": rc.source_name(args), "task": args.task, "data_task": args.data_task,
              "layer": args.layer, "images": seen, "unknown_ids": unknown_ids, "ignore_ids": list(args.ignore_ids),
              "classes": fitted["cls"].tolist(), "dropped_classes": fitted["dropped"].tolist(), "ridge": fitted["ridge"],
              "ridge_note": "untuned",
              "grid": "the head's output pixels (each feature pixel's score at its four output pixels)" if head
              else "the encoder's own grid, labels resized to it (nearest)"}
    if foreign:
        report.update(foreign_dataset="synthetic" if args.foreign_synthetic else args.foreign_dataset,
                      foreign_task=args.foreign_task, foreign_images=foreign_seen)
    report.update(meter.report(args.tpr))
    if not head:
        report["grid_size"] = meter.grid
    known, same = report["known_pixels"], report["nearest_agrees"]
    report["nearest_agreement"] = same / known if head and known else None
    report["mIoU"] = None
    if same_space:
        report["mIoU"] = {}
        for name, m in conf.items():
            d = m.cpu().double()
            miou, per_class = iou_rule(nc, nc - 1, d.diagonal(), d.sum(0), d.sum(1))
            report["mIoU"][name] = {"mIoU": float(miou), "iou_classes": [float(v) for v in per_class]}
    hist = meter.hist()
    tables = [(k, report["kinds"][k], hist[KINDS.index(k)]) for k in meter.kinds]
    if logit is not None:
        lh = logit.hist()
        report["logit_kinds"] = logit.report(args.tpr)["kinds"]
        for k, m in report["logit_kinds"].items():
            m["occupied_bins"] = int((lh[OS.KINDS.index(k)].sum(0) > 0).sum())
        tables += [(k, report["logit_kinds"][k], lh[OS.KINDS.index(k)]) for k in OS.KINDS]
    for k, m, h in tables:                             # the occupied bins: the metrics can be formed again from them
        m["hist"] = {name: [[int(b), int(h[g, b])] for b in h[g].nonzero().reshape(-1)]
                     for g, name in ((KNOWN, "known"), (UNKNOWN, "unknown"))}
        print(f"{k:9s} AUROC {m['auroc'] * 100:6.2f} %  AUPR {m['aupr'] * 100:6.2f} %  FPR at {args.tpr * 100:g} % TPR "
              f"{m['fpr_at_tpr'] * 100:6.2f} % (code >= {m['threshold_code']})  tie mass {m['tie_mass']:.3g}  "
              f"P {m['P']}  N {m['N']}  bins {m['occupied_bins']}")
    if report["nearest_agreement"] is not None:
        print(f"nearest class mean = the head's label on {report['nearest_agreement'] * 100:.2f} % of {known} known pixels")
    if report["mIoU"]:
        print(f"mIoU: head {report['mIoU']['head']['mIoU'] * 100:.2f} %  nearest class mean "
              f"{report['mIoU']['nearest']['mIoU'] * 100:.2f} %")
    print(f"{report['nonfinite']} non-finite pixels; ridge {fitted['ridge']:g} is untuned")
    return report


def _fit_threshold(args, dev, nc, net, fitted):
    nc_data = args.num_classes[args.data_task]
    lut, unknown_ids = _lut(args, nc_data, False)
    meter = DensityMeter(nc, fitted, KINDS, lut)
    n = 0
    for _, images, target in rc.batches(_data_args(args, args.dataset, args.data_task, args.synthetic), nc_data, dev):
        meter.add(net, images, args.task, target=target)
        n += images.shape[0]
    hist = meter.hist()
    kinds = {}
    for k in meter.kinds:
        known = hist[KINDS.index(k), KNOWN]
        t = OS.threshold_at_known_fpr(known, args.known_fpr)
        kinds[k] = {"threshold_code": t, "threshold_score": OS.threshold_score(t), "known_pixels": int(known.sum()),
                    "rejected_known": int(known[t:].sum()), "cdf_starts": OS.cdf_starts(OS.cdf_lut(known))}
        print(f"{k:9s} reject code >= {t} (score >= {kinds[k]['threshold_score']}): "
              f"{kinds[k]['rejected_known']} of {kinds[k]['known_pixels']} known pixels")
    report = {"mode": "fit-threshold", "dataset": rc.source_name(args), "task": args.task, "data_task": args.data_task,
              "images": n, "known_fpr": args.known_fpr, "unknown_ids": unknown_ids, "ignore_ids": list(args.ignore_ids),
              "num_classes": nc, "nonfinite": meter.nonfinite(), "kinds": kinds}
    hc.write_json(report, args.fit_threshold)
    return report


def read_threshold(path, kind, nc):
    """The fit of ``kind`` in a ``--fit-threshold`` file -> (threshold code, cdf u8 [65536] on the host)."""
    import json
    with open(path) as f:
        saved = json.load(f)
    if saved.get("mode") != "fit-threshold" or kind not in saved.get("kinds", {}):
        raise RuntimeError(f"--threshold {path}: not a --fit-threshold file that holds the kind {kind}")
    if saved.get("num_classes") != nc:
        raise RuntimeError(f"--threshold {path}: fitted on a head of {saved.get('num_classes')} classes, this one has {nc}")
    k = saved["kinds"][kind]
    return OS.check_thr("--threshold", k["threshold_code"]), OS.cdf_from_starts(k["cdf_starts"])


def _write_maps(args, dev, nc, net, fitted):
    from . import predict as P
    thr, cdf = read_threshold(args.threshold, args.kind, nc)
    cdf = cdf.to(dev)
    os.makedirs(args.out, exist_ok=True)
    palette = None
    if args.colour:                                    # the classes' colours; white for the reject id
        palette = torch.full((256, 3), 255, dtype=torch.uint8)
        palette[:nc] = P.default_palette(nc)
        palette = palette.to(dev)
    meter = DensityMeter(nc, fitted, [args.kind])
    counters = OS.new_apply_counters(nc, dev)
    some = {k: counters[k] for k in ("seen", "rejected", "bad_labels")}
    n = 0
    with hc.png_pool() as pool:
        png = hc.PngWriter(pool, args.out)
        nc_data = None if args.images else args.num_classes[args.data_task]
        for stems, images, _ in rc.image_or_dataset_batches(_data_args(args, None, args.data_task, args.synthetic), nc_data,
                                                            pool, dev, score=False):
            label, nearest, code = meter.add(net, images, args.task, const_group=IGNORED, map_kind=args.kind,
                                             want_label=True, want_nearest=args.nearest)
            out, score = OS.openset_apply(label, code, nc, thr, None, args.unknown_id, cdf, counters=some)
            planes = [out.unsqueeze(3), score.unsqueeze(3)]
            if nearest is not None:
                planes.append(nearest.unsqueeze(3))
            if palette is not None:
                planes.append(palette[out.long()])
            host = torch.cat(planes, 3).cpu().numpy()
            png.wait()                                 # the batch before this one: bounds what is in flight
            for j, stem in enumerate(stems):
                png.submit(host[j, :, :, 0], f"{stem}_label.png")
                png.submit(host[j, :, :, 1], f"{stem}_unknown.png")
                if nearest is not None:
                    png.submit(host[j, :, :, 2], f"{stem}_nearest.png")
                if palette is not None:
                    png.submit(host[j, :, :, -3:], f"{stem}_colour.png")
            n += len(stems)
        png.wait()
    seen, rejected = counters["seen"].tolist(), counters["rejected"].tolist()
    report = {"mode": "maps", "dataset": rc.source_name(args), "task": args.task, "images": n, "kind": args.kind,
              "threshold_code": thr, "unknown_id": args.unknown_id, "seen": seen, "rejected": rejected,
              "rejected_share": sum(rejected) / max(1, sum(seen)), "nonfinite": meter.nonfinite(), "written": png.written}
    print(f"{n} images: {report['rejected_share'] * 100:.2f} % of {sum(seen)} pixels rejected ({args.kind} code >= {thr}); "
          f"{len(png.written)} maps written to {args.out}")
    return report


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
    if args.fit and args.data_task != args.task:
        raise RuntimeError("--fit takes the class means from --task's own labels: --data-task does not go with it")
    if args.foreign_synthetic and args.foreign_task == args.data_task:
        raise RuntimeError("--foreign-synthetic draws the domain of --foreign-task, which is --data-task's: the same "
                           "images; give another --foreign-task")
    nc_data = args.num_classes[args.data_task]
    for name, ids in (("--unknown-ids", args.unknown_ids), ("--ignore-ids", args.ignore_ids)):
        if any(not 0 <= v < nc_data for v in ids):
            raise RuntimeError(f"{name} {ids}: task {args.data_task}'s labels lie in [0, {nc_data})")
    if args.threshold and not os.path.isfile(args.threshold):
        raise RuntimeError(f"--threshold {args.threshold}: no such file")
    nc = args.num_classes[args.task]
    fitted = None
    if args.model:
        fitted = load_model(args.model, layer=args.layer, nc=nc, task=args.task)
        args.layer = fitted["layer"]
        if args.layer not in FIT_LAYERS:
            raise RuntimeError(f"--model {args.model}: fitted for the layer {args.layer!r}, the report knows {FIT_LAYERS}")
        if args.layer != "penultimate" and (args.fit_threshold or args.out or args.with_logit_scores):
            raise RuntimeError(f"--model {args.model} was fitted on the {args.layer} layer: thresholds, reject maps and "
                               "--with-logit-scores need the penultimate layer, whose grid the head's labels share")
    elif args.layer is None:
        args.layer = "penultimate"
    dev, _, net = hc.load_model(args.state, args.num_classes, args.task)
    if args.fit:
        report = _fit(args, dev, nc, net)
    elif args.score:
        report = _score(args, dev, nc, net, fitted)
    elif args.fit_threshold:
        report = _fit_threshold(args, dev, nc, net, fitted)
    else:
        report = _write_maps(args, dev, nc, net, fitted)
    if args.json:
        hc.write_json(report, args.json)
    return report


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused."""
    modes = [bool(args.fit), bool(args.score), bool(args.fit_threshold), bool(args.out)]
    if sum(modes) != 1:
        raise RuntimeError("give one of --fit MODEL.npz, --score (with --model and --json FILE), --fit-threshold FILE "
                           "(with --model) or --out DIR (with --model and --threshold FILE)")
    if args.fit and args.model:
        raise RuntimeError("--fit MODEL.npz writes a model, --model MODEL.npz reads one: give one of them")
    if not args.fit and not args.model:
        raise RuntimeError("--score, --fit-threshold and --out need --model MODEL.npz (written by --fit)")
    if args.score and not args.json:
        raise RuntimeError("--score writes its report to --json FILE")
    if args.out and not args.threshold:
        raise RuntimeError("--out DIR needs --threshold FILE (written by --fit-threshold)")
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
    if args.layer == "encoder" and (args.fit_threshold or args.out):
        raise RuntimeError("--layer encoder: thresholds and reject maps need the penultimate layer, whose grid the "
                           "head's labels share; the encoder layer is scored with --score alone")
    if args.layer == "encoder" and args.with_logit_scores:
        raise RuntimeError("--with-logit-scores compares on the head's output pixels: it needs --layer penultimate")
    if args.with_logit_scores and not args.score:
        raise RuntimeError("--with-logit-scores goes with --score")
    if args.nearest and not args.out:
        raise RuntimeError("--nearest writes <stem>_nearest.png: it goes with --out DIR")
    if (args.foreign_dataset or args.foreign_synthetic) and not args.score:
        raise RuntimeError("--foreign-dataset goes with --score")
    if args.foreign_dataset and args.foreign_synthetic:
        raise RuntimeError("--foreign-dataset and --foreign-synthetic exclude each other")
    if (args.foreign_dataset or args.foreign_synthetic) and args.unknown_ids:
        raise RuntimeError("--foreign-dataset makes every pixel of the foreign images the unknowns: --unknown-ids does "
                           "not go with it")
    if args.fit and (args.unknown_ids or args.ignore_ids):
        raise RuntimeError("--fit uses every labelled pixel but the void class: --unknown-ids and --ignore-ids go with "
                           "--score and --fit-threshold")
    if min(args.height, args.width, args.batch_size) < 1 or args.synthetic < 0 or args.foreign_synthetic < 0:
        raise RuntimeError("sizes and --batch-size must be positive")
    if args.height % 8 or args.width % 8:
        raise RuntimeError("--height and --width must be multiples of 8 (the encoder's stride)")
    if not (args.ridge >= 0.0 and args.ridge < float("inf")):
        raise RuntimeError(f"--ridge {args.ridge} must be a finite number >= 0")
    if args.min_rows is not None and args.min_rows < 1:
        raise RuntimeError(f"--min-rows {args.min_rows} must be at least 1")
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
    p = hc.RefusingParser(_refusals, description="density report of a checkpoint: Mahalanobis open-set scores in feature "
                                                 "space, the nearest class mean, AUROC / AUPR / FPR at 95 % TPR, reject "
                                                 "thresholds and label maps with a reject id")
    p.add_argument("--state", required=True, help="checkpoint written by the trainers (or by the reference)")
    p.add_argument("--num-classes", type=int, nargs="+", required=True)
    p.add_argument("--task", type=int, required=True, help="which task's decoder runs")
    rc.add_data_flags(p, dataset_help="a labelled dataset", synthetic_help="N procedural images instead (labelled)")
    p.add_argument("--fit", help="fit the Gaussians on this split and write the model (.npz) here")
    p.add_argument("--layer", choices=FIT_LAYERS, help="--fit: which features (default penultimate); else checked "
                                                       "against the model's")
    p.add_argument("--ridge", type=float, default=DEFAULT_RIDGE,
                   help="added to both covariances as ridge * mean variance * I (default %(default)s; untuned)")
    p.add_argument("--min-rows", type=int, help="classes with fewer rows get no mean (default 2 C)")
    p.add_argument("--model", help="a model written by --fit")
    p.add_argument("--data-task", type=int, help="open the dataset in this task's label space (default --task)")
    p.add_argument("--score", action="store_true", help="judge the scores against the unknown pixels; needs --json")
    p.add_argument("--with-logit-scores", action="store_true",
                   help="--score: openset's four logit scores on the same pixels, in the same table")
    p.add_argument("--unknown-ids", type=int, nargs="+", default=[],
                   help="target ids that count as unknown (default: the void class of --data-task)")
    p.add_argument("--ignore-ids", type=int, nargs="+", default=[], help="target ids left out of both groups")
    p.add_argument("--tpr", type=float, default=OS.DEFAULT_TPR, help="the TPR at which the FPR is read (default %(default)s)")
    p.add_argument("--foreign-dataset", choices=("cityscapes", "BDD", "IDD"),
                   help="with --score: every pixel of this dataset's images is unknown, every non-void pixel of "
                        "--dataset known")
    p.add_argument("--foreign-synthetic", type=int, default=0, help="N procedural images of --foreign-task's domain instead")
    p.add_argument("--foreign-task", type=int, help="the label space / domain of the foreign images (default --task)")
    p.add_argument("--fit-threshold", help="write per kind the reject threshold at --known-fpr and the known pixels' CDF here")
    p.add_argument("--known-fpr", type=float, default=OS.DEFAULT_KNOWN_FPR,
                   help="share of the known pixels that the fitted threshold may reject (default %(default)s)")
    p.add_argument("--images", help="folder of unlabelled .jpg / .png images (searched recursively)")
    p.add_argument("--threshold", help="a file written by --fit-threshold")
    p.add_argument("--kind", default="maha", help="the score that rejects (default %(default)s)")
    p.add_argument("--out", help="write <stem>_label.png (train ids, --unknown-id where rejected) and <stem>_unknown.png here")
    p.add_argument("--unknown-id", type=int, default=255)
    p.add_argument("--colour", action="store_true", help="also write <stem>_colour.png (white where rejected)")
    p.add_argument("--nearest", action="store_true", help="also write <stem>_nearest.png (the nearest class mean's id)")
    p.add_argument("--json", help="write the report here")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
