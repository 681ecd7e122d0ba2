"""Representation similarity on MI355X: what an incremental step does to the representation, and how
far apart two domains lie as the network sees them, over a whole validation set.

Everything here is a function of first and second moments of feature rows -- class counts,
per-class sums and the Gram blocks X^T X, Y^T Y, X^T Y -- which one fused kernel accumulates on the
exact-fp32 MFMA from the two models' NHWC features read once, a pivot subtracted on the way in and
the partial sums reduced in fp64 in a fixed order (include/mdil_similarity.h).  The rest is small
fp64 algebra on the host: linear CKA, the Frechet distance, per-class centroid shift, separability.

    python -m mdil_ss_amd.similarity --before CKPT --before-num-classes 20 \
        --after CKPT --after-num-classes 20 20 --task 0 (--dataset cityscapes|BDD|IDD | --synthetic N) \
        [--layers encoder penultimate logits] [--json FILE] [--subset val --height 512 --width 1024 --batch-size 6]

per layer: linear CKA between the two checkpoints, class separability before and after, per-class
centroid shift.

    python -m mdil_ss_amd.similarity --state CKPT --num-classes 20 20 \
        (--task-a 0 --dataset-a cityscapes [--datadir-a DIR] --task-b 1 --dataset-b BDD [--datadir-b DIR] |
         --task-a 0 --task-b 1 --synthetic N) [--layers ...] [--json FILE]

per layer: the Frechet distance between the two domains' features and, when both tasks have the
same class count, the distance between their per-class centroids.  Rows labelled with the task's
last (ignore) class are left out of every moment."""
from argparse import Namespace

import numpy as np
import torch

from . import _head_common as hc
from . import _report_common as rc
from . import _similarity_lib
from . import latent

LAYERS = latent.LAYERS
_FN, _PATH = "similarity", "similarity"
MAX_CX, MAX_CY, MAX_CLASSES = _similarity_lib.MAX_CX, _similarity_lib.MAX_CY, _similarity_lib.MAX_CLASSES
MAX_ROWS = _similarity_lib.MAX_ROWS
ROWS_PER_CALL = 1 << 20                        # bounds the workspace: 176 MB at 128 + 128 channels
PIVOT_ROWS = 1024                              # the default pivot: the mean of this many first rows


def _chk(t, name, dtype=torch.float32):
    hc.chk(_FN, _PATH, t, name, dtype)


# ----------------------------------------------------------------------------------- the device
class MomentMeter:
    """Accumulates the moments of feature rows over many batches: ``x`` [rows, cx] alone, or paired
    with ``y`` [rows, cy] at the same positions, with u8 ``labels`` [rows] in [0, nc) (a row with a
    larger label is skipped).  The pivots are fixed by the first ``add``: the per-channel mean of
    its first rows unless ``pivot_x`` / ``pivot_y`` are given."""

    def __init__(self, cx, cy, nc, device, pivot_x=None, pivot_y=None):
        cx, cy, nc = int(cx), int(cy), int(nc)
        if not 1 <= cx <= MAX_CX:
            raise RuntimeError(f"mdil {_FN}: cx {cx} channels (supported: 1 to {MAX_CX})")
        if not 0 <= cy <= MAX_CY:
            raise RuntimeError(f"mdil {_FN}: cy {cy} channels (supported: 0 to {MAX_CY})")
        if not 1 <= nc <= MAX_CLASSES:
            raise RuntimeError(f"mdil {_FN}: nc {nc} classes (supported: 1 to {MAX_CLASSES})")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"mdil {_FN}: device must be a cuda device (got {device}); there is no CPU fallback "
                               f"in the {_PATH} path")
        self.cx, self.cy, self.nc, self.device = cx, cy, nc, device
        self.state = self.workspace = None      # on the device from the first add on
        self.pivot_x = self._given_pivot(pivot_x, cx, "pivot_x")
        self.pivot_y = self._given_pivot(pivot_y, cy, "pivot_y") if cy else None
        self.rows = 0

    def _given_pivot(self, p, c, name):
        if p is None:
            return None
        p = torch.as_tensor(p, dtype=torch.float32).reshape(-1)
        if p.numel() != c:
            raise RuntimeError(f"mdil {_FN}: {name} must have {c} values (got {p.numel()})")
        return p.contiguous()

    def _rows(self, t, c, name):
        _chk(t, name)
        if t.dim() < 2 or t.shape[-1] != c or t.numel() == 0:
            raise RuntimeError(f"mdil {_FN}: {name} must be float32 [rows,{c}] (got {tuple(t.shape)})")
        if t.device != self.device:
            raise RuntimeError(f"mdil {_FN}: {name} on {t.device}, the meter on {self.device}")
        return t.view(-1, c)

    def reset(self):
        """Clears the accumulated moments; the pivots stay."""
        if self.state is not None:
            self.state.zero_()
        self.rows = 0

    def add(self, x, y=None, labels=None):
        """One batch: ``x`` f32 [..., cx], ``y`` f32 [..., cy] (exactly when cy > 0), ``labels`` u8
        with one entry per row (None: nc must be 1), all contiguous on the meter's device."""
        x = self._rows(x, self.cx, "x")
        rows = x.shape[0]
        if (y is not None) != (self.cy > 0):
            raise RuntimeError(f"mdil {_FN}: y must be given exactly when cy > 0 (cy {self.cy})")
        if y is not None:
            y = self._rows(y, self.cy, "y")
            if y.shape[0] != rows:
                raise RuntimeError(f"mdil {_FN}: x has {rows} rows and y {y.shape[0]}")
        if labels is None:
            if self.nc != 1:
                raise RuntimeError(f"mdil {_FN}: labels are needed with nc {self.nc} classes")
        else:
            _chk(labels, "labels", torch.uint8)
            if labels.numel() != rows or labels.device != self.device:
                raise RuntimeError(f"mdil {_FN}: labels must be uint8 [{rows}] on {self.device} "
                                   f"(got {tuple(labels.shape)} on {labels.device})")
            labels = labels.view(-1)
        lib = _similarity_lib.load()
        if self.state is None:
            self.state = torch.zeros(lib.mdil_sim_state_bytes(self.cx, self.cy, self.nc) // 8, dtype=torch.float64,
                                     device=self.device)
        if self.pivot_x is None:
            self.pivot_x = x[:PIVOT_ROWS].cpu().double().mean(0).float()
        if y is not None and self.pivot_y is None:
            self.pivot_y = y[:PIVOT_ROWS].cpu().double().mean(0).float()
        self.pivot_x = self.pivot_x.to(self.device)
        self.pivot_y = None if y is None else self.pivot_y.to(self.device)
        with torch.no_grad(), torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            for r0 in range(0, rows, ROWS_PER_CALL):
                n = min(ROWS_PER_CALL, rows - r0)
                need = lib.mdil_sim_workspace_bytes(n, self.cx, self.cy, self.nc)
                if self.workspace is None or self.workspace.numel() < need:
                    self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
                _similarity_lib.check(
                    lib.mdil_sim_accumulate(x[r0:r0 + n].data_ptr(), hc.ptr(None if y is None else y[r0:r0 + n]),
                                            hc.ptr(None if labels is None else labels[r0:r0 + n]), n, self.cx, self.cy,
                                            self.nc, self.pivot_x.data_ptr(), hc.ptr(self.pivot_y),
                                            self.state.data_ptr(), self.workspace.data_ptr(), stream),
                    "mdil_sim_accumulate")
        self.rows += rows
        return self

    def moments(self):
        """The state on the host, fp64 numpy: ``n`` [nc], ``skipped``, ``sx`` [nc,cx], ``sy`` [nc,cy],
        ``gxx`` [cx,cx], ``gyy`` [cy,cy], ``gxy`` [cx,cy] -- all of the PIVOTED rows -- and the pivots."""
        if self.state is None:
            raise RuntimeError(f"mdil {_FN}: moments() before the first add()")
        return unpack_state(self.state.cpu().numpy(), self.cx, self.cy, self.nc, self.pivot_x.cpu().numpy(),
                            None if self.pivot_y is None else self.pivot_y.cpu().numpy())


def unpack_state(state, cx, cy, nc, pivot_x, pivot_y=None):
    """The flat fp64 ``state`` of include/mdil_similarity.h -> the moments dict (host arrays)."""
    state = np.asarray(state, dtype=np.float64)
    sizes = (("n", (nc,)), ("skipped", ()), ("sx", (nc, cx)), ("sy", (nc, cy)), ("gxx", (cx, cx)), ("gyy", (cy, cy)),
             ("gxy", (cx, cy)))
    want = sum(int(np.prod(shape, dtype=np.int64)) for _, shape in sizes)
    if state.ndim != 1 or state.size != want:
        raise RuntimeError(f"mdil {_FN}: a state of {state.size} values does not fit cx {cx}, cy {cy}, nc {nc} ({want})")
    m, pos = {"cx": cx, "cy": cy, "nc": nc}, 0
    for name, shape in sizes:
        k = int(np.prod(shape, dtype=np.int64))
        m[name] = state[pos:pos + k].reshape(shape).copy() if shape else float(state[pos])
        pos += k
    m["pivot_x"] = np.asarray(pivot_x, dtype=np.float64).reshape(cx)
    m["pivot_y"] = np.zeros(0) if pivot_y is None else np.asarray(pivot_y, dtype=np.float64).reshape(cy)
    return m


def _layer_labels(labels, feat):
    """Labels [N,H,W] at the input's size -> u8 [N*h*w] on the layer's grid (nearest)."""
    if labels is None:
        return None
    if not isinstance(labels, torch.Tensor) or labels.dim() != 3 or labels.shape[0] != feat.shape[0]:
        got = tuple(labels.shape) if isinstance(labels, torch.Tensor) else type(labels).__name__
        raise RuntimeError(f"mdil {_FN}: labels must be a [N,H,W] tensor for the {feat.shape[0]} images (got {got})")
    return latent.resize_labels(labels, feat.shape[1], feat.shape[2]).to(device=feat.device, dtype=torch.uint8).contiguous()


def _meter(meter, cx, cy, labels, classes, device):
    if meter is not None:
        return meter
    if labels is not None and classes is None:
        raise RuntimeError(f"mdil {_FN}: labels without a meter need classes=")
    return MomentMeter(cx, cy, 1 if labels is None else classes, device)


def compare(model_a, model_b, images, task, layer, labels=None, meter=None, classes=None):
    """Feeds the ``layer`` features of ``model_a`` (x) and ``model_b`` (y) on ``images`` [N,3,H,W] for
    ``task``, with ``labels`` [N,H,W] resized to the layer's grid, into ``meter`` (a new one of
    ``classes`` classes when None).  -> the meter."""
    fa, fb = latent.latents(model_a, images, task, layer), latent.latents(model_b, images, task, layer)
    if fa.shape[:3] != fb.shape[:3]:
        raise RuntimeError(f"mdil {_FN}: the two models' {layer} grids differ ({tuple(fa.shape)}, {tuple(fb.shape)})")
    meter = _meter(meter, fa.shape[3], fb.shape[3], labels, classes, fa.device)
    return meter.add(fa, fb, _layer_labels(labels, fa))


def population(model, images, task, layer, labels=None, meter=None, classes=None):
    """Feeds the ``layer`` features of one model (x alone) into ``meter``.  -> the meter."""
    f = latent.latents(model, images, task, layer)
    meter = _meter(meter, f.shape[3], 0, labels, classes, f.device)
    return meter.add(f, None, _layer_labels(labels, f))


# ------------------------------------------------------------------------------------- the host
def _side(m, side):
    """-> (N, per-class sums [nc,c], Gram [c,c], pivot [c]) of side "x" or "y"."""
    if side == "y" and not m["cy"]:
        raise RuntimeError(f"mdil {_FN}: these moments hold one population (cy 0)")
    N = float(np.sum(m["n"]))
    if N <= 0:
        raise RuntimeError(f"mdil {_FN}: no rows were counted")
    return N, np.asarray(m["s" + side], dtype=np.float64), np.asarray(m["g" + side + side], dtype=np.float64), \
        np.asarray(m["pivot_" + side], dtype=np.float64)


def covariances(m):
    """The means (pivot undone) and the centred covariances, normalised by the row count N:
    ``mean_x``, ``cxx`` and, with two populations, ``mean_y``, ``cyy``, ``cxy``; ``n`` = N."""
    N, sx, gxx, px = _side(m, "x")
    mx = sx.sum(0) / N
    out = {"n": N, "mean_x": px + mx, "cxx": gxx / N - np.outer(mx, mx)}
    if m["cy"]:
        _, sy, gyy, py = _side(m, "y")
        my = sy.sum(0) / N
        out.update(mean_y=py + my, cyy=gyy / N - np.outer(my, my),
                   cxy=np.asarray(m["gxy"], dtype=np.float64) / N - np.outer(mx, my))
    return out


def linear_cka(m):
    """|Cxy|_F^2 / (|Cxx|_F |Cyy|_F) on the centred covariances."""
    c = covariances(m)
    if "cxy" not in c:
        raise RuntimeError(f"mdil {_FN}: linear_cka needs two populations (cy 0)")
    den = np.linalg.norm(c["cxx"]) * np.linalg.norm(c["cyy"])
    return float(np.linalg.norm(c["cxy"]) ** 2 / den) if den > 0 else float("nan")


def _psd_sqrt(S):
    w, V = np.linalg.eigh((S + S.T) / 2)
    return (V * np.sqrt(np.clip(w, 0.0, None))) @ V.T


def frechet(m_a, m_b):
    """|mu_a - mu_b|^2 + tr S_a + tr S_b - 2 tr (S_a^1/2 S_b S_a^1/2)^1/2 between the x populations of
    two moment sets (``eigh`` twice, eigenvalues clipped at 0)."""
    a, b = covariances(m_a), covariances(m_b)
    if a["cxx"].shape != b["cxx"].shape:
        raise RuntimeError(f"mdil {_FN}: frechet between {a['cxx'].shape[0]} and {b['cxx'].shape[0]} channels")
    ra = _psd_sqrt(a["cxx"])
    M = ra @ b["cxx"] @ ra
    w = np.linalg.eigvalsh((M + M.T) / 2)
    d = a["mean_x"] - b["mean_x"]
    return float(d @ d + np.trace(a["cxx"]) + np.trace(b["cxx"]) - 2.0 * np.sqrt(np.clip(w, 0.0, None)).sum())


def _scatter(m, side):
    """-> (tr S_b, tr S_w, N) of one side: S_w = G - sum_c n_c mu_c mu_c^T, S_b = sum_c n_c (mu_c - mu)(mu_c - mu)^T
    (in pivoted coordinates; both are shift-invariant)."""
    N, s, g, _ = _side(m, side)
    n = np.asarray(m["n"], dtype=np.float64)
    have = n > 0
    mu_c = s[have] / n[have, None]
    mu = s.sum(0) / N
    tr_w = np.trace(g) - float((n[have, None] * mu_c * mu_c).sum())
    tr_b = float((n[have, None] * (mu_c - mu) ** 2).sum())
    return tr_b, tr_w, N


def separability(m):
    """tr S_b / tr S_w, between-class over within-class scatter: {"x": ..., "y": ... or None}."""
    out = {}
    for side in ("x", "y"):
        if side == "y" and not m["cy"]:
            out[side] = None
            continue
        tr_b, tr_w, _ = _scatter(m, side)
        out[side] = float(tr_b / tr_w) if tr_w > 0 else float("nan")
    return out


def class_shift(m, other=None):
    """Per class present on both sides, |mu_x,c - mu_y,c| and the same over the root of the pooled
    within-class variance of x (tr S_w / N).  The two sides are x and y of ``m``, or, with ``other``,
    the x populations of ``m`` and ``other``.  -> {"classes": [...], "shift": [...], "relative": [...]}."""
    _, sa, _, pa = _side(m, "x")
    na = np.asarray(m["n"], dtype=np.float64)
    if other is None:
        _, sb, _, pb = _side(m, "y")
        nb = na
    else:
        _, sb, _, pb = _side(other, "x")
        nb = np.asarray(other["n"], dtype=np.float64)
    if sa.shape != sb.shape:
        raise RuntimeError(f"mdil {_FN}: class_shift between {sa.shape} and {sb.shape} class sums")
    _, tr_w, N = _scatter(m, "x")
    sigma = np.sqrt(max(tr_w, 0.0) / N)
    classes = [c for c in range(len(na)) if na[c] > 0 and nb[c] > 0]
    shift = [float(np.linalg.norm((pa + sa[c] / na[c]) - (pb + sb[c] / nb[c]))) for c in classes]
    return {"classes": classes, "shift": shift, "relative": [s / sigma if sigma > 0 else float("nan") for s in shift]}


# ------------------------------------------------------------------------------------------ CLI
def _lists(c):
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def _side_args(args, task, dataset, datadir):
    """The namespace the batch feeder reads, for one side."""
    ns = Namespace(**vars(args))
    ns.task, ns.dataset = task, dataset
    if dataset and datadir:
        from .dataset import _ALIASES
        setattr(ns, {"cityscapes": "cs_datadir", "BDD": "bdd_datadir", "IDD": "idd_datadir"}[_ALIASES[dataset]], datadir)
    return ns


def _feed(args, nc, dev, layers, each):
    """Runs ``each(layer, images, target)`` over every batch and layer; -> the number of images."""
    seen = 0
    for stems, images, target in rc.batches(args, nc, dev, unique_stems=True):
        seen += len(stems)
        for layer in layers:
            each(layer, images, target)
    return seen


def _checkpoints(args):
    dev, nc, before = hc.load_model(args.before, args.before_num_classes, args.task)
    _, _, after = hc.load_model(args.after, args.after_num_classes, args.task)
    meters = {}

    def each(layer, images, target):
        meters[layer] = compare(before, after, images, args.task, layer, labels=target, meter=meters.get(layer),
                                classes=nc - 1)

    images = _feed(_side_args(args, args.task, args.dataset, None), nc, dev, args.layers, each)
    report = {"mode": "checkpoints", "dataset": "synthetic" if args.synthetic else args.dataset, "task": args.task,
              "images": images, "classes": nc - 1, "layers": {}}
    print(f"{report['dataset']} (task {args.task}), before -> after, {images} images")
    print(f"{'layer':<12} {'rows':>10} {'CKA':>9} {'sep before':>11} {'sep after':>10} {'max shift':>10} {'(class)':>8}")
    for layer in args.layers:
        m = meters[layer].moments()
        sep, shift = separability(m), class_shift(m)
        worst = int(np.argmax(shift["relative"])) if shift["classes"] else None
        entry = {"rows": float(np.sum(m["n"])), "skipped": m["skipped"], "channels": [m["cx"], m["cy"]],
                 "cka": linear_cka(m), "separability_before": sep["x"], "separability_after": sep["y"],
                 "class_shift": shift, "rows_per_class": m["n"].tolist(), "matrices": _lists(covariances(m))}
        report["layers"][layer] = entry
        tail = ("-", "-") if worst is None else (f"{shift['relative'][worst]:.4f}", str(shift["classes"][worst]))
        print(f"{layer:<12} {int(entry['rows']):>10} {entry['cka']:>9.6f} {sep['x']:>11.5f} {sep['y']:>10.5f} "
              f"{tail[0]:>10} {tail[1]:>8}")
    return report


def _domains(args):
    dev, _, model = hc.load_model(args.state, args.num_classes, args.task_a)
    sides = {}
    for key, task, dataset, datadir in (("a", args.task_a, args.dataset_a, args.datadir_a),
                                        ("b", args.task_b, args.dataset_b, args.datadir_b)):
        nc, meters = args.num_classes[task], {}

        def each(layer, images, target, task=task, nc=nc, meters=meters):
            meters[layer] = population(model, images, task, layer, labels=target, meter=meters.get(layer),
                                       classes=nc - 1)

        images = _feed(_side_args(args, task, dataset, datadir), nc, dev, args.layers, each)
        sides[key] = (nc, meters, images)
    (nca, ma, ia), (ncb, mb, ib) = sides["a"], sides["b"]
    name = lambda d: "synthetic" if args.synthetic else d  # noqa: E731
    report = {"mode": "domains", "dataset_a": name(args.dataset_a), "dataset_b": name(args.dataset_b),
              "task_a": args.task_a, "task_b": args.task_b, "images_a": ia, "images_b": ib, "layers": {}}
    print(f"{report['dataset_a']} (task {args.task_a}, {ia} images) against {report['dataset_b']} "
          f"(task {args.task_b}, {ib} images)")
    print(f"{'layer':<12} {'Frechet':>12} {'tr cov a':>12} {'tr cov b':>12} {'max centroid distance':>22}")
    for layer in args.layers:
        a, b = ma[layer].moments(), mb[layer].moments()
        ca, cb = covariances(a), covariances(b)
        entry = {"rows_a": ca["n"], "rows_b": cb["n"], "channels": [a["cx"], b["cx"]], "frechet": None,
                 "trace_a": float(np.trace(ca["cxx"])), "trace_b": float(np.trace(cb["cxx"])), "centroid_distance": None,
                 "matrices": {"mean_a": ca["mean_x"].tolist(), "cov_a": ca["cxx"].tolist(),
                              "mean_b": cb["mean_x"].tolist(), "cov_b": cb["cxx"].tolist()}}
        if a["cx"] == b["cx"]:
            entry["frechet"] = frechet(a, b)
            if nca == ncb:
                entry["centroid_distance"] = class_shift(a, b)
        report["layers"][layer] = entry
        cd = entry["centroid_distance"]
        print(f"{layer:<12} " + (f"{entry['frechet']:>12.5f}" if entry["frechet"] is not None else f"{'-':>12}") +
              f" {entry['trace_a']:>12.5f} {entry['trace_b']:>12.5f} " +
              (f"{max(cd['shift']):>22.5f}" if cd and cd["shift"] else f"{'-':>22}"))
    return report


def main(args):
    _refusals(args)
    report = _checkpoints(args) if args.before else _domains(args)
    if args.json:
        hc.write_json(report, args.json)
    return report


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused."""
    ckpt, dom = bool(args.before or args.after), bool(args.state)
    if ckpt == dom:
        raise RuntimeError("give either --before CKPT --after CKPT (two checkpoints on one task) or --state CKPT "
                           "(two domains through one checkpoint)")
    if min(args.height, args.width) < 8 or args.height % 8 or args.width % 8:
        raise RuntimeError("--height and --width must be positive multiples of 8")
    if args.batch_size < 1 or args.synthetic < 0:
        raise RuntimeError("--batch-size must be positive and --synthetic not negative")
    if len(set(args.layers)) != len(args.layers):
        raise RuntimeError("--layers names a layer twice")
    if ckpt:
        if not (args.before and args.after and args.before_num_classes and args.after_num_classes):
            raise RuntimeError("--before, --before-num-classes, --after and --after-num-classes go together")
        if args.task is None:
            raise RuntimeError("--before / --after need --task T")
        ca = rc.refuse_pair(args)
        if bool(args.synthetic) == bool(args.dataset):
            raise RuntimeError("give exactly one of --dataset cityscapes|BDD|IDD and --synthetic N")
        counts = [ca]
    else:
        if not args.num_classes:
            raise RuntimeError("--state needs --num-classes")
        if args.task_a is None or args.task_b is None:
            raise RuntimeError("--state needs --task-a I and --task-b J")
        for flag, task in (("--task-a", args.task_a), ("--task-b", args.task_b)):
            if not 0 <= task < len(args.num_classes):
                raise RuntimeError(f"{flag} {task}: the model has tasks 0 to {len(args.num_classes) - 1}")
        real = bool(args.dataset_a) and bool(args.dataset_b)
        if bool(args.dataset_a) != bool(args.dataset_b) or real == bool(args.synthetic):
            raise RuntimeError("give --dataset-a A and --dataset-b B, or --synthetic N")
        if args.synthetic and args.task_a == args.task_b:
            raise RuntimeError("--synthetic draws one domain per task: --task-a and --task-b must differ")
        counts = [args.num_classes[args.task_a], args.num_classes[args.task_b]]
    for nc in counts:
        if not 2 <= nc <= MAX_CLASSES + 1:
            raise RuntimeError(f"{nc} classes: the similarity path takes 2 to {MAX_CLASSES + 1} (the last is ignored)")


def build_parser():
    names = ("cityscapes", "BDD", "IDD")
    p = hc.RefusingParser(_refusals, description="representation similarity: two checkpoints on one task, or two "
                                                 "domains through one checkpoint")
    p.add_argument("--before", help="checkpoint before the incremental step")
    p.add_argument("--before-num-classes", type=int, nargs="+")
    p.add_argument("--after", help="checkpoint after it")
    p.add_argument("--after-num-classes", type=int, nargs="+")
    p.add_argument("--task", type=int, help="--before / --after: which task's adapters and decoder run")
    p.add_argument("--state", help="one checkpoint, two domains")
    p.add_argument("--num-classes", type=int, nargs="+")
    p.add_argument("--task-a", type=int)
    p.add_argument("--dataset-a", choices=names)
    p.add_argument("--datadir-a", help="root folder of --dataset-a (default: that dataset's own flag)")
    p.add_argument("--task-b", type=int)
    p.add_argument("--dataset-b", choices=names)
    p.add_argument("--datadir-b", help="root folder of --dataset-b")
    p.add_argument("--layers", nargs="+", choices=LAYERS, default=list(LAYERS))
    p.add_argument("--json", help="write the report (with its matrices) here")
    rc.add_data_flags(p, "--before / --after: the validation set",
                      "N procedural images (per domain) instead of datasets")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
