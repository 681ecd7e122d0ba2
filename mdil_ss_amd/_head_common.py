"""What the head drivers share (predict.py, fullres.py, ensemble.py and, with _report_common.py on
top, drift.py, calibrate.py, boundary.py, pseudo.py, route.py, segments.py, refine.py, significance.py,
openset.py, audit.py, acquire.py and ripu.py; latent.py and similarity.py take the loader and the parser): the
argument checks of their entry points -- each takes the entry point's name, so every message reads
as it always did -- the 16-bit map, threshold and counter helpers of the map add-ons (pseudo,
openset, audit, acquire, ripu), the checkpoint loader, the image folder -> image tensor steps, the bounded
PNG writer and the score report of the inference command lines.  _annotate_common.py builds the label
tree writer of audit, acquire and ripu on ``PngWriter`` and ends their ``main`` with ``write_json``."""
import json
import os
from argparse import ArgumentParser
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

MAX_PNG_THREADS = 16


# ------------------------------------------------------------------------- entry-point checks
def chk(fn, path, t, name, dtype=torch.float32):
    """``fn``: "predict_head" ...; ``path``: what the message calls the path ("prediction" ...)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        got = (f"{t.dtype}, {t.device}, contiguous={t.is_contiguous()}" if isinstance(t, torch.Tensor)
               else type(t).__name__)
        raise RuntimeError(f"mdil {fn}: {name} must be a contiguous {str(dtype)[6:]} device tensor "
                           f"(got {got}); there is no CPU fallback in the {path} path")


def ptr(t):
    return None if t is None else t.data_ptr()


def check_params(fn, w, b, x=None):
    """The ``ConvTranspose2d(16, nc, 2, 2)`` parameters, judged together with the one feature tensor
    ``x`` when there is one (the ensemble judges its views itself).  -> nc"""
    bad = w.dim() != 4 or w.shape[0] != 16 or tuple(w.shape[2:]) != (2, 2) or b.numel() != w.shape[1]
    if x is not None:
        if x.dim() != 4 or x.shape[3] != 16 or x.numel() == 0 or bad:
            raise RuntimeError(f"mdil {fn}: expects NHWC features [N,H,W,16] and ConvTranspose2d(16, nc, 2, 2) "
                               f"parameters (got x {tuple(x.shape)}, w {tuple(w.shape)}, bias {tuple(b.shape)})")
    elif bad:
        raise RuntimeError(f"mdil {fn}: expects ConvTranspose2d(16, nc, 2, 2) parameters as weight and bias "
                           f"(got w {tuple(w.shape)}, bias {tuple(b.shape)})")
    return w.shape[1]


def check_nc(fn, lib, nc):
    """-> ``nc`` as an int within the class range of the binding module ``lib``."""
    nc = int(nc)
    if not lib.MIN_CLASSES <= nc <= lib.MAX_CLASSES:
        raise RuntimeError(f"mdil {fn}: {nc} classes (supported: {lib.MIN_CLASSES} to {lib.MAX_CLASSES})")
    return nc


def check_classes(fn, lib, nc, x, w, b, what="features"):
    """``check_nc``, then weight and bias on ``x``'s device."""
    check_nc(fn, lib, nc)
    if w.device != x.device or b.device != x.device:
        raise RuntimeError(f"mdil {fn}: {what} on {x.device}, weight on {w.device}, bias on {b.device}")


def check_out_size(fn, lib, out_size):
    """-> (Ho, Wo)"""
    try:
        Ho, Wo = (int(v) for v in out_size)
    except (TypeError, ValueError):
        raise RuntimeError(f"mdil {fn}: out_size must be (height, width), got {out_size!r}") from None
    if not (1 <= Ho <= lib.MAX_SIZE and 1 <= Wo <= lib.MAX_SIZE):
        raise RuntimeError(f"mdil {fn}: out_size {Ho} x {Wo} outside [1, {lib.MAX_SIZE}]")
    return Ho, Wo


def check_tables(fn, path, dev, dtype, tables):
    """``tables``: (tensor or None, name, shape); those given must be ``dtype`` of that shape on ``dev``."""
    for t, name, shape in tables:
        if t is not None:
            chk(fn, path, t, name, dtype)
            if tuple(t.shape) != shape or t.device != dev:
                raise RuntimeError(f"mdil {fn}: {name} must be {str(dtype)[6:]} {list(shape)} on {dev} "
                                   f"(got {tuple(t.shape)} on {t.device})")


def check_scoring(fn, path, dev, N, nc, Ho, Wo, id_map, palette, target, confusion, bad_targets, ignore_index):
    check_tables(fn, path, dev, torch.uint8,
                 ((id_map, "id_map", (nc,)), (palette, "palette", (nc, 3)), (target, "target", (N, Ho, Wo))))
    if target is None:
        if confusion is not None or bad_targets is not None:
            raise RuntimeError(f"mdil {fn}: confusion / bad_targets given without a target")
    else:
        if confusion is None or bad_targets is None:
            raise RuntimeError(f"mdil {fn}: a target needs confusion (int64 [nc,nc]) and bad_targets "
                               "(int64 [1]) on the device; they are accumulated into")
        check_tables(fn, path, dev, torch.int64,
                     ((confusion, "confusion", (nc, nc)), (bad_targets, "bad_targets", (1,))))
    check_ignore_index(fn, ignore_index)


def check_ignore_index(fn, ignore_index):
    if not -1 <= int(ignore_index) <= 255:
        raise RuntimeError(f"mdil {fn}: ignore_index {ignore_index} outside [-1, 255]")


def check_id(fn, name, v):
    """-> the byte ``v`` that a map is to hold (``name``: "drop_id", "none_id" ...)."""
    if not 0 <= int(v) <= 255:
        raise RuntimeError(f"mdil {fn}: {name} {v} outside [0, 255]")
    return int(v)


# ------------------------------------------------------------- the map add-ons' 16-bit maps and counters
def q_values(qmap):
    """A stored 16-bit map as int64 (uint16 tensors support few operations)."""
    return qmap.view(torch.int16).to(torch.int64) & 0xffff


def check_q_thresholds(fn, thr, nc, q_one, clause):
    """-> the thresholds as a list of nc ints in [0, q_one]; ``clause`` says what a threshold decides."""
    try:
        t = [int(v) for v in (thr.tolist() if isinstance(thr, torch.Tensor) else thr)]
    except (TypeError, ValueError):
        raise RuntimeError(f"mdil {fn}: thr must be {nc} integers, got {thr!r}") from None
    if len(t) != nc or any(v < 0 or v > q_one for v in t):
        raise RuntimeError(f"mdil {fn}: thr must be {nc} integers in [0, {q_one}] ({clause}), got {t}")
    return t


def device_ints(fn, path, values, name, nc, dev, lo, hi):
    """nc ints in [lo, hi] or an int32 [nc] device tensor (taken as it is) -> the device tensor."""
    if isinstance(values, torch.Tensor) and values.is_cuda:
        check_tables(fn, path, dev, torch.int32, ((values, name, (nc,)),))
        return values
    try:
        v = [int(t) for t in (values.tolist() if isinstance(values, torch.Tensor) else values)]
    except (TypeError, ValueError):
        raise RuntimeError(f"mdil {fn}: {name} must be {nc} integers, got {values!r}") from None
    if len(v) != nc or any(t < lo or t > hi for t in v):
        raise RuntimeError(f"mdil {fn}: {name} must be {nc} integers in [{lo}, {hi}], got {v}")
    return torch.tensor(v, dtype=torch.int32).to(dev)


def zero_counters(shapes, dev, names=None):
    """{name: zeroed int64 tensor of ``shapes[name]`` on ``dev``} over ``names`` (default: every shape)."""
    return {k: torch.zeros(shapes[k], dtype=torch.int64, device=dev) for k in (shapes if names is None else names)}


# -------------------------------------------------------------------------------- command lines
class RefusingParser(ArgumentParser):
    """An ArgumentParser whose ``parse_args`` also runs ``refusals(args)`` and reports its
    RuntimeError as a usage error."""

    def __init__(self, refusals, **kw):
        super().__init__(**kw)
        self.refusals = refusals

    def parse_args(self, *a, **kw):
        args = super().parse_args(*a, **kw)
        try:
            self.refusals(args)
        except RuntimeError as e:
            self.error(str(e))
        return args


def load_model(state, num_classes, task):
    """-> (device, class count of ``task``, Net_RAP(num_classes) with the checkpoint ``state`` loaded, in eval mode)."""
    from .models.erfnet_RA_parallel import Net as Net_RAP
    from .trainer_common import _strip
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    nb = len(num_classes)
    if not 0 <= task < nb:
        raise RuntimeError(f"--task {task}: the model has tasks 0 to {nb - 1}")
    model = Net_RAP(num_classes, nb, nb - 1)
    saved = torch.load(state, map_location="cpu", weights_only=False)
    model.load_state_dict(_strip(saved["state_dict"]), strict=True)
    model.to(dev).eval()
    return dev, num_classes[task], model


def image_batch(arrays, dev):
    """uint8 [h,w,3] arrays -> f32 [n,3,h,w] in [0, 1] on the device (the bytes cross the bus)."""
    u8 = torch.from_numpy(np.stack(arrays)).to(dev)
    return u8.permute(0, 3, 1, 2).to(torch.float32).div_(255.0)


def image_batches(args, pool, dev):
    """The images under ``--images`` (predict.py's reader: sorted, unique stems, resized to ``--height`` x
    ``--width`` on ``pool``) -> (stems, images f32 [n,3,H,W] on the device) per batch of ``--batch-size``."""
    from . import predict as P
    files, stems = P._image_files(args.images)
    for i in range(0, len(files), args.batch_size):
        arrs = list(pool.map(lambda f: P._load_resized(f, args.height, args.width), files[i:i + args.batch_size]))
        yield stems[i:i + args.batch_size], image_batch(arrs, dev)


def _save_png(arr, path):
    from PIL import Image
    Image.fromarray(arr).save(path)


def png_pool():
    return ThreadPoolExecutor(max_workers=min(MAX_PNG_THREADS, os.cpu_count() or 1))


class PngWriter:
    """Writes maps on ``pool`` with a bound on what is in flight: ``wait()`` before submitting a
    batch, so that at most the batch before it is still being written.  ``written``: every path."""

    def __init__(self, pool, out):
        self.pool, self.out, self.written, self.pending = pool, out, [], []

    def wait(self):
        for f in self.pending:
            f.result()
        self.pending = []

    def submit(self, arr, name):
        path = os.path.join(self.out, name)
        self.pending.append(self.pool.submit(_save_png, np.ascontiguousarray(arr), path))
        self.written.append(path)


def score_report(report, meter, args, how=""):
    """Adds the meter's score to ``report`` and prints it; then the maps line and the JSON file."""
    if meter is not None:
        matrix = meter.matrix()
        miou, per_class = meter.iou(matrix)
        report.update(mIoU=float(miou), iou_classes=[float(v) for v in per_class], confusion=matrix.tolist(),
                      pixels=int(matrix.sum()))
        print(f"{report['dataset']} (task {args.task}) at the labels' own size{how}: "
              f"mIoU {float(miou) * 100:.2f} %  over {report['pixels']} pixels")
        print("per-class IoU: " + " ".join(f"{float(v) * 100:.2f}" for v in per_class))
    if args.out:
        print(f"{len(report['written'])} maps written to {args.out}")
    if args.json:
        write_json(report, args.json)
    return report


def write_json(report, path):
    with open(path, "w") as f:
        json.dump(report, f, indent=1)
