"""Segmentation maps from a checkpoint on MI355X -- what the reference's notebooks do by hand
(``model(images, task).max(1)`` on the host, then ``Colorize``) as one fused kernel and a script:
``output_conv`` + argmax (+ palette lookup, + softmax confidence of the winner) straight from the
decoder's 16-channel features, so the logits are never stored (include/mdil_predict.h).

    python -m mdil_ss_amd.predict --state model_best_....pth.tar --num-classes 20 20 27 --task 1 \
        --images DIR --out DIR [--colour] [--confidence] [--palette FILE.json]

writes ``<stem>_label.png`` (8-bit train ids) and, on request, ``<stem>_colour.png`` (RGB) and
``<stem>_conf.png`` (``round(255 p)`` of the winning class).  ``--synthetic N`` predicts on the
procedural dataset instead of a folder."""
import functools
import json
import os
from argparse import ArgumentParser

import numpy as np
import torch

from . import _head_common as hc
from . import _predict_lib
from ._head_common import MAX_PNG_THREADS, _save_png  # noqa: F401  (imported from here by users)
from .transform import colormap, colormap_cityscapes

_FN, _PATH = "predict_head", "prediction"
_chk = functools.partial(hc.chk, _FN, _PATH)


def default_palette(nc):
    """uint8 [nc, 3] (host).  20 classes: the Cityscapes train-id colours with the ignore class
    (19) black; any other count: the PASCAL-VOC bit-interleaved colour map."""
    if nc == 20:
        cmap = np.zeros((20, 3), dtype=np.uint8)
        cmap[:19] = colormap_cityscapes(19)
    else:
        cmap = colormap(nc)
    return torch.from_numpy(np.ascontiguousarray(cmap))


def predict_head(features, weight, bias, palette=None, want_confidence=False):
    """``output_conv`` + argmax on NHWC decoder features [N,H,W,16] and the
    ``ConvTranspose2d(16, nc, 2, 2)`` parameters, 2 <= nc <= 32, on the current stream.
    -> (label u8 [N,2H,2W], colour u8 [N,2H,2W,3] or None, confidence f32 [N,2H,2W] or None);
    the colour map is written when a ``palette`` (u8 [nc,3], device) is given."""
    lib = _predict_lib.load()
    _chk(features, "features")
    _chk(weight, "weight")
    _chk(bias, "bias")
    x, w, b = features, weight, bias
    nc = hc.check_params(_FN, w, b, x)
    N, H, W = x.shape[0], x.shape[1], x.shape[2]
    hc.check_classes(_FN, _predict_lib, nc, x, w, b)
    hc.check_tables(_FN, _PATH, x.device, torch.uint8, ((palette, "palette", (nc, 3)),))
    with torch.no_grad(), torch.cuda.device(x.device):
        label = torch.empty(N, 2 * H, 2 * W, dtype=torch.uint8, device=x.device)
        colour = None if palette is None else torch.empty(N, 2 * H, 2 * W, 3, dtype=torch.uint8, device=x.device)
        conf = torch.empty(N, 2 * H, 2 * W, dtype=torch.float32, device=x.device) if want_confidence else None
        _predict_lib.check(
            lib.mdil_predict_head(x.data_ptr(), w.data_ptr(), b.data_ptr(), N, H, W, nc, hc.ptr(palette),
                                  label.data_ptr(), hc.ptr(colour), hc.ptr(conf),
                                  torch.cuda.current_stream(x.device).cuda_stream),
            "mdil_predict_head")
    return label, colour, conf


def predict(model, images, task, palette=None, want_confidence=False):
    """Label (and colour / confidence) maps of ``images`` [N,3,H,W] for ``task``: the model's
    decoder features, then ``predict_head`` with that task's ``output_conv`` parameters."""
    model.eval()
    with torch.no_grad():
        feat = model.features(images, task)
        w, b = model.head_params(task)
        return predict_head(feat.contiguous(), w.detach(), b.detach(), palette, want_confidence)


# ------------------------------------------------------------------------------------------ CLI
def _image_files(root):
    from .dataset import is_image
    files = sorted(os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs if is_image(f))
    if not files:
        raise RuntimeError(f"no .jpg / .png images under {root}")
    stems = [os.path.splitext(os.path.basename(f))[0] for f in files]
    if len(set(stems)) != len(stems):
        dup = sorted(s for s in set(stems) if stems.count(s) > 1)
        raise RuntimeError(f"image names under {root} are not unique (e.g. {dup[0]}): the outputs would collide")
    return files, stems


def _load_resized(path, height, width):
    """The validation transform's image half: PIL bilinear resize -> uint8 [H,W,3]."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB").resize((width, height), Image.BILINEAR), dtype=np.uint8)


def _batches(args, nc, pool, dev):
    """-> (stems, images f32 [n,3,H,W] on the device) per batch.  Not _report_common's feeder: this command
    line has no dataset and no targets, and its procedural images come without their labels."""
    bs = args.batch_size
    if args.synthetic:
        from .dataset import ProceduralSeg
        ds = ProceduralSeg(args.synthetic, args.height, args.width, nc, seed=12 + args.task, domain=args.task)
        for i in range(0, len(ds), bs):
            idx = range(i, min(i + bs, len(ds)))
            yield [f"synthetic_{j:04d}" for j in idx], torch.stack([ds[j][0] for j in idx]).to(dev)
        return
    yield from hc.image_batches(args, pool, dev)


def main(args):
    dev, nc, model = hc.load_model(args.state, args.num_classes, args.task)
    palette = None
    if args.colour:
        if args.palette:
            with open(args.palette) as f:
                palette = torch.tensor(json.load(f), dtype=torch.uint8)
            if tuple(palette.shape) != (nc, 3):
                raise RuntimeError(f"--palette {args.palette}: expected {nc} [r, g, b] rows, got {tuple(palette.shape)}")
        else:
            palette = default_palette(nc)
        palette = palette.contiguous().to(dev)
    os.makedirs(args.out, exist_ok=True)
    with hc.png_pool() as pool:
        png = hc.PngWriter(pool, args.out)
        for stems, images in _batches(args, nc, pool, dev):
            label, colour, conf = predict(model, images, args.task, palette, args.confidence)
            # one device-to-host copy per batch: every requested map as bytes, channels side by side
            planes = [label.unsqueeze(3)]
            if colour is not None:
                planes.append(colour)
            if conf is not None:
                planes.append(conf.mul(255.0).round_().nan_to_num_(0.0).clamp_(0.0, 255.0).to(torch.uint8).unsqueeze(3))
            host = (torch.cat(planes, 3) if len(planes) > 1 else planes[0]).cpu().numpy()
            png.wait()                         # the batch before this one: bounds what is in flight
            for k, stem in enumerate(stems):
                png.submit(host[k, :, :, 0], f"{stem}_label.png")
                c = 1
                if colour is not None:
                    png.submit(host[k, :, :, 1:4], f"{stem}_colour.png")
                    c = 4
                if conf is not None:
                    png.submit(host[k, :, :, c], f"{stem}_conf.png")
        png.wait()
    print(f"{len(png.written)} maps written to {args.out}")
    return png.written


def build_parser():
    p = ArgumentParser(description="label / colour / confidence maps from a checkpoint")
    p.add_argument("--state", required=True, help="checkpoint written by the trainers (or by the reference)")
    p.add_argument("--num-classes", type=int, nargs="+", required=True)
    p.add_argument("--task", type=int, required=True, help="which task's decoder predicts")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--images", help="folder of .jpg / .png images (searched recursively)")
    src.add_argument("--synthetic", type=int, default=0, help="predict on N procedural images instead")
    p.add_argument("--out", required=True, help="output folder")
    p.add_argument("--colour", action="store_true", help="also write <stem>_colour.png")
    p.add_argument("--confidence", action="store_true", help="also write <stem>_conf.png = round(255 p)")
    p.add_argument("--palette", help="JSON file: one [r, g, b] row per class (default: default_palette)")
    p.add_argument("--height", type=int, default=512)
    p.add_argument("--width", type=int, default=1024)
    p.add_argument("--batch-size", type=int, default=6)
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
