"""Which head for an image of unknown domain, on MI355X.  The model is multi-domain -- one shared
ERFNet and, per domain, its own BatchNorm statistics, adapters and decoder head -- and every other
entry point takes ``--task T``.  This one chooses T per image (include/mdil_route.h):

    python -m mdil_ss_amd.route --state model_best_....pth.tar --num-classes 20 20 27 \
        --by stats|entropy|confidence|margin [--tasks 0 1 2] --images DIR --out DIR [--colour] --json FILE
    python -m mdil_ss_amd.route --state model_best_....pth.tar --num-classes 20 20 27 --by stats \
        --dataset BDD --subset val --task 1 --score --json FILE        # what does guessing the domain cost

``stats``: the image's own moments of the shared stem's 16 channels (``route_stem``: stem conv +
max-pool + per-image sums in one pass over the image, no network forward) against every domain's
``encoder.initial_block.bn_ini[t]`` running statistics, as the KL divergence of diagonal Gaussians;
only the chosen heads' forwards run.  ``entropy`` / ``confidence`` / ``margin``: one forward per
domain, and what that domain's head says about the image (``route_head``: ``output_conv`` +
softmax + per-image sums; the logits are never stored).  The lowest score wins; a head whose
softmax sum is not finite at any pixel of an image scores inf on that image and loses.

The second form takes a labelled set of domain ``--task T`` and reports where its images were sent,
the mIoU with head T on every image (the figure every other tool reports) and the mIoU under
routing.  How well either kind of route tells REAL domains apart is not measured here."""
import math
import os

import torch

from . import _head_common as hc
from . import _report_common as rc
from . import _route_lib

_PATH = "routing"
BY = ("stats", "entropy", "confidence", "margin")
HEAD_COLUMN = {"entropy": 0, "confidence": 1, "margin": 2}        # the columns of route_head's scores
STEM_CHANNELS = _route_lib.STEM_CHANNELS


# --------------------------------------------------------------------------------- entry points
def stem_workspace_bytes(N, Hi, Wi):
    need = _route_lib.load().mdil_route_stem_workspace_bytes(N, Hi, Wi)
    if need < 0:
        raise RuntimeError(f"mdil route_stem: no workspace for N {N}, image {Hi} x {Wi}")
    return need


def head_workspace_bytes(N, H, W, nc):
    need = _route_lib.load().mdil_route_head_workspace_bytes(N, H, W, nc)
    if need < 0:
        raise RuntimeError(f"mdil route_head: no workspace for N {N}, features {H} x {W}, {nc} classes")
    return need


def stem_moments(images, weight, bias, *, act=False, nonfinite=None):
    """The shared stem on planar images [N,3,Hi,Wi] (Hi, Wi even) with the ``Conv2d(3, 13, 3, 2, 1)``
    parameters, on the current stream -> (moments f64 [N,16,2]: per image and channel sum a and sum a^2,
    act f32 [N,Hi/2,Wi/2,16] or None).  ``nonfinite`` (int64 [N], device) gains one count per position
    with a non-finite activation."""
    fn = "route_stem"
    lib = _route_lib.load()
    for t, name in ((images, "images"), (weight, "weight"), (bias, "bias")):
        hc.chk(fn, _PATH, t, name)
    x, w, b = images, weight, bias
    if x.dim() != 4 or x.shape[1] != 3 or x.numel() == 0 or x.shape[2] % 2 or x.shape[3] % 2 or \
            tuple(w.shape) != (STEM_CHANNELS - 3, 3, 3, 3) or tuple(b.shape) != (STEM_CHANNELS - 3,):
        raise RuntimeError(f"mdil {fn}: expects planar images [N,3,Hi,Wi] of even size and Conv2d(3, 13, 3, 2, 1) "
                           f"parameters (got images {tuple(x.shape)}, w {tuple(w.shape)}, bias {tuple(b.shape)})")
    if w.device != x.device or b.device != x.device:
        raise RuntimeError(f"mdil {fn}: images on {x.device}, weight on {w.device}, bias on {b.device}")
    N, Hi, Wi = x.shape[0], x.shape[2], x.shape[3]
    hc.check_tables(fn, _PATH, x.device, torch.int64, ((nonfinite, "nonfinite", (N,)),))
    with torch.no_grad(), torch.cuda.device(x.device):
        moments = torch.empty(N, STEM_CHANNELS, 2, dtype=torch.float64, device=x.device)
        ws = torch.empty(stem_workspace_bytes(N, Hi, Wi) // 8, dtype=torch.float64, device=x.device)
        a = torch.empty(N, Hi // 2, Wi // 2, STEM_CHANNELS, dtype=torch.float32, device=x.device) if act else None
        _route_lib.check(
            lib.mdil_route_stem(x.data_ptr(), w.data_ptr(), b.data_ptr(), N, Hi, Wi, moments.data_ptr(), hc.ptr(a),
                                hc.ptr(nonfinite), ws.data_ptr(), ws.numel() * 8,
                                torch.cuda.current_stream(x.device).cuda_stream),
            "mdil_route_stem")
    return moments, a


def route_head(features, weight, bias, *, label=True, maps=False, scores=True, nonfinite=None):
    """``output_conv`` + softmax on NHWC decoder features [N,H,W,16] and the ``ConvTranspose2d(16, nc,
    2, 2)`` parameters, 2 <= nc <= 32, on the current stream -> dict: ``label`` u8 [N,2H,2W]; with
    ``maps`` ``conf``, ``ent`` and ``margin`` f32 [N,2H,2W]; ``scores`` f64 [N,3], per image the sums of
    ent, conf and margin over its pixels.  What was not asked for is None.  ``nonfinite`` (int64 [N],
    device) gains one count per pixel whose softmax sum is not finite; such a pixel enters no sum."""
    fn = "route_head"
    lib = _route_lib.load()
    for t, name in ((features, "features"), (weight, "weight"), (bias, "bias")):
        hc.chk(fn, _PATH, t, name)
    x, w, b = features, weight, bias
    nc = hc.check_params(fn, w, b, x)
    N, H, W = x.shape[0], x.shape[1], x.shape[2]
    hc.check_classes(fn, _route_lib, nc, x, w, b)
    hc.check_tables(fn, _PATH, x.device, torch.int64, ((nonfinite, "nonfinite", (N,)),))
    if not label and not maps and not scores and nonfinite is None:
        raise RuntimeError(f"mdil {fn}: nothing to do (no label, no maps, no scores, no nonfinite counter)")
    with torch.no_grad(), torch.cuda.device(x.device):
        new = lambda dtype: torch.empty(N, 2 * H, 2 * W, dtype=dtype, device=x.device)  # noqa: E731
        out = {"label": new(torch.uint8) if label else None}
        for k in ("conf", "ent", "margin"):
            out[k] = new(torch.float32) if maps else None
        out["scores"] = torch.empty(N, 3, dtype=torch.float64, device=x.device) if scores else None
        ws = torch.empty(head_workspace_bytes(N, H, W, nc) // 8, dtype=torch.float64, device=x.device) if scores else None
        _route_lib.check(
            lib.mdil_route_head(x.data_ptr(), w.data_ptr(), b.data_ptr(), N, H, W, nc, hc.ptr(out["label"]),
                                hc.ptr(out["conf"]), hc.ptr(out["ent"]), hc.ptr(out["margin"]), hc.ptr(out["scores"]),
                                hc.ptr(nonfinite), hc.ptr(ws), 0 if ws is None else ws.numel() * 8,
                                torch.cuda.current_stream(x.device).cuda_stream),
            "mdil_route_head")
    return out


# ------------------------------------------------------------------------------ host arithmetic
def check_tasks(tasks, nb):
    """-> the tasks as a list of distinct ints in [0, nb); None: all of them."""
    tasks = list(range(nb)) if tasks is None else [int(t) for t in tasks]
    if not tasks or len(set(tasks)) != len(tasks) or any(not 0 <= t < nb for t in tasks):
        raise RuntimeError(f"mdil routing: tasks must be distinct and within 0 to {nb - 1}, got {tasks}")
    return tasks


def domain_stats(model, tasks):
    """-> (mean f64 [T,16], var f64 [T,16], eps) from ``encoder.initial_block.bn_ini[t]`` of ``tasks``."""
    bns = model.encoder.initial_block.bn_ini
    tasks = check_tasks(tasks, len(bns))
    mean = torch.stack([bns[t].running_mean.detach().double() for t in tasks])
    var = torch.stack([bns[t].running_var.detach().double() for t in tasks])
    return mean, var, float(bns[tasks[0]].eps)


def stats_scores(moments, pixels, mean, var, eps):
    """The KL divergence of the image's channel Gaussians from each domain's, in fp64 torch.
    ``moments`` [N,16,2] (sum a, sum a^2 over ``pixels`` positions), ``mean`` / ``var`` [T,16] -> f64 [N,T]:
        mu = s1 / n,  var_img = s2 / n - mu^2
        score_t = sum_c 0.5 [ ln((v_tc + eps) / (var_img + eps)) + (var_img + eps + (mu - m_tc)^2) / (v_tc + eps) - 1 ]"""
    m = moments.double()
    mean, var = mean.double().to(m.device), var.double().to(m.device)
    n = float(pixels)
    mu = m[:, :, 0] / n
    vi = (m[:, :, 1] / n - mu * mu)[:, None, :] + eps                  # [N,1,16]
    vt = var[None] + eps                                               # [1,T,16]
    return (0.5 * (torch.log(vt / vi) + (vi + (mu[:, None, :] - mean[None]) ** 2) / vt - 1.0)).sum(2)


def head_scores(sums, pixels, nc, by, nonfinite=None):
    """``sums`` f64 [N,3] of ``route_head`` over ``pixels`` pixels of an image, a head of ``nc`` classes
    -> f64 [N], lower = the head is surer: ``entropy``: mean ent / ln(nc), so that a 20-class and a
    27-class head compare; ``confidence``: 1 - mean conf; ``margin``: 1 - mean margin.
    ``nonfinite``: int64 [N], THIS head's count of pixels that entered no sum.  An image with any such
    pixel scores inf with this head, so the head loses: a mean over fewer pixels is not a smaller entropy."""
    if by not in HEAD_COLUMN:
        raise RuntimeError(f"mdil routing: head scores are {sorted(HEAD_COLUMN)}, got {by!r}")
    mean = sums.double()[:, HEAD_COLUMN[by]] / float(pixels)
    score = mean / math.log(nc) if by == "entropy" else 1.0 - mean
    if nonfinite is not None:
        score = torch.where(nonfinite.to(score.device) > 0, torch.full_like(score, float("inf")), score)
    return score


def choose(scores):
    """``scores`` [N,T] -> int64 [N] (host): the position of the lowest score of each row; ties go to the
    lowest position, a non-finite score loses (a row of them gives 0)."""
    s = scores.detach().double().cpu()
    s = torch.where(torch.isfinite(s), s, torch.full_like(s, float("inf")))
    T = s.shape[1]
    first = torch.where(s == s.min(1, keepdim=True)[0], torch.arange(T)[None], torch.full((1, 1), T))
    return first.min(1)[0]


def routed_set(chosen, true_task, num_classes):
    """Which images enter the mIoU under routing.  ``chosen``: the task of every image -> (scored: list
    of bool, misrouted_unscored): an image sent to another head enters with that head's label map when
    that head has as many classes as head ``true_task``; otherwise it is left out and counted."""
    scored = [num_classes[t] == num_classes[true_task] for t in chosen]
    return scored, sum(1 for t, s in zip(chosen, scored) if t != true_task and not s)


def confusion(label, target, nc, ignore_index):
    """int64 [nc,nc] on the device (row = target) by ``bincount`` -- exact -- over the pixels whose
    target is below nc and not ``ignore_index``; -> (matrix, targets out of range)."""
    t, p = target.reshape(-1).long(), label.reshape(-1).long()
    counted = (t < nc) & (t != ignore_index) & (p < nc)
    bad = ((t >= nc) & (t != ignore_index)).sum()
    return torch.bincount(t[counted] * nc + p[counted], minlength=nc * nc).reshape(nc, nc), bad


class Router:
    """``Router(model, by, tasks)``: ``scores(images)`` f64 [N,T] (device), ``choose(images)`` the task of
    every image (list of ints), ``predict(images)`` -> (tasks, label maps u8 [N,Hi,Wi] of the routed heads),
    ``route(images)`` the same with the scores and the non-finite count.  Nothing of a call is kept."""

    def __init__(self, model, by="stats", tasks=None):
        if by not in BY:
            raise RuntimeError(f"mdil Router: by must be one of {list(BY)}, got {by!r}")
        self.model, self.by = model, by
        self.tasks = check_tasks(tasks, len(model.decoder))
        self.classes = [model.decoder[t].output_conv.weight.shape[1] for t in self.tasks]
        if by == "stats":
            self.stats = domain_stats(model, self.tasks)

    def _images(self, images):
        if not isinstance(images, torch.Tensor) or images.dim() != 4 or not images.is_cuda:
            raise RuntimeError("mdil Router: images must be a float32 [N,3,H,W] device tensor; there is no CPU fallback "
                               f"in the {_PATH} path")
        return images.contiguous()

    def _head(self, images, t, **kw):
        feat = self.model.features(images, t).contiguous()
        w, b = self.model.head_params(t)
        return route_head(feat, w.detach(), b.detach(), **kw)

    def head_labels(self, images, task):
        """The label map u8 [N,Hi,Wi] of ``task``'s head: one forward, ``predict_head``'s bits."""
        self.model.eval()
        with torch.no_grad():
            return self._head(self._images(images), task, scores=False)["label"]

    def _run(self, images, labels):
        """``images`` as ``_images`` gives them -> (scores [N,T], non-finite counts int64 [N,T] (stats: [N,1]),
        None or every task's label map [T][N,Hi,Wi] where the route made them)"""
        self.model.eval()
        N, pixels = images.shape[0], images.shape[2] * images.shape[3]
        with torch.no_grad():
            if self.by == "stats":
                nonf = torch.zeros(N, dtype=torch.int64, device=images.device)
                conv = self.model.encoder.initial_block.conv
                moments, _ = stem_moments(images, conv.weight.detach(), conv.bias.detach(), nonfinite=nonf)
                return stats_scores(moments, pixels // 4, *self.stats), nonf[:, None], None
            cols, counts, maps = [], [], []
            for t, nc in zip(self.tasks, self.classes):
                nonf = torch.zeros(N, dtype=torch.int64, device=images.device)       # per task: which head it was
                r = self._head(images, t, label=labels, nonfinite=nonf)
                cols.append(head_scores(r["scores"], pixels, nc, self.by, nonf))
                counts.append(nonf)
                maps.append(r["label"])
            return torch.stack(cols, 1), torch.stack(counts, 1), maps

    def scores(self, images):
        return self._run(self._images(images), False)[0]

    def choose(self, images):
        return [self.tasks[i] for i in choose(self.scores(images)).tolist()]

    def route(self, images):
        """-> dict: ``tasks`` (list of ints), ``label`` u8 [N,Hi,Wi] of the routed heads, ``scores`` f64 [N,T]
        (device), ``nonfinite`` (int: non-finite stem positions or, summed over the heads, softmax sums).
        The statistics route runs only the forwards of the tasks that were chosen; the head routes have
        every task's label map already."""
        images = self._images(images)
        scores, nonf, maps = self._run(images, True)
        pos = choose(scores)
        label = torch.empty(images.shape[0], images.shape[2], images.shape[3], dtype=torch.uint8, device=images.device)
        with torch.no_grad():
            for i in sorted(set(pos.tolist())):
                idx = (pos == i).nonzero()[:, 0].to(images.device)
                label[idx] = maps[i][idx] if maps is not None else \
                    self._head(images[idx], self.tasks[i], scores=False)["label"]
        return {"tasks": [self.tasks[i] for i in pos.tolist()], "label": label, "scores": scores,
                "nonfinite": int(nonf.sum().item())}

    def predict(self, images):
        r = self.route(images)
        return r["tasks"], r["label"]


# ------------------------------------------------------------------------------------------ CLI
def main(args):
    _refusals(args)
    from .fullres import iou_rule
    from .predict import default_palette
    dev, _, model = hc.load_model(args.state, args.num_classes, args.task if args.task is not None else 0)
    router = Router(model, args.by, args.tasks)
    palettes = {nc: default_palette(nc).to(dev) for nc in set(args.num_classes)} if args.colour else {}
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    T = args.task
    ncT = args.num_classes[T] if T is not None else None
    per_image, sent, nonfinite = [], {t: 0 for t in router.tasks}, 0
    if args.score:
        z = lambda: torch.zeros(ncT, ncT, dtype=torch.int64, device=dev)  # noqa: E731
        conf_T, conf_routed, bad = z(), z(), torch.zeros((), dtype=torch.int64, device=dev)
        unscored = 0
    with hc.png_pool() as pool:
        png = hc.PngWriter(pool, args.out)
        nc_data = None if args.images else args.num_classes[args.task]   # a dataset is read in --task's label space
        for stems, images, target in rc.image_or_dataset_batches(args, nc_data, pool, dev, args.score, bool(args.out)):
            routed = router.route(images)
            tasks, label, scores = routed["tasks"], routed["label"], routed["scores"].cpu().tolist()
            nonfinite += routed["nonfinite"]
            for s, t, row in zip(stems, tasks, scores):
                per_image.append({"image": s, "task": t, "scores": {str(k): v for k, v in zip(router.tasks, row)}})
                sent[t] += 1
            if args.score:
                own = router.head_labels(images, T)                                # head T on every image
                m, b = confusion(own, target, ncT, ncT - 1)
                conf_T += m
                bad += b
                keep, lost = routed_set(tasks, T, args.num_classes)
                unscored += lost
                if any(keep):
                    idx = torch.tensor([i for i, k in enumerate(keep) if k], device=dev)
                    conf_routed += confusion(label[idx], target[idx], ncT, ncT - 1)[0]
            if args.out:
                planes = [label.unsqueeze(3)]
                if args.colour:
                    colour = torch.empty(*label.shape, 3, dtype=torch.uint8, device=dev)
                    for i, t in enumerate(tasks):
                        pal = palettes[args.num_classes[t]]
                        colour[i] = pal[label[i].long().clamp(max=pal.shape[0] - 1)]
                    planes.append(colour)
                host = (torch.cat(planes, 3) if len(planes) > 1 else planes[0]).cpu().numpy()
                png.wait()                             # the batch before this one: bounds what is in flight
                for k, stem in enumerate(stems):
                    png.submit(host[k, :, :, 0], f"{stem}_label.png")
                    if args.colour:
                        png.submit(host[k, :, :, 1:4], f"{stem}_colour.png")
        png.wait()
    report = {"dataset": rc.source_name(args), "by": args.by,
              "tasks": router.tasks, "images": len(per_image), "routes": per_image,
              "sent": {str(t): n for t, n in sent.items()}, "nonfinite": nonfinite, "written": png.written}
    print(f"{report['dataset']}: {len(per_image)} images routed by {args.by}: " +
          ", ".join(f"{n} to task {t}" for t, n in sent.items()))
    if T is not None:
        report.update(task=T, routing_accuracy=sent.get(T, 0) / max(1, len(per_image)))
        print(f"routing accuracy (true task {T}): {report['routing_accuracy'] * 100:.2f} %")
    if args.score:
        if int(bad.item()):
            raise RuntimeError(f"mdil routing: {int(bad.item())} target pixels are outside [0, {ncT}) and are not the "
                               f"ignore index {ncT - 1}")
        for name, m in (("head", conf_T.cpu()), ("routed", conf_routed.cpu())):
            d = m.double()
            miou, per_class = iou_rule(ncT, ncT - 1, d.diagonal(), d.sum(0), d.sum(1))
            report.update({f"mIoU_{name}": float(miou), f"iou_classes_{name}": [float(v) for v in per_class],
                           f"confusion_{name}": m.tolist(), f"pixels_{name}": int(m.sum())})
        report["misrouted_unscored"] = unscored
        print(f"mIoU with head {T} on every image {report['mIoU_head'] * 100:.2f} %; under routing "
              f"{report['mIoU_routed'] * 100:.2f} % ({unscored} misrouted images went to a head with another class "
              "count and are left out of it)")
    if args.out:
        print(f"{len(png.written)} maps written to {args.out}")
    if args.json:
        hc.write_json(report, args.json)
    return report


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused."""
    if sum(bool(v) for v in (args.images, args.dataset, args.synthetic)) != 1:
        raise RuntimeError("give one source of images: --images DIR, --dataset cityscapes|BDD|IDD or --synthetic N")
    nb = len(args.num_classes)
    check_tasks(args.tasks, nb)
    if args.images and args.task is not None:
        raise RuntimeError("--task names the true domain of a labelled set; --images are of unknown domain")
    if not args.images:
        if args.task is None:
            raise RuntimeError("--dataset and --synthetic need --task T, the domain the images come from")
        rc.refuse_task(args.task, args.num_classes)
    if args.score and args.images:
        raise RuntimeError("--score needs labels: give --dataset or --synthetic with --task T")
    if args.score and args.tasks is not None and args.task not in args.tasks:
        raise RuntimeError(f"--score: the true task {args.task} is not among --tasks {args.tasks}")
    if not args.out and not args.json:
        raise RuntimeError("nothing to do: give --out DIR or --json FILE")
    if args.colour and not args.out:
        raise RuntimeError("--colour writes <stem>_colour.png: it needs --out DIR")
    if min(args.height, args.width, args.batch_size) < 1 or args.synthetic < 0:
        raise RuntimeError("sizes and --batch-size must be positive")
    if args.height % 2 or args.width % 2:
        raise RuntimeError(f"--height {args.height} --width {args.width}: the network's input size must be even")


def build_parser():
    p = hc.RefusingParser(_refusals, description="route images of unknown domain to a head: per image the score of "
                                                 "every task, the chosen task and its label map")
    p.add_argument("--state", required=True, help="checkpoint written by the trainers (or by the reference)")
    p.add_argument("--num-classes", type=int, nargs="+", required=True)
    p.add_argument("--by", choices=BY, default="stats",
                   help="stats: the stem's moments against each domain's BatchNorm statistics (no forward); entropy, "
                        "confidence, margin: what each domain's head says (one forward per task)")
    p.add_argument("--tasks", type=int, nargs="+", help="the tasks to choose among (default: all)")
    p.add_argument("--images", help="folder of .jpg / .png images of unknown domain (searched recursively)")
    rc.add_data_flags(p, dataset_help="a labelled dataset of domain --task instead: the report also holds the routing "
                                      "accuracy", synthetic_help="N procedural images of domain --task instead")
    p.add_argument("--task", type=int, help="with --dataset / --synthetic: the true domain")
    p.add_argument("--score", action="store_true",
                   help="with --dataset / --synthetic: the mIoU with head --task on every image and under routing")
    p.add_argument("--out", help="write <stem>_label.png here: 8-bit train ids of the routed head")
    p.add_argument("--colour", action="store_true", help="also write <stem>_colour.png")
    p.add_argument("--json", help="write the report here")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
