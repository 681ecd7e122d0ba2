"""Latent-space plots on MI355X -- what the reference's ``Plot_Tsne_Notebook.ipynb`` does with a CPU
t-SNE: the encoder output, the decoder's 16-channel penultimate features or the logits of one
validation image, every position paired with its nearest-resized ground-truth label, embedded in
two dimensions by an EXACT t-SNE that runs on the device (include/mdil_tsne.h: squared distances,
sklearn's perplexity search, the gradient descent on the KL divergence) and scattered in the
dataset's colours.

    python -m mdil_ss_amd.latent --state model_best_....pth.tar --num-classes 20 20 --task 0 \
        (--dataset cityscapes|bdd|idd --datadir DIR --index K | --image PNG --label PNG | --synthetic 1) \
        --layer encoder|penultimate|logits [--points 20000] [--perplexity 100] [--iterations 2000] \
        [--seed 2] --out DIR [--height 512 --width 1024] [--classes-at-least K]

writes ``<stem>_<layer>_tsne.npz`` (``Y``, ``labels``, ``kl_log``, the arguments) and
``<stem>_<layer>_tsne.png`` and prints the final KL divergence.  Activations are NHWC, so the
features of one image ARE the row-major point matrix: nothing is moved before the distances."""
import io
import json
import os
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

from . import _head_common as hc
from . import _tsne_lib
from .predict import default_palette

LAYERS = ("encoder", "penultimate", "logits")
_STRIDE = {"encoder": 8, "penultimate": 2, "logits": 1}        # input pixels per position
_PATH = "latent-space"
MAX_POINTS, MAX_DIM = _tsne_lib.MAX_POINTS, _tsne_lib.MAX_DIM


# ---------------------------------------------------------------------------------- the latents
def latents(model, images, task, layer):
    """The NHWC activations of ``images`` [N,3,H,W] for ``task`` at ``layer``: "encoder"
    [N,H/8,W/8,128], "penultimate" [N,H/2,W/2,16] (what ``Net.features`` gives) or "logits"
    [N,H,W,nc]; contiguous, so ``.view(-1, C)`` is the point matrix.  Runs the model's own
    ``plan`` one step at a time in eval mode (``models.erfnet_RA_parallel.Net``)."""
    if layer not in LAYERS:
        raise RuntimeError(f"mdil latents: layer must be one of {LAYERS}, got {layer!r}")
    if not isinstance(images, torch.Tensor) or not images.is_cuda:
        raise RuntimeError("mdil_ss_amd.latent runs on MI355X only (input must be a cuda tensor); "
                           "there is no CPU fallback in the product path")
    from . import ops
    model.eval()
    with torch.no_grad():
        x = ops.to_nhwc(images)
        steps = model.plan(task, None, head=(layer == "logits"))
        # step 0 is the initial block, steps 1 .. len(encoder.layers) the encoder's layers
        stop = len(model.encoder.layers) + 1 if layer == "encoder" else len(steps)
        for f in steps[:stop]:
            x = f(x)
        return x.contiguous()


def resize_labels(labels, h, w):
    """``Resize([h, w], NEAREST)`` of a label tensor [..., H, W]: source index floor(i * H / h)."""
    lab = labels if isinstance(labels, torch.Tensor) else torch.as_tensor(labels)
    lead = lab.shape[:-2]
    out = F.interpolate(lab.reshape(1, -1, *lab.shape[-2:]).to(torch.float32), size=(int(h), int(w)), mode="nearest")
    return out.reshape(*lead, int(h), int(w)).to(lab.dtype)


def sample_points(n, points, seed):
    """Indices of the points that are embedded: all ``n`` in order when ``points >= n``, else the
    notebook's draw ``RandomState(seed).choice(arange(n), points, replace=False)``."""
    n, points = int(n), int(points)
    if points < 2:
        raise RuntimeError(f"mdil sample_points: {points} points (at least 2)")
    if min(n, points) > MAX_POINTS:
        raise RuntimeError(f"mdil sample_points: {min(n, points)} points (supported: up to {MAX_POINTS}); "
                           "ask for fewer with points=")
    if points >= n:
        return np.arange(n)
    return np.random.RandomState(seed).choice(np.arange(n), points, replace=False)


# -------------------------------------------------------------------------------- entry points
def _chk(fn, t, name, dtype=torch.float32):
    hc.chk(fn, _PATH, t, name, dtype)


def _tensor(fn, t, name, dtype=torch.float32):
    """Refuses what is no tensor at all; sizes are judged next, dtype / layout / device after them."""
    if not isinstance(t, torch.Tensor):
        _chk(fn, t, name, dtype)


def _check_n(fn, N):
    if not 2 <= N <= MAX_POINTS:
        raise RuntimeError(f"mdil {fn}: {N} points (supported: 2 to {MAX_POINTS})")


def _check_square(fn, t, name, N=None):
    if t.dim() != 2 or t.shape[0] != t.shape[1] or (N is not None and t.shape[0] != N):
        want = "[N,N]" if N is None else f"[{N},{N}]"
        raise RuntimeError(f"mdil {fn}: {name} must be float32 {want} (got {tuple(t.shape)})")


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def workspace(N, device):
    """The scratch buffer ``affinities`` and ``run`` need for N points (either, one at a time)."""
    _check_n("tsne_workspace", N)
    return torch.empty(_tsne_lib.load().mdil_tsne_workspace_bytes(N), dtype=torch.uint8, device=device)


def _check_workspace(fn, ws, ref):
    N = ref.shape[0]
    if ws is None:
        return workspace(N, ref.device)
    _chk(fn, ws, "workspace", torch.uint8)
    need = _tsne_lib.load().mdil_tsne_workspace_bytes(N)
    if ws.numel() < need or ws.device != ref.device:
        raise RuntimeError(f"mdil {fn}: workspace must hold {need} bytes on {ref.device} "
                           f"(got {ws.numel()} on {ws.device})")
    return ws


def sqdist(points):
    """f32 [N,d] -> f32 [N,N], D[i][j] = sum_k (x_ik - x_jk)^2 from the differences: the diagonal
    is exactly 0 and D equals its transpose bit for bit."""
    fn = "tsne_sqdist"
    lib = _tsne_lib.load()
    _tensor(fn, points, "points")
    if points.dim() != 2:
        raise RuntimeError(f"mdil {fn}: points must be float32 [N,d] (got {tuple(points.shape)})")
    N, d = points.shape
    _check_n(fn, N)
    if not 1 <= d <= MAX_DIM:
        raise RuntimeError(f"mdil {fn}: {d} dimensions (supported: 1 to {MAX_DIM})")
    _chk(fn, points, "points")
    with torch.no_grad(), torch.cuda.device(points.device):
        D = torch.empty(N, N, dtype=torch.float32, device=points.device)
        _tsne_lib.check(lib.mdil_tsne_sqdist(points.data_ptr(), N, d, D.data_ptr(), _stream(points)),
                        "mdil_tsne_sqdist")
    return D


def affinities(D, perplexity, workspace=None):
    """sklearn's ``_joint_probabilities`` (exact method) on squared distances f32 [N,N].
    -> (P f32 [N,N], symmetric, zero diagonal, sum 1; the per-row betas f64 [N])."""
    fn = "tsne_affinities"
    lib = _tsne_lib.load()
    _tensor(fn, D, "D")
    _check_square(fn, D, "D")
    N = D.shape[0]
    _check_n(fn, N)
    perplexity = float(perplexity)
    if not 1.0 <= perplexity < N:
        raise RuntimeError(f"mdil {fn}: perplexity {perplexity:g} must be at least 1 and less than the {N} points")
    _chk(fn, D, "D")
    ws = _check_workspace(fn, workspace, D)
    with torch.no_grad(), torch.cuda.device(D.device):
        P = torch.empty(N, N, dtype=torch.float32, device=D.device)
        betas = torch.empty(N, dtype=torch.float64, device=D.device)
        _tsne_lib.check(lib.mdil_tsne_affinities(D.data_ptr(), N, perplexity, betas.data_ptr(), P.data_ptr(),
                                                 ws.data_ptr(), _stream(D)), "mdil_tsne_affinities")
    return P, betas


def run(P, Y, update, gains, iterations, *, first_iter=0, exaggeration_iters=250, exaggeration=12.0,
        learning_rate=200.0, kl_every=50, workspace=None):
    """Enqueues ``iterations`` steps of sklearn's ``_gradient_descent`` on the exact KL divergence;
    ``Y``, ``update`` and ``gains`` (f32 [N,2]) are advanced in place.  -> kl_log f32
    [iterations // kl_every, 2] on the device: (KL, gradient norm) of every ``kl_every``-th step."""
    fn = "tsne_run"
    lib = _tsne_lib.load()
    _tensor(fn, P, "P")
    _check_square(fn, P, "P")
    N = P.shape[0]
    _check_n(fn, N)
    _chk(fn, P, "P")
    for t, name in ((Y, "Y"), (update, "update"), (gains, "gains")):
        _chk(fn, t, name)
        if tuple(t.shape) != (N, 2) or t.device != P.device:
            raise RuntimeError(f"mdil {fn}: {name} must be float32 [{N},2] on {P.device} "
                               f"(got {tuple(t.shape)} on {t.device})")
    iterations, first_iter, kl_every = int(iterations), int(first_iter), int(kl_every)
    if iterations < 0 or first_iter < 0:
        raise RuntimeError(f"mdil {fn}: iterations {iterations} and first_iter {first_iter} must not be negative")
    if not (float(exaggeration) > 0 and float(learning_rate) > 0):
        raise RuntimeError(f"mdil {fn}: exaggeration {exaggeration} and learning_rate {learning_rate} must be positive")
    ws = _check_workspace(fn, workspace, P)
    with torch.no_grad(), torch.cuda.device(P.device):
        kl_log = torch.zeros(iterations // kl_every if kl_every > 0 else 0, 2, dtype=torch.float32, device=P.device)
        _tsne_lib.check(
            lib.mdil_tsne_run(P.data_ptr(), N, Y.data_ptr(), update.data_ptr(), gains.data_ptr(), iterations,
                              first_iter, int(exaggeration_iters), float(exaggeration), float(learning_rate),
                              kl_every, kl_log.data_ptr() if kl_log.numel() else None, ws.data_ptr(), _stream(P)),
            "mdil_tsne_run")
    return kl_log


def random_init(n, seed):
    """What sklearn's ``init="random"`` draws: 1e-4 * RandomState(seed).standard_normal((n, 2)), f32 (host)."""
    return torch.from_numpy((1e-4 * np.random.RandomState(seed).standard_normal((n, 2))).astype(np.float32))


def tsne(points, perplexity=100, iterations=2000, learning_rate=200.0, early_exaggeration=12.0,
         exaggeration_iters=250, seed=2, init=None, kl_every=50):
    """``TSNE(n_components=2, method="exact", init="random", random_state=seed)`` on device points
    f32 [N,d].  -> (Y f32 [N,2] on the device, kl_log f32 [iterations // kl_every, 2] on the device).
    ``learning_rate="auto"``: max(N / early_exaggeration / 4, 50).  No early stopping."""
    D = sqdist(points)
    N = D.shape[0]
    ws = workspace(N, D.device)
    P, _ = affinities(D, perplexity, ws)
    del D
    if isinstance(learning_rate, str):
        if learning_rate != "auto":
            raise RuntimeError(f"mdil tsne: learning_rate must be a number or 'auto', got {learning_rate!r}")
        learning_rate = max(N / float(early_exaggeration) / 4.0, 50.0)
    Y = (random_init(N, seed) if init is None else torch.as_tensor(init, dtype=torch.float32)).to(P.device)
    Y = Y.clone().contiguous()
    if tuple(Y.shape) != (N, 2):
        raise RuntimeError(f"mdil tsne: init must be [{N},2] (got {tuple(Y.shape)})")
    update, gains = torch.zeros_like(Y), torch.ones_like(Y)
    kl_log = run(P, Y, update, gains, iterations, exaggeration_iters=exaggeration_iters,
                 exaggeration=early_exaggeration, learning_rate=learning_rate, kl_every=kl_every, workspace=ws)
    return Y, kl_log


# ------------------------------------------------------------------------------------- the plot
def scatter_png(Y, labels, palette, path, size=1024, marker=5, skip=None):
    """Scatter of Y [N,2] in the colours ``palette[labels]`` on white, ``size`` x ``size`` pixels:
    the axes span the data's bounding box plus a 4 % margin, square markers of ``marker`` pixels,
    drawn in class-index order; classes in ``skip`` (default: the last, ignore, class) are left out.
    numpy + PIL only; the same inputs give the same bytes."""
    from PIL import Image
    Y = np.asarray(Y.detach().cpu() if isinstance(Y, torch.Tensor) else Y, dtype=np.float64)
    labels = np.asarray(labels.detach().cpu() if isinstance(labels, torch.Tensor) else labels).astype(np.int64)
    palette = np.asarray(palette.cpu() if isinstance(palette, torch.Tensor) else palette, dtype=np.uint8)
    if Y.ndim != 2 or Y.shape[1] != 2 or labels.shape != (Y.shape[0],):
        raise RuntimeError(f"mdil scatter_png: Y must be [N,2] and labels [N] (got {Y.shape}, {labels.shape})")
    skip = (len(palette) - 1,) if skip is None else tuple(skip)
    lo, hi = Y.min(0), Y.max(0)
    span = np.where(hi > lo, hi - lo, 1.0)
    lo, span = lo - 0.04 * span, 1.08 * span
    px = np.rint((Y[:, 0] - lo[0]) / span[0] * (size - 1)).astype(np.int64)
    py = (size - 1) - np.rint((Y[:, 1] - lo[1]) / span[1] * (size - 1)).astype(np.int64)
    canvas = np.full((size, size, 3), 255, dtype=np.uint8)
    offsets = np.arange(marker) - marker // 2
    for c in range(len(palette)):
        if c in skip:
            continue
        sel = labels == c
        for dy in offsets:
            for dx in offsets:
                canvas[np.clip(py[sel] + dy, 0, size - 1), np.clip(px[sel] + dx, 0, size - 1)] = palette[c]
    Image.fromarray(canvas).save(path)
    return path


def save_npz(path, **arrays):
    """``np.savez`` without the clock: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, arr in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


# ------------------------------------------------------------------------------------------ CLI
def _resized(image, label, height, width, nc):
    """The validation transform: PIL bilinear image / nearest label, 255 -> the ignore class."""
    from .dataset import MyCoTransform
    img, lab = MyCoTransform(False, height, width).resize_bytes(image.convert("RGB"), label)
    lab = lab.copy()
    lab[lab == 255] = nc - 1
    return img, lab


def _sample(args, nc, dev):
    """-> (stem, images f32 [1,3,h,w] on the device, label u8 [h,w] on the host)."""
    from PIL import Image
    need = args.classes_at_least
    if args.synthetic:
        from .dataset import ProceduralSeg
        ds = ProceduralSeg(max(args.synthetic, args.index + 1), args.height, args.width, nc, seed=12 + args.task,
                           domain=args.task)
        for i in range(args.index, len(ds)):
            img, lab = ds[i]
            if len(torch.unique(lab)) >= need:
                return f"synthetic_{i:04d}", img[None].to(dev), lab[0].to(torch.uint8)
        raise RuntimeError(f"no synthetic image from index {args.index} on has {need} distinct labels")
    if args.image:
        with Image.open(args.image) as im, Image.open(args.label) as lb:
            img, lab = _resized(im, lb.convert("P"), args.height, args.width, nc)
        return os.path.splitext(os.path.basename(args.image))[0], hc.image_batch([img], dev), torch.from_numpy(lab)
    from .dataset import _ALIASES, _CLASSES
    key = _ALIASES[{"cityscapes": "cityscapes", "bdd": "BDD", "idd": "IDD"}[args.dataset.lower()]]
    if not args.datadir or not os.path.isdir(args.datadir):
        raise RuntimeError(f"dataset root for {args.dataset} not found: {args.datadir} (set --datadir)")
    ds = _CLASSES[key](args.datadir, None, args.subset)
    for i in range(args.index, len(ds)):
        image, label = ds[i]
        img, lab = _resized(image, label, args.height, args.width, nc)
        if len(np.unique(lab)) >= need:
            stem = os.path.splitext(os.path.basename(ds.filenames[i]))[0]
            return stem, hc.image_batch([img], dev), torch.from_numpy(lab)
    raise RuntimeError(f"no image of {args.dataset} from index {args.index} on has {need} distinct labels")


def positions(args):
    """How many positions ``--layer`` has at ``--height`` x ``--width``."""
    s = _STRIDE[args.layer]
    return (args.height // s) * (args.width // s)


def main(args):
    _refusals(args)
    dev, nc, model = hc.load_model(args.state, args.num_classes, args.task)
    stem, images, label = _sample(args, nc, dev)
    feat = latents(model, images, args.task, args.layer)
    h, w, C = feat.shape[1:]
    labels = label if args.layer == "logits" else resize_labels(label, h, w)
    idx = sample_points(h * w, args.points, args.seed)
    points = feat.view(-1, C)[torch.from_numpy(idx).to(dev)].contiguous()
    labels = labels.reshape(-1).numpy()[idx]
    Y, kl_log = tsne(points, perplexity=args.perplexity, iterations=args.iterations, learning_rate=args.learning_rate,
                     seed=args.seed, kl_every=args.kl_every)
    Y, kl_log = Y.cpu().numpy(), kl_log.cpu().numpy()
    os.makedirs(args.out, exist_ok=True)
    base = os.path.join(args.out, f"{stem}_{args.layer}_tsne")
    arguments = {k: v for k, v in sorted(vars(args).items()) if k not in ("out", "state", "datadir")}
    save_npz(base + ".npz", Y=Y, labels=labels.astype(np.uint8), kl_log=kl_log, index=idx.astype(np.int64),
             arguments=np.array(json.dumps(arguments)))
    scatter_png(Y, labels, default_palette(nc), base + ".png", skip=(nc - 1,))
    final = f"final KL divergence {kl_log[-1, 0]:.4f} after {args.iterations} iterations" if len(kl_log) else \
        f"{args.iterations} iterations (no KL logged: --kl-every {args.kl_every})"
    print(f"{stem} ({args.layer}, task {args.task}): {len(idx)} points of {C} dimensions, perplexity "
          f"{args.perplexity:g}: {final}")
    print(f"written: {base}.npz {base}.png")
    return {"stem": stem, "points": len(idx), "kl_log": kl_log.tolist(), "written": [base + ".npz", base + ".png"]}


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused."""
    sources = [bool(args.dataset), bool(args.image), bool(args.synthetic)]
    if sum(sources) != 1:
        raise RuntimeError("give exactly one of --dataset NAME --datadir DIR, --image PNG --label PNG, --synthetic 1")
    if bool(args.image) != bool(args.label):
        raise RuntimeError("--image and --label go together")
    if args.dataset and not args.datadir:
        raise RuntimeError("--dataset needs --datadir DIR")
    if min(args.height, args.width) < 8 or args.height % 8 or args.width % 8:
        raise RuntimeError("--height and --width must be positive multiples of 8")
    if args.index < 0 or args.iterations < 1 or args.kl_every < 1 or args.classes_at_least < 0:
        raise RuntimeError("--index and --classes-at-least must not be negative; --iterations and --kl-every at least 1")
    n = min(positions(args), args.points)
    if args.points < 2:
        raise RuntimeError("--points must be at least 2")
    if n > MAX_POINTS:
        raise RuntimeError(f"{n} points: an exact t-SNE here takes up to {MAX_POINTS}; lower --points")
    if not 1 <= args.perplexity < n:
        raise RuntimeError(f"--perplexity {args.perplexity:g} must be at least 1 and less than the {n} points")


def _rate(text):
    return text if text == "auto" else float(text)


def build_parser():
    p = hc.RefusingParser(_refusals, description="t-SNE plots of a model's latent spaces for one image")
    p.add_argument("--state", required=True, help="checkpoint written by the trainers (or by the reference)")
    p.add_argument("--num-classes", type=int, nargs="+", required=True)
    p.add_argument("--task", type=int, required=True, help="which task's adapters and decoder run")
    p.add_argument("--dataset", choices=("cityscapes", "bdd", "idd"), type=str.lower)
    p.add_argument("--datadir", help="--dataset: its root folder")
    p.add_argument("--subset", default="val")
    p.add_argument("--index", type=int, default=0, help="which image of the dataset (or the first one tried)")
    p.add_argument("--classes-at-least", type=int, default=0,
                   help="skip to the first image with at least this many distinct labels")
    p.add_argument("--image", help="one image file instead of a dataset")
    p.add_argument("--label", help="--image: its train-id label PNG")
    p.add_argument("--synthetic", type=int, default=0, help="procedural images instead of a dataset")
    p.add_argument("--layer", choices=LAYERS, required=True)
    p.add_argument("--points", type=int, default=20000, help="positions embedded (drawn without replacement)")
    p.add_argument("--perplexity", type=float, default=100.0)
    p.add_argument("--iterations", type=int, default=2000)
    p.add_argument("--learning-rate", type=_rate, default=200.0, help="a number or 'auto'")
    p.add_argument("--kl-every", type=int, default=50)
    p.add_argument("--seed", type=int, default=2)
    p.add_argument("--height", type=int, default=512, help="the network's input height")
    p.add_argument("--width", type=int, default=1024, help="the network's input width")
    p.add_argument("--out", required=True, help="folder for <stem>_<layer>_tsne.npz and .png")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
