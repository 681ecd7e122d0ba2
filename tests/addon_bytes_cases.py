"""The cases of tests/test_addon_bytes_gpu.py: every output buffer of the three inference add-ons
(predict_head, fullres_head, ensemble_head) as a SHA-256, to be compared with the digests recorded
in tests/golden/addon_bytes.json.  Inputs come from a CPU ``torch.Generator`` with fixed seeds, so
they do not depend on the device; the kernels' arithmetic is deterministic (the confusion counts are
integer atomics), so the bytes are a property of the kernel sources alone.

    python tests/addon_bytes_cases.py FILE.json        # record (needs an MI355X)

The committed file was recorded from the kernel sources as they were BEFORE the add-ons came to
share mdil_ss_amd/ext/head_common.h; it is the proof that sharing changed no byte and is not
re-recorded."""
import hashlib
import json
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "addon_bytes.json")
CLASSES = (2, 20, 32)
IGNORE = 255
SMALL, SECOND = (1, 9, 7), (1, 12, 10)               # feature shapes (N, H, W)
PACKED, BYTES = (36, 28), (25, 31)                   # Wo a multiple of 4 / not
# the shapes of each library's test_grid_stride_loop_past_the_grid_bound
BIG_PREDICT = (1, 513, 1023)
BIG_FULLRES = ((1, 200, 300), (1025, 2051))
BIG_ENSEMBLE = ([(1, 200, 300), (1, 150, 225)], [0, 1], (1025, 2051))


def _inputs(nc, shapes, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(16, nc, 2, 2, generator=g)
    b = torch.randn(nc, generator=g) * 0.2
    xs = [F.relu(torch.randn(n, h, w_, 16, generator=g)) for n, h, w_ in shapes]      # NHWC
    ids = torch.randperm(256, generator=g)[:nc].to(torch.uint8)
    pal = torch.randint(0, 256, (nc, 3), generator=g, dtype=torch.uint8)
    return xs, w, b, ids, pal, g


def _target(nc, shape, g):
    """Train ids with about 1 in 8 pixels the ignore index and exactly one out-of-range value."""
    t = torch.randint(0, nc, shape, generator=g, dtype=torch.uint8)
    t[torch.rand(shape, generator=g) < 0.125] = IGNORE
    t.view(-1)[t.numel() // 3] = nc
    return t


def _digest(t):
    return None if t is None else hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()


def _predict(dev, nc, shape, seed):
    from mdil_ss_amd.predict import predict_head
    (x,), w, b, _, pal, _ = _inputs(nc, [shape], seed)
    label, colour, conf = predict_head(x.to(dev), w.to(dev), b.to(dev), pal.to(dev), True)
    return {"label": _digest(label), "colour": _digest(colour), "confidence": _digest(conf)}


def _scored(dev, nc, N, size, ids, pal, g):
    return dict(id_map=ids.to(dev), palette=pal.to(dev), target=_target(nc, (N,) + tuple(size), g).to(dev),
                ignore_index=IGNORE, confusion=torch.zeros(nc, nc, dtype=torch.int64, device=dev),
                bad_targets=torch.zeros(1, dtype=torch.int64, device=dev))


def _fullres(dev, nc, shape, size, seed):
    from mdil_ss_amd.fullres import fullres_head
    (x,), w, b, ids, pal, g = _inputs(nc, [shape], seed)
    kw = _scored(dev, nc, shape[0], size, ids, pal, g)
    label, colour = fullres_head(x.to(dev), w.to(dev), b.to(dev), size, **kw)
    return {"label": _digest(label), "colour": _digest(colour), "confusion": _digest(kw["confusion"]),
            "bad_targets": _digest(kw["bad_targets"])}


def _ensemble(dev, nc, shapes, flips, size, mode, seed):
    from mdil_ss_amd.ensemble import ensemble_head
    xs, w, b, ids, pal, g = _inputs(nc, shapes, seed)
    kw = _scored(dev, nc, shapes[0][0], size, ids, pal, g)
    views = [(x.to(dev), bool(f)) for x, f in zip(xs, flips)]
    label, colour, conf = ensemble_head(views, w.to(dev), b.to(dev), size, mode=mode, confidence=True, **kw)
    return {"label": _digest(label), "colour": _digest(colour), "confidence": _digest(conf),
            "confusion": _digest(kw["confusion"]), "bad_targets": _digest(kw["bad_targets"])}


def cases():
    """{name: run(dev) -> {buffer: sha256}}, in a fixed order."""
    out = {}
    for nc in CLASSES:
        out[f"predict-nc{nc}"] = lambda dev, nc=nc: _predict(dev, nc, SMALL, 100 + nc)
        for tag, size in (("packed", PACKED), ("bytes", BYTES)):
            out[f"fullres-{tag}-nc{nc}"] = lambda dev, nc=nc, size=size: _fullres(dev, nc, SMALL, size, 200 + nc)
        for mode in ("prob", "logit"):
            out[f"ensemble-{mode}-nc{nc}"] = lambda dev, nc=nc, mode=mode: _ensemble(
                dev, nc, [SMALL, SMALL, SECOND], [0, 1, 0], BYTES, mode, 300 + nc)
    out["predict-grid"] = lambda dev: _predict(dev, 2, BIG_PREDICT, 401)
    out["fullres-grid"] = lambda dev: _fullres(dev, 2, BIG_FULLRES[0], BIG_FULLRES[1], 402)
    for mode in ("prob", "logit"):
        out[f"ensemble-grid-{mode}"] = lambda dev, mode=mode: _ensemble(dev, 2, *BIG_ENSEMBLE, mode, 403)
    return out


def record(path):
    sys.path.insert(0, REPO)
    import mdil_ss_amd  # noqa: F401
    assert torch.cuda.is_available(), "recording needs an MI355X"
    dev = torch.device("cuda", 0)
    digests = {name: run(dev) for name, run in cases().items()}
    with open(path, "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} cases recorded in {path}")


if __name__ == "__main__":
    record(sys.argv[1])
