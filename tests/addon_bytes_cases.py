"""The cases of tests/test_addon_bytes_gpu.py: every output buffer of the three inference add-ons
(predict_head, fullres_head, ensemble_head) and every map, counter and fp64 sum of the two report
add-ons (drift_head, calib_head; of their meters the report) as a SHA-256, to be compared with the
digests recorded in tests/golden/addon_bytes.json.  Inputs come from a CPU ``torch.Generator`` with fixed seeds, so
they do not depend on the device; the kernels' arithmetic is deterministic (the confusion counts are
integer atomics), so the bytes are a property of the kernel sources alone.

    python tests/addon_bytes_cases.py FILE.json        # record (needs an MI355X)

The predict / fullres / ensemble entries were recorded from the kernel sources as they were BEFORE
those add-ons came to share mdil_ss_amd/ext/head_common.h.  The drift / calib entries were recorded
from the sources as they were BEFORE logits4, the wave tree, the fold kernel and the workspace
checks moved into that header and the drivers came to share mdil_ss_amd/_report_common.py; that
recording reproduced every earlier entry.  The file is the proof that sharing changed no byte and
is not re-recorded.  The report cases use public names only, so the file runs on both sides."""
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
BIG_DRIFT = (1, 513, 1023)
BIG_CALIB = ((1, 257, 511), (0.5, 1.0, 2.0))
SEVERAL, SEVERAL_NC = (3, 16, 48), 27                # 9 work-groups: the fold adds several rows
METER_NC = 20
CALIB_FULL = dict(temps=tuple(0.25 * 16 ** (i / 15) for i in range(16)), bins=15, class_temp=0)
CALIB_NARROW = dict(temps=(1.0,), bins=32, class_temp=None)


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


def _pair(nc, shape, seed):
    """Model A as ``_inputs`` gives it and model B, a perturbation of it: x + 0.1 x', w + 0.05 w'."""
    (x,), w, b, _, _, g = _inputs(nc, [shape], seed)
    xb = x + 0.1 * torch.randn(x.shape, generator=g)
    wb = w + 0.05 * torch.randn(w.shape, generator=g)
    return (x, w, b), (xb, wb, b), g


def _clean_target(nc, shape, g):
    """``_target`` without its out-of-range value: a meter's ``host()`` refuses one by design."""
    t = _target(nc, shape, g)
    t.view(-1)[t.numel() // 3] = 0
    return t


def _digests(out, counters):
    d = {k: _digest(v) for k, v in out.items()}
    d.update({k: _digest(v) for k, v in counters.items() if k != "workspace"})
    return d


def _text_digest(report):
    return hashlib.sha256(json.dumps(report, sort_keys=True).encode()).hexdigest()


def _drift(dev, nc, shape, seed, scored=True):
    from mdil_ss_amd.drift import drift_head, workspace_bytes
    a, b, g = _pair(nc, shape, seed)
    N, H, W = shape
    z = lambda *s: torch.zeros(*s, dtype=torch.int64, device=dev)                       # noqa: E731
    c = {"transition": z(nc, nc), "bad_targets": z(1), "sums": torch.zeros(nc + 1, dtype=torch.float64, device=dev),
         "workspace": torch.empty(workspace_bytes(N, H, W, nc) // 8, dtype=torch.float64, device=dev)}
    if scored:
        c.update(confusion_a=z(nc, nc), confusion_b=z(nc, nc), outcome=z(nc, 4))
    target = _target(nc, (N, 2 * H, 2 * W), g).to(dev) if scored else None
    out = drift_head(*(t.to(dev) for t in a + b), target=target, ignore_index=IGNORE, labels=True, kl=True,
                     change=True, counters=c)
    return _digests(out, c)


def _drift_meter(dev, nc, shapes, seed):
    from mdil_ss_amd.drift import DriftMeter
    meter = DriftMeter(nc, IGNORE)
    for i, shape in enumerate(shapes):
        a, b, g = _pair(nc, shape, seed + i)
        target = _clean_target(nc, (shape[0], 2 * shape[1], 2 * shape[2]), g).to(dev)
        meter.add(*(t.to(dev) for t in a + b), target=target)
    return {"report": _text_digest(meter.report())}


def _calib(dev, nc, shape, seed, temps, bins, class_temp):
    from mdil_ss_amd.calibrate import calib_head, workspace_bytes
    (x,), w, b, _, _, g = _inputs(nc, [shape], seed)
    N, H, W = shape
    K = len(temps)
    z = lambda *s: torch.zeros(*s, dtype=torch.int64, device=dev)                       # noqa: E731
    c = {"hist": z(K, bins, 3), "nonfinite": z(K), "bad_targets": z(1),
         "sums": torch.zeros(K, 3, dtype=torch.float64, device=dev),
         "workspace": torch.empty(workspace_bytes(N, H, W, nc, K) // 8, dtype=torch.float64, device=dev)}
    if class_temp is not None:
        c["class_hist"] = z(nc, bins, 3)
    target = _target(nc, (N, 2 * H, 2 * W), g).to(dev)
    out = calib_head(x.to(dev), w.to(dev), b.to(dev), target, temps, bins=bins, ignore_index=IGNORE,
                     class_temp=class_temp, label=True, maps=True, counters=c)
    return _digests(out, c)


def _calib_meter(dev, nc, shapes, seed):
    from mdil_ss_amd.calibrate import CalibrationMeter
    meter = CalibrationMeter(nc, CALIB_FULL["temps"], CALIB_FULL["bins"], IGNORE, CALIB_FULL["class_temp"])
    for i, shape in enumerate(shapes):
        (x,), w, b, _, _, g = _inputs(nc, [shape], seed + i)
        target = _clean_target(nc, (shape[0], 2 * shape[1], 2 * shape[2]), g).to(dev)
        meter.add(x.to(dev), w.to(dev), b.to(dev), target=target)
    return {"report": _text_digest(meter.report())}


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
    # the report add-ons: every map, every counter and the sums of drift_head and calib_head
    for nc in CLASSES:
        out[f"drift-nc{nc}"] = lambda dev, nc=nc: _drift(dev, nc, SMALL, 500 + nc)
        out[f"calib-full-nc{nc}"] = lambda dev, nc=nc: _calib(dev, nc, SMALL, 600 + nc, **CALIB_FULL)
        out[f"calib-narrow-nc{nc}"] = lambda dev, nc=nc: _calib(dev, nc, SMALL, 700 + nc, **CALIB_NARROW)
    out["drift-several"] = lambda dev: _drift(dev, SEVERAL_NC, SEVERAL, 540)
    out["drift-unscored"] = lambda dev: _drift(dev, 20, SMALL, 541, scored=False)
    out["calib-full-several"] = lambda dev: _calib(dev, SEVERAL_NC, SEVERAL, 640, **CALIB_FULL)
    out["calib-narrow-several"] = lambda dev: _calib(dev, SEVERAL_NC, SEVERAL, 740, **CALIB_NARROW)
    out["drift-grid"] = lambda dev: _drift(dev, 2, BIG_DRIFT, 404)
    out["calib-grid"] = lambda dev: _calib(dev, 2, BIG_CALIB[0], 405, temps=BIG_CALIB[1], bins=15, class_temp=1)
    out["drift-meter"] = lambda dev: _drift_meter(dev, METER_NC, [SMALL, SEVERAL], 550)
    out["calib-meter"] = lambda dev: _calib_meter(dev, METER_NC, [SMALL, SEVERAL], 650)
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
