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


# ------------------------------------------------------------------------- the map add-ons
def _poison(x):
    """One NaN and one +inf feature, in two different pixels."""
    x = x.clone()
    x[0, 0, 1, 3] = float("nan")
    x[0, x.shape[1] - 1, x.shape[2] // 2, 7] = float("inf")
    return x


def _head_inputs(nc, shape, seed, poison):
    """``_inputs`` for one feature tensor, on the host, with the target of its label grid."""
    (x,), w, b, ids, _, g = _inputs(nc, [shape], seed)
    target = _target(nc, (shape[0], 2 * shape[1], 2 * shape[2]), g)
    return (_poison(x) if poison else x), w, b, ids, target, g


def _zeros(dev, *shape):
    return torch.zeros(*shape, dtype=torch.int64, device=dev)


def _prefixed(prefix, tensors):
    return {f"{prefix}_{k}": _digest(v) for k, v in tensors.items()}


def _pseudo(dev, nc, shape, seed, poison=False):
    from mdil_ss_amd import pseudo as P
    x, w, b, ids, target, g = _head_inputs(nc, shape, seed, poison)
    hist, nonfinite = _zeros(dev, nc, 256), _zeros(dev, 1)
    label, qconf = P.pseudo_head(x.to(dev), w.to(dev), b.to(dev), hist, nonfinite)
    sel = hist.cpu().argmax(1).tolist()                  # per class the fullest high byte
    hist2, bad_labels = _zeros(dev, nc, 256), _zeros(dev, 1)
    P.pseudo_refine(label, qconf, nc, sel, hist2, bad_labels)
    thr = torch.randint(0, P.Q_ONE + 1, (nc,), generator=g).tolist()
    counters = P.new_apply_counters(nc, dev)
    out = P.pseudo_apply(label, qconf, nc, thr, ids.to(dev), 255, target.to(dev), IGNORE, counters)
    d = {"label": _digest(label), "qconf": _digest(qconf), "hist": _digest(hist), "nonfinite": _digest(nonfinite),
         "hist2": _digest(hist2), "refine_bad_labels": _digest(bad_labels), "out": _digest(out)}
    d.update(_prefixed("apply", counters))
    return d


def _openset(dev, nc, shape, seed, poison=False):
    from mdil_ss_amd import openset as O
    x, w, b, ids, target, g = _head_inputs(nc, shape, seed, poison)
    lut = O.group_lut(unknown_ids=[1], ignore_ids=[IGNORE]).to(dev)
    target = target.to(dev)
    hist, nonfinite = _zeros(dev, len(O.KINDS), 2, O.CODES), _zeros(dev, 1)
    label, code = O.openset_head(x.to(dev), w.to(dev), b.to(dev), target, lut, kinds=O.KINDS, map_kind="entropy",
                                 hist=hist, nonfinite=nonfinite)
    thr = int(O.code_values(code).median())              # rejects about half of the pixels
    cdf = O.cdf_lut(hist[O.KINDS.index("entropy"), O.KNOWN].cpu()).to(dev)
    counters = O.new_apply_counters(nc, dev)
    out, score = O.openset_apply(label, code, nc, thr, ids.to(dev), 255, cdf, target, lut, counters)
    d = {"label": _digest(label), "code": _digest(code), "hist": _digest(hist), "nonfinite": _digest(nonfinite),
         "out": _digest(out), "score": _digest(score)}
    d.update(_prefixed("apply", counters))
    return d


def _audit(dev, nc, shape, seed, poison=False):
    from mdil_ss_amd import audit as A
    x, w, b, _, target, g = _head_inputs(nc, shape, seed, poison)
    x, w, b, target = (t.to(dev) for t in (x, w, b, target))
    N = shape[0]
    first = A.new_head_counters(nc, N, dev, ("count", "qsum", "bad_targets", "nonfinite"))
    A.audit_head(x, w, b, target, IGNORE, counters=first)
    thr = A.thresholds(first["count"].cpu(), first["qsum"].cpu())
    second = A.new_head_counters(nc, N, dev)
    qmap, suggest = A.audit_head(x, w, b, target, IGNORE, thr, A.GIVEN, 255, second, want_suggest=True)
    max_q = torch.randint(-1, A.Q_ONE, (nc,), generator=g).tolist()
    d = {"qmap": _digest(qmap), "suggest": _digest(suggest)}
    d.update(_prefixed("sweep1", first))
    d.update(_prefixed("sweep2", second))
    for mode in A.MODES:
        counters = A.new_apply_counters(nc, dev)
        out, mask = A.audit_apply(target, suggest, qmap, nc, max_q, mode, IGNORE, 255, 255, counters, want_mask=True)
        d.update({f"{mode}_out": _digest(out), f"{mode}_mask": _digest(mask)})
        d.update(_prefixed(mode, counters))
    return d


ACQUIRE_TILE = (4, 6)                                    # ragged on every shape here; a work-group spans several


def _acquire(dev, nc, shape, seed, poison=False):
    from mdil_ss_amd import acquire as Q
    x, w, b, _, target, g = _head_inputs(nc, shape, seed, poison)
    x, w, b, target = (t.to(dev) for t in (x, w, b, target))
    N, size = shape[0], (2 * shape[1], 2 * shape[2])
    d = {}
    for kind in Q.KINDS:
        tiles = Q.new_tiles(N, size, ACQUIRE_TILE, nc, dev)
        counters = {k: _zeros(dev, 1) for k in Q.HEAD_COUNTERS}
        label, qmap = Q.acquire_head(x, w, b, ACQUIRE_TILE, kind, target, IGNORE, tiles, counters, want_label=True,
                                     want_qmap=True)
        d.update({f"{kind}_label": _digest(label), f"{kind}_qmap": _digest(qmap), f"{kind}_tiles": _digest(tiles)})
        d.update(_prefixed(kind, counters))
    selected = (torch.rand((N,) + Q.tile_grid(size, ACQUIRE_TILE), generator=g) < 0.4).to(torch.uint8)
    previous, fill = (_target(nc, (N,) + size, g) for _ in range(2))
    counters = Q.new_apply_counters(nc, dev)
    out, mask = Q.acquire_apply(selected.to(dev), size, ACQUIRE_TILE, nc, target, previous.to(dev), fill.to(dev), IGNORE,
                                255, counters, want_mask=True)
    d.update({"out": _digest(out), "mask": _digest(mask)})
    d.update(_prefixed("apply", counters))
    return d


def _route(dev, nc, shape, seed, poison=False):
    from mdil_ss_amd import route as R
    x, w, b, _, _, _ = _head_inputs(nc, shape, seed, poison)
    nonfinite = _zeros(dev, shape[0])
    out = R.route_head(x.to(dev), w.to(dev), b.to(dev), label=True, maps=True, scores=True, nonfinite=nonfinite)
    d = {k: _digest(v) for k, v in out.items()}
    d["nonfinite"] = _digest(nonfinite)
    return d


def _stem(dev, shape, seed, poison=False):
    from mdil_ss_amd import route as R
    g = torch.Generator().manual_seed(seed)
    images = torch.rand(shape, generator=g)
    w = torch.randn(R.STEM_CHANNELS - 3, 3, 3, 3, generator=g) * 0.3
    b = torch.randn(R.STEM_CHANNELS - 3, generator=g) * 0.2
    if poison:
        images[0, 1, 2, 5] = float("nan")
        images[0, 2, shape[2] - 1, 0] = float("inf")
    nonfinite = _zeros(dev, shape[0])
    moments, act = R.stem_moments(images.to(dev), w.to(dev), b.to(dev), act=True, nonfinite=nonfinite)
    return {"moments": _digest(moments), "act": _digest(act), "nonfinite": _digest(nonfinite)}


MAP_GOLDEN = os.path.join(REPO, "tests", "golden", "map_addon_bytes.json")
# 513 x 1023 feature pixels: past 768 x 256 and 256 x 1024 of them, so every head's loop strides, and its
# 1026 x 2046 label grid is past the 512 x 256 x 8 pixels of the map kernels' grid
MAP_GRID = (1, 513, 1023)
STEM_SMALL, STEM_GRID = (1, 3, 18, 14), (1, 3, 514, 514)   # 257 x 257 positions: past 256 x 256 of one image


def map_cases():
    """{name: run(dev) -> {buffer: sha256}} of the map add-ons (pseudo, openset, audit, acquire, route): every
    output map and every counter of their eleven kernels, recorded in MAP_GOLDEN from the kernel sources as
    they were BEFORE these add-ons came to share mdil_ss_amd/ext/map_common.h."""
    out = {}
    runs = (("pseudo", _pseudo, 1000), ("openset", _openset, 1100), ("audit", _audit, 1200),
            ("acquire", _acquire, 1300), ("route", _route, 1400))
    for tag, run, seed in runs:
        for nc in CLASSES:
            out[f"{tag}-nc{nc}"] = lambda dev, run=run, nc=nc, seed=seed: run(dev, nc, SMALL, seed + nc)
        out[f"{tag}-several"] = lambda dev, run=run, seed=seed: run(dev, SEVERAL_NC, SEVERAL, seed + 40)
        out[f"{tag}-grid"] = lambda dev, run=run, seed=seed: run(dev, 2, MAP_GRID, seed + 50)
        out[f"{tag}-nonfinite"] = lambda dev, run=run, seed=seed: run(dev, 20, SMALL, seed + 60, poison=True)
    out["stem-small"] = lambda dev: _stem(dev, STEM_SMALL, 1500)
    out["stem-grid"] = lambda dev: _stem(dev, STEM_GRID, 1501)
    out["stem-nonfinite"] = lambda dev: _stem(dev, STEM_SMALL, 1502, poison=True)
    return out


def record(path, table=cases):
    sys.path.insert(0, REPO)
    import mdil_ss_amd  # noqa: F401
    assert torch.cuda.is_available(), "recording needs an MI355X"
    dev = torch.device("cuda", 0)
    digests = {name: run(dev) for name, run in table().items()}
    with open(path, "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} cases recorded in {path}")


if __name__ == "__main__":
    record(sys.argv[1], map_cases if sys.argv[2:] == ["map"] else cases)
