"""Label audit on MI355X: which labels of a dataset does the head confidently contradict?  Confident
learning (Northcutt, Jiang and Chuang, JAIR 2021) over a split, two sweeps of one fused kernel:

  sweep 1  per class, the number of pixels GIVEN that class and the sum of their self-confidence (the
           head's probability of the given class, 16 bits); the mean, rounded up, is the class's threshold;
  sweep 2  per pixel the SUGGESTED class: the most probable one among the classes at or above their own
           threshold (none, if no class is); every labelled pixel is counted under (given, suggested) --
           the confident joint -- and per image.  Its off-diagonal pixels are the label issues.

    python -m mdil_ss_amd.audit --state CKPT --num-classes 20 20 --task 1 --dataset BDD --subset val \
        --json FILE [--out DIR] [--top 20]
    python -m mdil_ss_amd.audit --state CKPT --num-classes 20 20 --task 1 --dataset BDD --subset val --fit THR.json
    python -m mdil_ss_amd.audit --state CKPT --num-classes 20 20 --task 1 --dataset BDD --subset train \
        --thresholds THR.json --json FILE --clean-root ROOT --layout BDD --mode prune --max-self-confidence 0.5

The report gives the thresholds, the confident joint, the joint calibrated to the class counts
(Northcutt's eq. 2-3), per class the estimated share of wrong given labels and of missed true labels,
the estimated number of label issues, the most confused (given -> suggested) pairs and the images with
the largest share of issues.  ``--out`` writes ``<stem>_issues.png`` (the suggested class's colour where
there is an issue, grey elsewhere); ``--clean-root`` writes a label tree, laid out as ``pseudo
--out-root`` lays it out, in which the issues are pruned (255) or relabelled.  ``audit_head`` never
stores the logits; everything after the 16-bit probabilities is integer arithmetic
(include/mdil_audit.h), so every counter is the same bytes on every run.

Two cautions.  Confident learning wants OUT-OF-SAMPLE probabilities: on a split the head was trained on
it undercounts the issues (the head has memorised part of the noise), and the class-weighted
cross-entropy the trainers use skews the self-confidences towards the rare classes, so fit and read the
thresholds per class and prefer a held-out split (``--fit`` on one split, ``--thresholds`` on another).
And, as with every add-on here, everything was measured on a randomly initialised network only: the
kernels' arithmetic and speed are tested, the usefulness of the issues on a trained head is not."""
import os

import torch

from . import _annotate_common as ac
from . import _audit_lib
from . import _head_common as hc
from . import _report_common as rc

_PATH = "label-audit"
Q_ONE = 65536                                   # q = min(65535, floor(p * Q_ONE)); thr = Q_ONE is never met
QMAP = torch.uint16
HEAD_COUNTERS = ("count", "qsum", "joint", "per_image", "bad_targets", "nonfinite")
APPLY_COUNTERS = ("seen", "acted", "bad_targets")
MODES = ("prune", "relabel")
GIVEN = "given"                                 # q_class: the q of the pixel's given class
GREY = 128


q_values = hc.q_values                          # a stored q map as int64
check_id = hc.check_id


def check_nc(fn, nc):
    return hc.check_nc(fn, _audit_lib, nc)


def check_thr(fn, thr, nc):
    """-> the thresholds as a list of nc ints in [0, 65536]."""
    return hc.check_q_thresholds(fn, thr, nc, Q_ONE, "class c is confident when q_c >= thr[c]")


def head_counter_shapes(nc, N):
    return {"count": (nc,), "qsum": (nc,), "joint": (nc, nc + 1), "per_image": (N, nc, 2), "bad_targets": (1,),
            "nonfinite": (1,)}


def new_head_counters(nc, N, dev, names=HEAD_COUNTERS):
    """The int64 counters of ``audit_head`` for ``nc`` classes and a batch of ``N`` images, zeroed, on ``dev``."""
    return hc.zero_counters(head_counter_shapes(nc, N), dev, names)


def apply_counter_shapes(nc):
    return {"seen": (nc,), "acted": (nc, nc), "bad_targets": (1,)}


def new_apply_counters(nc, dev):
    return hc.zero_counters(apply_counter_shapes(nc), dev)


# --------------------------------------------------------------------------------- entry points
def audit_head(features, weight, bias, target=None, ignore_index=-1, thr=None, q_class=None, none_id=255,
               counters=None, want_suggest=False):
    """``output_conv`` + the softmax as 16-bit q per class on NHWC decoder features [N,H,W,16] and the
    ``ConvTranspose2d(16, nc, 2, 2)`` parameters, 2 <= nc <= 32, on the current stream.
    -> (qmap u16 [N,2H,2W] of class ``q_class`` -- an int in [0, nc), or ``"given"`` for the pixel's
    given class -- or None, suggest u8 [N,2H,2W] or None without ``want_suggest``).  ``target``: u8
    [N,2H,2W] on the device; ``thr``: nc ints in [0, 65536] or an int32 [nc] device tensor (class c is
    confident when q_c >= thr[c]); ``counters``: any of ``HEAD_COUNTERS`` as int64 device tensors (the
    shapes of ``head_counter_shapes``), accumulated into, never cleared.  All but "nonfinite" need a
    target; ``want_suggest``, "joint" and "per_image" need ``thr``."""
    fn = "audit_head"
    lib = _audit_lib.load()
    for t, name in ((features, "features"), (weight, "weight"), (bias, "bias")):
        hc.chk(fn, _PATH, t, name)
    x, w, b = features, weight, bias
    nc = hc.check_params(fn, w, b, x)
    N, H, W = x.shape[0], x.shape[1], x.shape[2]
    hc.check_classes(fn, _audit_lib, nc, x, w, b)
    hc.check_ignore_index(fn, ignore_index)
    none_id = check_id(fn, "none_id", none_id)
    dev = x.device
    hc.check_tables(fn, _PATH, dev, torch.uint8, ((target, "target", (N, 2 * H, 2 * W)),))
    c = rc.check_counters(fn, counters, HEAD_COUNTERS)
    shapes = head_counter_shapes(nc, N)
    hc.check_tables(fn, _PATH, dev, torch.int64, tuple((c[k], k, shapes[k]) for k in HEAD_COUNTERS))
    if target is None and any(c[k] is not None for k in HEAD_COUNTERS if k != "nonfinite"):
        raise RuntimeError(f"mdil {fn}: the counters count, qsum, joint, per_image and bad_targets need a target "
                           "(uint8 [N,2H,2W]) on the device")
    if thr is None and (want_suggest or c["joint"] is not None or c["per_image"] is not None):
        raise RuntimeError(f"mdil {fn}: a suggest map, joint and per_image need thr ({nc} integers in [0, {Q_ONE}])")
    if q_class is not None:
        if q_class == GIVEN:
            q_class = nc
        if not isinstance(q_class, int) or not 0 <= q_class <= nc:
            raise RuntimeError(f"mdil {fn}: q_class must be a class in [0, {nc}) or \"{GIVEN}\", got {q_class!r}")
        if q_class == nc and target is None:
            raise RuntimeError(f"mdil {fn}: q_class \"{GIVEN}\" needs a target")
    if q_class is None and not want_suggest and all(v is None for v in c.values()):
        raise RuntimeError(f"mdil {fn}: nothing to do (no qmap, no suggest map, no counters)")
    with torch.no_grad(), torch.cuda.device(dev):
        thr_d = None if thr is None else hc.device_ints(fn, _PATH, thr, "thr", nc, dev, 0, Q_ONE)
        qmap = torch.empty(N, 2 * H, 2 * W, dtype=QMAP, device=dev) if q_class is not None else None
        suggest = torch.empty(N, 2 * H, 2 * W, dtype=torch.uint8, device=dev) if want_suggest else None
        _audit_lib.check(
            lib.mdil_audit_head(x.data_ptr(), w.data_ptr(), b.data_ptr(), N, H, W, nc, hc.ptr(target),
                                int(ignore_index), hc.ptr(thr_d), 0 if q_class is None else q_class, none_id,
                                hc.ptr(qmap), hc.ptr(suggest), *(hc.ptr(c[k]) for k in HEAD_COUNTERS),
                                torch.cuda.current_stream(dev).cuda_stream),
            "mdil_audit_head")
    return qmap, suggest


def audit_apply(target, suggest, selfq, nc, max_q, mode="prune", ignore_index=-1, none_id=255, drop_id=255,
                counters=None, want_out=True, want_mask=False):
    """The cleaned map of stored maps (any shape, one size), on the current stream.  An issue (target
    valid, a class suggested, and it is not the target) of given class c is acted on when
    ``selfq <= max_q[c]`` (nc ints in [-1, 65535] or an int32 [nc] device tensor): pruned to ``drop_id``
    or relabelled to the suggestion; every other pixel keeps its target.  -> (out u8 or None, mask u8
    or None: 255 acted on, 128 an issue left alone, 0 otherwise).  ``counters``: any of
    ``APPLY_COUNTERS`` as int64 device tensors (``apply_counter_shapes``), accumulated into."""
    fn = "audit_apply"
    lib = _audit_lib.load()
    nc = check_nc(fn, nc)
    if mode not in MODES:
        raise RuntimeError(f"mdil {fn}: mode {mode!r} (one of {list(MODES)})")
    hc.check_ignore_index(fn, ignore_index)
    none_id, drop_id = check_id(fn, "none_id", none_id), check_id(fn, "drop_id", drop_id)
    hc.chk(fn, _PATH, target, "target", torch.uint8)
    hc.chk(fn, _PATH, suggest, "suggest", torch.uint8)
    hc.chk(fn, _PATH, selfq, "selfq", QMAP)
    if target.numel() == 0 or target.shape != suggest.shape or target.shape != selfq.shape or \
            target.device != suggest.device or target.device != selfq.device:
        raise RuntimeError(f"mdil {fn}: expects uint8 target and suggest maps and a uint16 selfq map of one shape on "
                           f"one device (got target {tuple(target.shape)} on {target.device}, suggest "
                           f"{tuple(suggest.shape)} on {suggest.device}, selfq {tuple(selfq.shape)} on {selfq.device})")
    dev = target.device
    c = rc.check_counters(fn, counters, APPLY_COUNTERS)
    shapes = apply_counter_shapes(nc)
    hc.check_tables(fn, _PATH, dev, torch.int64, tuple((c[k], k, shapes[k]) for k in APPLY_COUNTERS))
    if not want_out and not want_mask and all(v is None for v in c.values()):
        raise RuntimeError(f"mdil {fn}: nothing to do (no out map, no mask, no counters)")
    with torch.no_grad(), torch.cuda.device(dev):
        max_q_d = hc.device_ints(fn, _PATH, max_q, "max_q", nc, dev, -1, Q_ONE - 1)
        out = torch.empty_like(target) if want_out else None
        mask = torch.empty_like(target) if want_mask else None
        _audit_lib.check(
            lib.mdil_audit_apply(target.data_ptr(), suggest.data_ptr(), selfq.data_ptr(), target.numel(), nc,
                                 int(ignore_index), none_id, MODES.index(mode), max_q_d.data_ptr(), drop_id,
                                 hc.ptr(out), hc.ptr(mask), *(hc.ptr(c[k]) for k in APPLY_COUNTERS),
                                 torch.cuda.current_stream(dev).cuda_stream),
            "mdil_audit_apply")
    return out, mask


# ------------------------------------------------------------------------- the report arithmetic
def _ints(t, who, name):
    t = torch.as_tensor(t)
    if t.is_cuda or t.dtype != torch.int64:
        raise RuntimeError(f"mdil {who}: {name} must be a host int64 tensor (got {t.dtype} on {t.device})")
    return t


def thresholds(count, qsum):
    """thr[c] = ceil(qsum[c] / count[c]), the mean self-confidence of the pixels given class c rounded up
    (q >= thr is q >= the mean, q being an integer); 65536 -- never met -- where count[c] == 0.  Exact,
    in Python integers."""
    count, qsum = _ints(count, "audit thresholds", "count"), _ints(qsum, "audit thresholds", "qsum")
    if count.dim() != 1 or count.shape != qsum.shape:
        raise RuntimeError(f"mdil audit thresholds: count and qsum must be int64 [nc] (got {tuple(count.shape)} and "
                           f"{tuple(qsum.shape)})")
    out = []
    for n, s in zip(count.tolist(), qsum.tolist()):
        if n < 0 or s < 0 or s > n * (Q_ONE - 1):
            raise RuntimeError(f"mdil audit thresholds: count {n} and qsum {s} are not the counters of one sweep")
        out.append(Q_ONE if n == 0 else -(-s // n))
    return out


def max_q_of(share):
    """A self-confidence in [0, 1] -> the largest q at or below it (65535 for 1)."""
    if not 0.0 <= float(share) <= 1.0:
        raise RuntimeError(f"mdil audit: self-confidence {share} outside [0, 1]")
    return min(Q_ONE - 1, int(float(share) * Q_ONE))


def confident_joint_report(joint, count, top=20):
    """The confident joint ``joint`` (int64 [nc, nc + 1], the last column "no class confident") and the
    class counts ``count`` (int64 [nc]) -> the figures of Northcutt et al., in fp64 on the host:

        C        = joint without the "none" column
        Q~[i][j] = C[i][j] / sum_j C[i][j] * count[i]          (eq. 2: rows scaled to the class counts)
        Q        = Q~ / sum Q~                                  (eq. 3: the estimated joint of given and true label)
        noise_given[i]  = 1 - Q[i][i] / sum_j Q[i][j]           share of the labels GIVEN as i that are wrong
        noise_missed[j] = 1 - Q[j][j] / sum_i Q[i][j]           share of the pixels that ARE j and are labelled otherwise
        issues          = n * sum_{i != j} Q[i][j],  n = the pixels of the rows that have a confident pixel
        pairs           = the off-diagonal cells, largest Q first (ties: lowest given, then suggested, class)

    A class none of whose pixels has a confident class gives a zero row and a noise of 0."""
    joint, count = _ints(joint, "confident_joint_report", "joint"), _ints(count, "confident_joint_report", "count")
    nc = count.numel()
    if count.dim() != 1 or tuple(joint.shape) != (nc, nc + 1):
        raise RuntimeError(f"mdil confident_joint_report: expects joint [nc, nc + 1] and count [nc] (got "
                           f"{tuple(joint.shape)} and {tuple(count.shape)})")
    C = joint[:, :nc].double()
    rows = C.sum(1)
    scaled = torch.where(rows[:, None] > 0, C / rows.clamp(min=1.0)[:, None] * count.double()[:, None],
                         torch.zeros_like(C))
    total = float(scaled.sum())
    Q = scaled / total if total > 0 else scaled
    diag = Q.diagonal()
    given, true = Q.sum(1), Q.sum(0)
    noise_given = torch.where(given > 0, 1.0 - diag / given.clamp(min=1e-300), torch.zeros_like(given))
    noise_missed = torch.where(true > 0, 1.0 - diag / true.clamp(min=1e-300), torch.zeros_like(true))
    off = Q.clone()
    off.fill_diagonal_(0.0)
    cells = sorted(((-float(off[i, j]), i, j) for i in range(nc) for j in range(nc) if i != j and off[i, j] > 0))
    pairs = [{"given": i, "suggested": j, "joint": -v, "confident_pixels": int(joint[i, j])} for v, i, j in cells[:top]]
    return {"calibrated_joint": Q.tolist(), "noise_given": noise_given.tolist(), "noise_missed": noise_missed.tolist(),
            "estimated_issues": float(off.sum()) * total, "estimated_issue_share": float(off.sum()),
            "confident_issues": int(joint[:, :nc].sum() - joint[:, :nc].diagonal().sum()),
            "no_confident_class": joint[:, nc].tolist(), "top_pairs": pairs}


class LabelAuditor:
    """The meter of this add-on.  ``fit(*source, target=)`` is sweep 1 on a batch (count and qsum
    accumulate on the device); ``thresholds()`` reads them back once, or ``set_thresholds`` gives saved
    ones; ``audit(*source, target=)`` is sweep 2 on a batch: it adds to the joint and keeps the batch's
    per-image counts, and returns the batch's (self-q map, suggest map).  The forward runs once per
    sweep; the features are not kept between the sweeps."""

    def __init__(self, nc, ignore_index=-1, none_id=255):
        self.nc = check_nc("LabelAuditor", nc)
        hc.check_ignore_index("LabelAuditor", ignore_index)
        self.ignore_index, self.none_id = int(ignore_index), check_id("LabelAuditor", "none_id", none_id)
        self.fitted, self.audited, self.per_image, self.thr, self.thr_d = {}, {}, [], None, None

    def _predict(self, model, images, task, **kw):
        model.eval()
        with torch.no_grad():
            feat = model.features(images, task).contiguous()
            w, b = model.head_params(task)
            return self._head(feat, w.detach(), b.detach(), **kw)

    def _head(self, x, w, b, **kw):
        return audit_head(x, w, b, ignore_index=self.ignore_index, none_id=self.none_id, **kw)

    def _source(self, who, source, target):
        if len(source) != 3:
            raise RuntimeError(f"mdil LabelAuditor.{who}: expects (model, images, task) or (features, weight, bias)")
        if target is None:
            raise RuntimeError(f"mdil LabelAuditor.{who}: a label audit needs the batch's target")
        return rc.meter_source("LabelAuditor", _PATH, source, 1, self._predict, self._head, "features")

    def fit(self, *source, target=None):
        """Sweep 1 on a batch: count and qsum."""
        fn, dev, N, H, W = self._source("fit", source, target)
        if not self.fitted:
            self.fitted = new_head_counters(self.nc, N, dev, ("count", "qsum", "bad_targets", "nonfinite"))
        fn(*source, target=target, counters=self.fitted)

    def thresholds(self):
        """The thresholds of what ``fit`` has seen (and from here on of ``audit``)."""
        if not self.fitted:
            raise RuntimeError("mdil LabelAuditor.thresholds: fit() has seen no batch")
        rc.refuse_bad_targets("LabelAuditor", self.fitted, self.nc, self.ignore_index)
        self.set_thresholds(thresholds(self.fitted["count"].cpu(), self.fitted["qsum"].cpu()))
        return self.thr

    def set_thresholds(self, thr):
        self.thr, self.thr_d = check_thr("LabelAuditor.set_thresholds", thr, self.nc), None

    def audit(self, *source, target=None):
        """Sweep 2 on a batch -> (self-q u16 [N,2H,2W], suggest u8 [N,2H,2W])."""
        fn, dev, N, H, W = self._source("audit", source, target)
        if self.thr is None:
            raise RuntimeError("mdil LabelAuditor.audit: no thresholds yet (thresholds() after fit(), or set_thresholds)")
        if not self.audited:
            self.audited = new_head_counters(self.nc, N, dev, ("count", "joint", "bad_targets", "nonfinite"))
        if self.thr_d is None:
            self.thr_d = torch.tensor(self.thr, dtype=torch.int32).to(dev)
        per_image = torch.zeros(N, self.nc, 2, dtype=torch.int64, device=dev)
        selfq, suggest = fn(*source, target=target, thr=self.thr_d, q_class=GIVEN, want_suggest=True,
                            counters=dict(self.audited, per_image=per_image))
        self.per_image.append(per_image)
        return selfq, suggest

    def counters(self):
        """Sweep 2's counters on the host: count [nc], joint [nc, nc + 1], per_image [images, nc, 2],
        bad_targets and nonfinite as ints.  Refuses targets outside [0, nc) that are not the ignore index."""
        if not self.audited:
            raise RuntimeError("mdil LabelAuditor.counters: audit() has seen no batch")
        rc.refuse_bad_targets("LabelAuditor", self.audited, self.nc, self.ignore_index)
        nonfinite = int(self.audited["nonfinite"].item()) + (int(self.fitted["nonfinite"].item()) if self.fitted else 0)
        return {"count": self.audited["count"].cpu(), "joint": self.audited["joint"].cpu(),
                "per_image": torch.cat(self.per_image).cpu(), "bad_targets": 0, "nonfinite": nonfinite}


def top_images(per_image, stems, top):
    """The ``top`` images by their share of issues among their labelled pixels (ties: the earlier image)."""
    labelled, issues = per_image[:, :, 0].sum(1), per_image[:, :, 1].sum(1)
    order = sorted(range(len(stems)), key=lambda i: (-(int(issues[i]) / max(1, int(labelled[i]))), i))
    return [{"image": stems[i], "labelled": int(labelled[i]), "issues": int(issues[i]),
             "issue_share": int(issues[i]) / max(1, int(labelled[i])), "issues_per_class": per_image[i, :, 1].tolist()}
            for i in order[:top]]


# ------------------------------------------------------------------------------------------ CLI
def read_thresholds(path, nc):
    """The thresholds of a ``--fit`` file."""
    import json
    with open(path) as f:
        saved = json.load(f)
    if saved.get("mode") != "fit" or "thr" not in saved:
        raise RuntimeError(f"--thresholds {path}: not a file written by --fit")
    if saved.get("num_classes") != nc:
        raise RuntimeError(f"--thresholds {path}: fitted on a head of {saved.get('num_classes')} classes, this one has {nc}")
    return check_thr("--thresholds", saved["thr"], nc)


def plan_clean_tree(args):
    """The label tree of ``--clean-root`` -> (labels' folder, label names, images' folder or None)."""
    return rc.plan_label_tree(args, args.clean_root)


def main(args):
    _refusals(args)
    rc.refuse_task(args.task, args.num_classes)
    if args.thresholds and not os.path.isfile(args.thresholds):
        raise RuntimeError(f"--thresholds {args.thresholds}: no such file")
    nc = args.num_classes[args.task]
    saved_thr = read_thresholds(args.thresholds, nc) if args.thresholds else None
    dev, nc, model = hc.load_model(args.state, args.num_classes, args.task)
    ignore = nc - 1                                    # the trainers' relabelled ignore class
    meter = LabelAuditor(nc, ignore, 255)
    report = {"dataset": rc.source_name(args), "subset": args.subset, "task": args.task, "num_classes": nc,
              "ignore_index": ignore}
    if saved_thr is not None:
        meter.set_thresholds(saved_thr)
        report["thresholds_from"] = args.thresholds
    else:
        n = 0
        for _, images, target in rc.batches(args, nc, dev):
            meter.fit(model, images, args.task, target=target)
            n += images.shape[0]
        thr = meter.thresholds()
        count, qsum = meter.fitted["count"].tolist(), meter.fitted["qsum"].tolist()
        report.update(fit_images=n, fit_count=count, fit_qsum=qsum)
        if args.fit:
            hc.write_json({"mode": "fit", "dataset": rc.source_name(args), "subset": args.subset, "task": args.task,
                           "num_classes": nc, "ignore_index": ignore, "images": n, "thr": thr, "count": count,
                           "qsum": qsum, "nonfinite": int(meter.fitted["nonfinite"].item())}, args.fit)
            print(f"thresholds of {n} images written to {args.fit}")
    report.update(thr=meter.thr, thr_probability=[t / Q_ONE for t in meter.thr])
    print("thresholds: " + " ".join(f"{t / Q_ONE:.4f}" for t in meter.thr))
    if not (args.json or args.out or args.clean_root):
        return report

    from . import predict as P
    palette = P.default_palette(nc).to(dev) if args.out else None
    max_q = [max_q_of(args.max_self_confidence)] * nc
    acted = new_apply_counters(nc, dev)
    stems = []
    with hc.png_pool() as pool:
        writer = ac.LabelTreeWriter(pool, args, "--clean-root", args.clean_root, args.out)
        for s, images, target in rc.batches(args, nc, dev, unique_stems=bool(args.out)):
            selfq, suggest = meter.audit(model, images, args.task, target=target)
            writer.wait()
            out, mask = audit_apply(target, suggest, selfq, nc, max_q, args.mode, ignore, 255, 255, acted, want_mask=True,
                                    want_out=bool(args.clean_root)) if args.out or args.clean_root else (None, None)
            if args.out:
                grey = torch.full((1, 3), GREY, dtype=torch.uint8, device=dev)
                colour = torch.where((mask != 0).unsqueeze(3), palette[suggest.long().clamp(max=nc - 1)], grey)
                writer.write_maps(s, issues=colour)
            writer.write_batch(s, images, out, ignore)
            stems.extend(s)
        written = writer.close()
    c = meter.counters()
    joint, count = c["joint"], c["count"]
    report.update(images=len(stems), labelled_pixels=int(count.sum()), count=count.tolist(),
                  confident_joint=joint.tolist(), bad_targets=c["bad_targets"], nonfinite=c["nonfinite"],
                  top_images=top_images(c["per_image"], stems, args.top), written=written)
    report.update(confident_joint_report(joint, count, args.top))
    if args.out or args.clean_root:
        report.update(mode=args.mode, max_self_confidence=args.max_self_confidence, max_q=max_q[0],
                      acted=acted["acted"].tolist(), acted_pixels=int(acted["acted"].sum().item()))
    print(f"{report['dataset']} (task {args.task}): {len(stems)} images, {report['labelled_pixels']} labelled pixels, "
          f"{report['confident_issues']} confident label issues, an estimated {report['estimated_issues']:.0f} "
          f"({report['estimated_issue_share'] * 100:.2f} %); {report['nonfinite']} non-finite pixels")
    for pair in report["top_pairs"][:5]:
        print(f"  given {pair['given']:2d} -> suggested {pair['suggested']:2d}: {pair['joint'] * 100:.3f} % of the labels "
              f"({pair['confident_pixels']} confident pixels)")
    return ac.finish(report, written, args)


def _refusals(args):
    """Raise a RuntimeError that names why this combination of flags is refused."""
    rc.refuse_data(args)
    if not (args.json or args.fit or args.out or args.clean_root):
        raise RuntimeError("nothing to do: give --json FILE, --fit FILE, --out DIR or --clean-root ROOT")
    if args.fit and args.thresholds:
        raise RuntimeError("--fit FILE writes the thresholds of this split, --thresholds FILE reads saved ones: give one")
    ac.refuse_tree(args, "--clean-root", args.clean_root)
    if not 0.0 <= args.max_self_confidence <= 1.0:
        raise RuntimeError(f"--max-self-confidence {args.max_self_confidence} outside [0, 1]")
    if args.top < 0:
        raise RuntimeError(f"--top {args.top} is negative")


def build_parser():
    p = hc.RefusingParser(_refusals, description="label audit of a dataset against a checkpoint: confident-learning "
                                                 "thresholds, the confident joint, label issues per class and image, "
                                                 "issue maps and a cleaned label tree")
    p.add_argument("--state", required=True, help="checkpoint written by the trainers (or by the reference)")
    p.add_argument("--num-classes", type=int, nargs="+", required=True)
    p.add_argument("--task", type=int, required=True, help="which task's decoder audits, in its own label space")
    rc.add_data_flags(p, dataset_help="the labelled dataset to audit", synthetic_help="N procedural images instead (labelled)")
    p.add_argument("--fit", help="write the per-class thresholds of this split here")
    p.add_argument("--thresholds", help="a file written by --fit: skip sweep 1 and use its thresholds")
    p.add_argument("--json", help="write the report here")
    p.add_argument("--top", type=int, default=20, help="how many pairs and images the report lists (default %(default)s)")
    p.add_argument("--out", help="write <stem>_issues.png here: the suggested class's colour on an issue, grey elsewhere")
    p.add_argument("--clean-root", help="write a label tree with the issues pruned or relabelled, laid out as "
                                        "pseudo --out-root lays it out")
    p.add_argument("--layout", choices=("cityscapes", "BDD"), help="the tree --clean-root writes")
    p.add_argument("--mode", choices=MODES, default="prune", help="issues become 255 (prune) or the suggested class")
    p.add_argument("--max-self-confidence", type=float, default=1.0,
                   help="act only on issues whose given class has at most this probability (default %(default)s: all)")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
