"""What the GPU suites of the head add-ons share (predict, fullres, ensemble, drift, calibration,
boundary; latent and similarity take the model helpers): the seeded head inputs, their fp64
reference and near-tie rule, the label check with its two exclusion policies, targets and look-up
tables, the sentinel arena of the guard-band tests, and the device / model / checkpoint helpers
behind each file's fixtures.  Importing this needs CPU torch only; everything that touches the
package or a device does so when it is called.

Which pixels may differ.  An fp32 evaluation of a logit with k roundings on its longest path is
within gamma_k * S of the exact value, gamma_k = k u / (1 - k u), u = 2^-24,
S = |b_c| + sum_ci |x_ci| |w_ci,c| (resized like the logit where the logit is); so the order of two
classes can flip only where their exact margin is at most 2 * gamma_k * S (S of the larger of the
two).  ``near_tie`` marks those pixels; ``check_labels`` excludes them, requires every other pixel
to match exactly and bounds how many may be excluded.

tests/golden/head_cases.json pins the bytes of every draw here (tests/test_head_cases_cpu.py)."""
import functools

import torch
import torch.nn.functional as F

U = 2.0 ** -24
CLASSES = (2, 20, 27, 32)
SHAPES = ((1, 1, 1), (1, 9, 7), (2, 12, 20), (3, 16, 48))


def gamma(k):
    return k * U / (1 - k * U)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def as_bytes(t):
    return t.contiguous().view(torch.uint8) if t.dtype != torch.uint8 else t


def host(d):
    return {k: (None if v is None else v.cpu()) for k, v in d.items() if k != "workspace"}


def draw(nc, shape, seed):
    """Seeded head inputs (as tests/test_hip_parity.py::test_fused_head_and_loss draws them)
    -> x [N,16,H,W], w [16,nc,2,2], b [nc]."""
    N, H, W = shape
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(16, nc, 2, 2, generator=g) * 0.3
    b = torch.randn(nc, generator=g) * 0.2
    x = F.relu(torch.randn(N, 16, H, W, generator=g))
    return x, w, b


def case_seed(nc, shape):
    return 10 * nc + shape[1]


@functools.lru_cache(maxsize=None)
def head_inputs(nc, shape):
    """``draw`` at ``case_seed``: the inputs of case (nc, shape) in every suite; shared, never modified."""
    return draw(nc, shape, case_seed(nc, shape))


def head64(x, w, b):
    """-> (fp64 logits [N,nc,2H,2W], S [N,nc,2H,2W]: the same sum on absolute values)."""
    logits = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2)
    S = F.conv_transpose2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=2)
    return logits, S


def near_tie(logits, S, k):
    """Pixels whose top-2 margin is within 2 gamma_k S (the larger S of the two classes)."""
    top, idx = logits.topk(2, dim=1)
    bound = 2 * gamma(k) * S.gather(1, idx).max(1)[0]
    return (top[:, 0] - top[:, 1]) <= bound


def cap(pixels):
    return 0 if pixels < 100 else max(1, pixels // 1000)


def share(limit):
    """Exclusion policy: at most the share ``limit`` of a case's pixels."""
    def check(excluded, what):
        part = excluded.double().mean().item()
        print(f"{what}: excluded {int(excluded.sum())} of {excluded.numel()} pixels")
        assert part <= limit, f"{what}: {part:.2%} of the pixels are fp32 near-ties"
    return check


def count_cap(excluded, what):
    """Exclusion policy: at most ``cap(pixels)`` pixels, max(1, pixels // 1000) and none below 100."""
    n_ex = int(excluded.sum())
    print(f"{what}: excluded {n_ex} of {excluded.numel()} pixels (cap {cap(excluded.numel())})")
    assert n_ex <= cap(excluded.numel()), f"{what}: {n_ex} pixels are fp32 near-ties"


def check_labels(label, ref, excluded, what, limit):
    """``limit`` (``share(...)`` or ``count_cap``) is a condition on the reference alone and comes
    first; then u8 labels of the reference's shape that equal it at every pixel not excluded."""
    limit(excluded, what)
    assert label.dtype == torch.uint8 and tuple(label.shape) == tuple(ref.shape)
    wrong = (label.long() != ref) & ~excluded
    assert not wrong.any(), f"{what}: {int(wrong.sum())} of {wrong.numel()} labels differ from the fp64 argmax"


def predict_labels(dev, x, w, b):
    from mdil_ss_amd.predict import predict_head
    label = predict_head(nhwc(x).to(dev), w.to(dev), b.to(dev), None, False)[0]
    torch.cuda.synchronize()
    return label.cpu()


def make_target(nc, shape, ignore, seed):
    """u8 targets in [0, nc) with some ignore pixels and a few values >= nc."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, nc, shape, generator=g, dtype=torch.uint8)
    r = torch.rand(shape, generator=g)
    t[r < 0.10] = ignore
    t[(r >= 0.10) & (r < 0.12)] = nc                    # out of range
    t[(r >= 0.12) & (r < 0.13)] = 200
    return t


def random_palette(nc):
    return torch.randint(0, 256, (nc, 3), generator=torch.Generator().manual_seed(nc), dtype=torch.uint8)


def random_luts(nc):
    """(id_map u8 [nc], palette u8 [nc,3]) with a 255 and a duplicated row each."""
    g = torch.Generator().manual_seed(nc)
    ids = torch.randint(0, 256, (nc,), generator=g, dtype=torch.uint8)
    pal = torch.randint(0, 256, (nc, 3), generator=g, dtype=torch.uint8)
    ids[0], ids[nc - 1] = 255, ids[1]
    pal[0], pal[nc - 1] = torch.tensor([255, 0, 255], dtype=torch.uint8), pal[1]
    return ids, pal


def expected_counts(target, label, nc, ignore):
    """-> (confusion matrix [nc,nc] by bincount, targets out of range, pixels counted)."""
    t, p = target.reshape(-1).long(), label.reshape(-1).long()
    counted = (t < nc) & (t != ignore)
    matrix = torch.bincount(t[counted] * nc + p[counted], minlength=nc * nc).reshape(nc, nc)
    return matrix, int(((t >= nc) & (t != ignore)).sum()), int(counted.sum())


def check_confusion(head, dev, nc, N, size, ignore):
    """``head(target=, ignore_index=, confusion=, bad_targets=)`` -> (label, ...), called twice into the
    same counters: they hold the bincounts of its own labels, then twice that.  -> label on the host."""
    target = make_target(nc, (N,) + tuple(size), ignore, seed=nc + size[0])
    conf = torch.zeros(nc, nc, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    kw = dict(target=target.to(dev), ignore_index=ignore, confusion=conf, bad_targets=bad)
    label = head(**kw)[0].cpu()
    matrix, n_bad, n_counted = expected_counts(target, label, nc, ignore)
    assert n_bad > 0 or target.numel() < 50
    assert torch.equal(conf.cpu(), matrix) and int(bad.item()) == n_bad
    assert int(conf.sum().item()) == n_counted
    again = head(**kw)[0].cpu()                          # accumulates, does not overwrite
    assert torch.equal(again, label)
    assert torch.equal(conf.cpu(), 2 * matrix) and int(bad.item()) == 2 * n_bad
    return label


class Arena:
    """One 0xA5-filled u8 device buffer [guard | a | guard | b | ... | guard] for the maps ``sizes``
    (ordered {name: bytes}), every start 16-byte aligned: what a kernel writes outside the maps it
    was given lands in a guard band or in a map it was not given, and shows."""

    def __init__(self, dev, sizes, guard=256):
        self.sizes, self.off, pos = dict(sizes), {}, guard
        for name, n in self.sizes.items():
            self.off[name] = pos
            pos = (pos + n + guard + 15) // 16 * 16
        self.buf = torch.full((pos,), 0xA5, dtype=torch.uint8, device=dev)
        self.bytes = None

    def ptr(self, name):
        return self.buf.data_ptr() + self.off[name]

    def read(self):
        """Copy the buffer to the host, once the kernel is done; ``cut`` and ``assert_untouched`` read that copy."""
        self.bytes = self.buf.cpu()

    def cut(self, name):
        return self.bytes[self.off[name]:self.off[name] + self.sizes[name]]

    def assert_untouched(self, written_names, what=None):
        written = torch.zeros(self.bytes.numel(), dtype=torch.bool)
        for name in written_names:
            written[self.off[name]:self.off[name] + self.sizes[name]] = True
        assert (self.bytes[~written] == 0xA5).all(), what


def device(path_name):
    assert torch.cuda.is_available(), f"the {path_name} path needs an MI355X"
    import mdil_ss_amd  # noqa: F401
    return torch.device("cuda", 0)


def tiny_model(dev):
    from mdil_ss_amd.models.erfnet_RA_parallel import Net as Net_RAP
    torch.manual_seed(0)
    return Net_RAP([20, 20], 2, 1).to(dev).eval()


def teacher_student(dev):
    """(teacher [20], student [20, 20] initialised from it and then perturbed), on the device, eval mode."""
    from mdil_ss_amd.models.erfnet_RA_parallel import Net as Net_RAP
    from oracle import fixtures as fx
    from oracle import rap_oracle as O
    torch.manual_seed(1)
    teacher = Net_RAP([20], 1, 0)
    t_sd = {k: v.clone() for k, v in teacher.state_dict().items()}
    fx.perturb_bn(t_sd, 11)
    teacher.load_state_dict(t_sd)
    torch.manual_seed(0)
    student = Net_RAP([20, 20], 2, 1)
    s_sd = {k: v.clone() for k, v in student.state_dict().items()}
    for k, v in O.student_init_from_teacher(t_sd, s_sd, 1).items():
        s_sd[k].copy_(v)
    student.load_state_dict(s_sd)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for p in student.parameters():
            p.mul_(1 + 0.05 * torch.randn(p.shape, generator=g))
    return teacher.to(dev).eval(), student.to(dev).eval()


def save_checkpoint(model, path):
    """The trainers' checkpoint layout: DataParallel key names, tensors on the host."""
    torch.save({"state_dict": {"module." + k: v.cpu() for k, v in model.state_dict().items()}}, path)


def side_stream(fn):
    """``fn()`` on a fresh stream, synchronised before its result is handed back."""
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = fn()
    side.synchronize()
    return out
