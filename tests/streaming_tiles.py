"""Host-side mirror of how the streaming C -> C conv kernels (csrc/sconv.hip, wconv.hip, w4conv.hip)
split a launch into wave tiles, for tests/test_streaming_multitile_gpu.py, plus the fp64 reference
of the three-tap convolution those tests compare against.

All three kernels are persistent: 8 waves per work-group, ``nq`` pixel-tile queues per channel part
(capped by the CU count), wave ``w`` of queue ``gq`` owns tiles ``(w + 8 k) nq + gq``, k = 0, 1, ...
(its "rounds").  A wave meets the prefetch hand-over, the carried statistics and the ragged last
tile in a later round only when the launch has more than ``8 nq`` tiles."""
import torch

WAVES = 8
MAX_QUEUES = 256                                         # MDIL_BN_MAX_BLOCKS: one statistics partial per queue
PX_PER_TILE = {"sconv": 32, "wconv": 32, "w4conv": 64}
STREAMING = tuple(PX_PER_TILE)


def cu_count():
    return min(MAX_QUEUES, torch.cuda.get_device_properties(0).multi_processor_count)


def expected_family(C, ntaps, L, d):
    """Kernel family of a 3-tap (+ adapter tap) conv of dilation ``d`` along an axis of length ``L``:
    complete quads -> F(4,3), complete pairs -> F(2,3), else the direct form; the C = 64 adapter
    launches stay on F(2,3) (mdil_w4conv_covers)."""
    if L % (4 * d) == 0 and not (C == 64 and ntaps == 4):
        return "w4conv"
    if L % (2 * d) == 0:
        return "wconv"
    return "sconv"


def tiling(kind, C, ntaps, npix, plain, cus=None):
    """-> (queues, tiles) of one launch: sconv_queues / wconv_queues / w4conv_queues.  ``plain``: no
    residual / gate operand and no statistics (it only matters for F(4,3) at C = 64, whose plain
    form runs 64 output channels per work-group)."""
    cus = cu_count() if cus is None else min(MAX_QUEUES, cus)
    if kind == "sconv":
        nh, ntiles = C // 64, (npix + 31) // 32
    elif kind == "wconv":
        nh, ntiles = ((4 if ntaps == 4 else 2) if C == 128 else 1), (npix // 2 + 15) // 16
    elif kind == "w4conv":
        nh, ntiles = (1 if (C == 64 and plain) else C // 32), (npix // 4 + 15) // 16
    else:
        raise ValueError(kind)
    nq = min(cus // nh, (ntiles + WAVES - 1) // WAVES)
    if nh > 1:
        nq = (nq + 7) // 8 * 8
    return nq, ntiles


def tiles_per_wave(kind, C, ntaps, npix, plain, cus=None):
    """-> (min, max) tiles a wave of the launch runs."""
    nq, ntiles = tiling(kind, C, ntaps, npix, plain, cus)
    slots = WAVES * nq
    return ntiles // slots, -(-ntiles // slots)


def tile_map(kind, N, H, W, d, axis):
    """-> int64 [N*H*W]: the wave tile that stores each output pixel (NHWC pixel order).  The direct
    form tiles the pixels linearly; the Winograd forms number their pairs / quads (m = 2 / 4 pixels,
    ``d`` apart) so that 16 consecutive ones are as contiguous as the dilation allows:
    along W   id = ((n H + h) (W / m d) + wb) d + q,   w = m d wb + q (+ j d);
    along H   id = ((n (H / m d) + hb) d + q) W + w,   h = m d hb + q (+ j d)."""
    p = torch.arange(N * H * W)
    if kind == "sconv":
        return p // 32
    m = 4 if kind == "w4conv" else 2
    w, row = p % W, p // W
    if axis == "w":
        gid = (row * (W // (m * d)) + w // (m * d)) * d + w % d
    else:
        h, n = row % H, row // H
        gid = ((n * (H // (m * d)) + h // (m * d)) * d + h % d) * W + w
    return gid // 16


def launches(fn, capacity=256):
    """Run ``fn`` between ops.profile_begin() and ops.profile_end() -> [(family, cin, cout, ntaps, npix)]
    of its conv launches, in launch order."""
    from mdil_ss_amd import ops
    ops.profile_begin(capacity)
    try:
        fn()
    finally:
        recs = ops.profile_end(capacity)
    return [(k, ci, co, nt, int(round(fl / (2.0 * nt * ci * co)))) for k, ci, co, nt, fl, _ in recs
            if k in ops._PROF_CONV]


def paths(fn, capacity=256):
    """Kernel-family names ("sconv", "wconv", "w4conv", "tapconv", "c16conv") of the conv launches of ``fn``."""
    return [rec[0] for rec in launches(fn, capacity)]


# ------------------------------------------------------------------------------------------------
# fp64 reference: three shifted GEMMs on the NHWC tensor
# ------------------------------------------------------------------------------------------------
def _add_shifted(out, y, off, dim):
    """out[.., i, ..] += y[.., i + off, ..] along ``dim`` (zero outside)."""
    L = y.shape[dim]
    if off == 0:
        out += y
    elif 0 < off < L:
        out.narrow(dim, 0, L - off).add_(y.narrow(dim, off, L - off))
    elif -L < off < 0:
        out.narrow(dim, -off, L + off).add_(y.narrow(dim, 0, L + off))


def ref_conv3(x, w, d, axis, transpose=False):
    """x: [N,H,W,C] fp64, w: [C,C,3,1] (axis "h") or [C,C,1,3] (axis "w").
    forward:    out[p] = sum_k W_k   x[p + (k - 1) d]      (zero padding d, dilation d)
    transpose:  out[p] = sum_k W_k^T x[p - (k - 1) d]      (its data gradient)."""
    N, H, W_, C = x.shape
    w = w.double()
    flat = x.reshape(-1, C)
    out = torch.zeros_like(x)
    for k in range(3):
        wk = w[:, :, k, 0] if axis == "h" else w[:, :, 0, k]
        y = (flat @ (wk if transpose else wk.t())).reshape(N, H, W_, C)
        _add_shifted(out, y, (k - 1) * d * (-1 if transpose else 1), 1 if axis == "h" else 2)
    return out


def ref_1x1(x, wa, transpose=False):
    wa = wa.double().reshape(wa.shape[0], wa.shape[1])
    return (x.reshape(-1, x.shape[-1]) @ (wa if transpose else wa.t())).reshape(x.shape)
