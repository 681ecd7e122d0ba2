"""The grid plans of the capped-grid kernels of the training path (csrc/head.hip, loss.hip, pool.hip,
adam.hip), the cases that put them into their grid-stride loop, and the float64 references those cases
are compared with (tests/test_grid_rounds_cpu.py, tests/test_grid_rounds_gpu.py).
Importing this needs CPU torch only.

Each of these kernels launches at most a fixed number of work-groups and walks the rest of its tensor in
a loop: a thread (a wave, for the fused head) takes item i, i + stride, i + 2 stride, ...  ROUND k is
the k-th trip of that loop.  The constants below are copied from the sources and pinned against their
text by the CPU test; the plans do not depend on the device."""
import functools
import types

import torch
import torch.nn.functional as F

from oracle import fixtures as fx

# ------------------------------------------------------------------------------------------------
# constants of the sources
# ------------------------------------------------------------------------------------------------
MDIL_WG = 256                 # csrc/common.h
HD_T = 256                    # csrc/head.hip
HD_WAVES = HD_T // 64
HD_MAX_BLOCKS = 1024
HD_TILE = 16                  # pixels per wave tile
HD_REDUCE_STRIDE = 4 * 16     # head_wgrad_reduce_kernel: 4 slices x 16 loads in flight
LOSS_MAX_BLOCKS = 2048        # csrc/loss.hip
POOL_MAX_BLOCKS = 4096        # csrc/pool.hip, grid_for
ADAM_MAX_BLOCKS = 2048        # csrc/adam.hip

LOSS_BOUND = LOSS_MAX_BLOCKS * MDIL_WG        # items above which a thread takes a second one
POOL_BOUND = POOL_MAX_BLOCKS * MDIL_WG
ADAM_BOUND = ADAM_MAX_BLOCKS * MDIL_WG
HEAD_BOUND = HD_MAX_BLOCKS * HD_WAVES * HD_TILE


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------
# plans
# ------------------------------------------------------------------------------------------------
def head_plan(npix):
    """head_grid + the tile walk of every head kernel: a wave takes tiles widx, widx + 4 blocks, ..."""
    tiles = cdiv(npix, HD_TILE)
    blocks = max(1, min(HD_MAX_BLOCKS, cdiv(tiles, HD_WAVES)))
    waves = HD_WAVES * blocks
    return types.SimpleNamespace(
        npix=npix, blocks=blocks, waves=waves, tiles=tiles, rounds=cdiv(tiles, waves),
        per_wave=(tiles // waves, cdiv(tiles, waves)),          # (min, max) over the launched waves
        last_px=npix - (tiles - 1) * HD_TILE, last_round=(tiles - 1) // waves, last_slot=(tiles - 1) % waves,
        reduce_passes=cdiv(blocks, HD_REDUCE_STRIDE), reduce_clamped=blocks % HD_REDUCE_STRIDE != 0)


def head_round(q, npix):
    """Round of input pixel ``q`` (int or int64 tensor)."""
    return (q // HD_TILE) // head_plan(npix).waves


def head_slot(q, npix):
    """Wave slot (4 * block + wave) of input pixel ``q``."""
    return (q // HD_TILE) % head_plan(npix).waves


def flat_plan(n, wg=MDIL_WG, cap=LOSS_MAX_BLOCKS):
    """The one-item-per-thread kernels: min(cap, ceil(n / wg)) work-groups, thread t takes t, t + threads, ..."""
    blocks = max(1, min(cap, cdiv(n, wg)))
    threads = blocks * wg
    return types.SimpleNamespace(n=n, blocks=blocks, threads=threads, rounds=cdiv(n, threads),
                                 per_thread=(n // threads, cdiv(n, threads)))


def flat_round(i, n, wg=MDIL_WG, cap=LOSS_MAX_BLOCKS):
    return i // flat_plan(n, wg, cap).threads


def live_tiles(npix):
    """The tiles of the sparse forms: wave slot 5 in every round, the last tile's slot in every round."""
    p = head_plan(npix)
    out = []
    for slot in (5, p.last_slot):
        out += [t for t in range(slot, p.tiles, p.waves) if t not in out]
    return out


def tile_pixels(tile, npix):
    return list(range(tile * HD_TILE, min(npix, (tile + 1) * HD_TILE)))


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
NCS = (20, 27)
HEAD_CASES = {"H1": (2, 130, 257), "H2": (2, 260, 257), "H3": (1, 100, 131)}         # N, H, W of the features
LOSS_CASES = {"L1": (2, 600, 601)}                                                   # N, H, W of the logits
POOL_CASES = {"P1": ((3, 300, 302, 16), 64, 48), "P2": ((2, 840, 836, 3), 16, 13),   # x NHWC, z pitch, offset
              "P3": ((2, 184, 180, 64), 128, 64)}
ADAM_CASES = {"A1": 1060921}
CE_SCALE, KLD_SCALE = 0.7, 0.1          # the upstream gradients of test_fused_head_and_loss
SENTINEL = 12345.5


def class_weights(nc):
    """The class weights of test_fused_head_and_loss / test_losses; the last class has weight zero."""
    if nc == 20:
        return torch.tensor(fx.WEIGHT_BDD)
    return torch.cat([1.0 + 9.0 * torch.rand(nc - 1, generator=torch.Generator().manual_seed(4)), torch.zeros(1)])


@functools.lru_cache(maxsize=2)
def head_inputs(name, nc):
    """Seeded inputs of a head case, fp32 on the host, shared and never modified: student / teacher head
    parameters (scale 0.3 / 0.2), N(0, 1) features after ReLU as [N,16,H,W], labels [N,2H,2W], class weights."""
    N, H, W = HEAD_CASES[name]
    g = torch.Generator().manual_seed(1000 * nc + 7 * H + W)
    c = types.SimpleNamespace(name=name, nc=nc, N=N, H=H, W=W, npix=N * H * W, plan=head_plan(N * H * W))
    c.w, c.b = torch.randn(16, nc, 2, 2, generator=g) * 0.3, torch.randn(nc, generator=g) * 0.2
    c.wt, c.bt = torch.randn(16, nc, 2, 2, generator=g) * 0.3, torch.randn(nc, generator=g) * 0.2
    c.x, c.xt = F.relu(torch.randn(N, 16, H, W, generator=g)), F.relu(torch.randn(N, 16, H, W, generator=g))
    c.lab = fx.make_batch(N, 2 * H, 2 * W, nc, seed=3)[1][:, 0].contiguous()
    c.cw = class_weights(nc)
    return c


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def round_map(c):
    """[N,H,W] int64: the round of every input pixel's tile."""
    return head_round(torch.arange(c.npix), c.npix).reshape(c.N, c.H, c.W)


def last_tile_map(c):
    return (torch.arange(c.npix) // HD_TILE == c.plan.tiles - 1).reshape(c.N, c.H, c.W)


def up2(m):
    """A per-input-pixel map [N,H,W] at the 2 x 2 output pixels of each."""
    return m.repeat_interleave(2, 1).repeat_interleave(2, 2)


def live_mask(c, tiles=None):
    """[N,H,W] bool: the input pixels of the live tiles."""
    tiles = live_tiles(c.npix) if tiles is None else tiles
    m = torch.zeros(c.npix, dtype=torch.bool)
    for t in tiles:
        m[tile_pixels(t, c.npix)] = True
    return m.reshape(c.N, c.H, c.W)


def sparse_target(c):
    """The zero-weight class everywhere but at the 2 x 2 output pixels under each live tile."""
    return torch.where(up2(live_mask(c)), c.lab, torch.full_like(c.lab, c.nc - 1))


def sparse_features(c):
    m = live_mask(c)[:, None].to(torch.float32)
    return c.x * m, c.xt * m


# ------------------------------------------------------------------------------------------------
# float64 references: conv_transpose2d + the loss, gradients by autograd
# ------------------------------------------------------------------------------------------------
def ce64(logits, target, weight):
    """CrossEntropyLoss2d: -sum_p w[y_p] log_softmax(logits_p)[y_p] / sum_p w[y_p]  -> (loss, sum of weights)."""
    picked = F.log_softmax(logits, dim=1).gather(1, target.unsqueeze(1)).squeeze(1)
    wy = weight[target]
    return -(wy * picked).sum() / wy.sum(), wy.sum()


def kld64(s_logits, t_logits, numel=None):
    """The reference's KLDivLoss on probabilities: mean(t (log t - p_s)); ``numel`` replaces the divisor."""
    ps, t = F.softmax(s_logits, dim=1), F.softmax(t_logits, dim=1)
    total = (t * (t.log() - ps)).sum()
    return total / (t.numel() if numel is None else numel)


def head_ce_ref(x, w, b, target, weight, scale=CE_SCALE):
    """x [N,16,H,W], target [N,2H,2W] -> loss, wsum, logits NHWC and the gradients of ``scale * loss``
    (gx NHWC), all float64."""
    x, w, b = (t.double().requires_grad_(True) for t in (x, w, b))
    logits = F.conv_transpose2d(x, w, b, stride=2)
    loss, wsum = ce64(logits, target, weight.double())
    (scale * loss).backward()
    return types.SimpleNamespace(loss=float(loss.detach()), wsum=float(wsum.detach()), logits=nhwc(logits.detach()),
                                 gx=nhwc(x.grad), dw=w.grad, db=b.grad)


def head_kld_ref(xs, ws, bs, xt, wt, bt, scale=KLD_SCALE, numel=None):
    xs, ws, bs = (t.double().requires_grad_(True) for t in (xs, ws, bs))
    loss = kld64(F.conv_transpose2d(xs, ws, bs, stride=2),
                 F.conv_transpose2d(xt.double(), wt.double(), bt.double(), stride=2), numel)
    (scale * loss).backward()
    return types.SimpleNamespace(loss=float(loss.detach()), gx=nhwc(xs.grad), dw=ws.grad, db=bs.grad)


def dense_ce_ref(c):
    return head_ce_ref(c.x, c.w, c.b, c.lab, c.cw)


def dense_kld_ref(c):
    return head_kld_ref(c.x, c.w, c.b, c.xt, c.wt, c.bt)


def _gather(c, t, tiles):
    """The pixels of ``tiles`` of an [N,16,H,W] tensor as a one-row image [1,16,1,L], and their indices."""
    q = torch.tensor([p for tl in tiles for p in tile_pixels(tl, c.npix)])
    return t.permute(1, 0, 2, 3).reshape(16, -1)[:, q].reshape(1, 16, 1, -1), q


def _gather_target(c, q):
    """The labels under the input pixels ``q`` as the [1,2,2L] label image of the one-row feature image."""
    n, r = q // (c.H * c.W), q % (c.H * c.W)
    h, w = r // c.W, r % c.W
    rows = [torch.stack([c.lab[n, 2 * h + a, 2 * w + bb] for bb in (0, 1)], 1).reshape(-1) for a in (0, 1)]
    return torch.stack(rows)[None]


def sparse_ce_ref(c, tiles=None):
    """The sparse CE form.  The head maps every input pixel to its own 2 x 2 output pixels and pixels of weight
    zero add nothing to the loss, to the sum of weights or to any gradient, so the reference of the whole
    tensor IS the reference of the live pixels laid out as a one-row image (the CPU test compares the two).
    -> the reference (gx: [L,16] rows of the live pixels) and the pixels' indices."""
    tiles = live_tiles(c.npix) if tiles is None else tiles
    xg, q = _gather(c, c.x, tiles)
    r = head_ce_ref(xg, c.w, c.b, _gather_target(c, q), c.cw)
    r.gx = r.gx.reshape(-1, 16)
    return r, q


def sparse_kld_ref(c, tiles=None):
    """The sparse KLD form (both feature tensors zero outside the live tiles): dW comes from the live pixels
    alone, a staged zero contributes an exact zero.  One zero pixel is appended: its gx row is the row of
    every pixel outside the live tiles.  The loss and db are NOT those of the whole tensor.
    -> the reference (gx: [L,16] rows, gx_zero: [16]) and the pixels' indices."""
    tiles = live_tiles(c.npix) if tiles is None else tiles
    (xg, q), (xtg, _) = _gather(c, c.x, tiles), _gather(c, c.xt, tiles)
    pad = torch.zeros(1, 16, 1, 1)
    r = head_kld_ref(torch.cat([xg, pad], 3), c.w, c.b, torch.cat([xtg, pad], 3), c.wt, c.bt,
                     numel=c.npix * 4 * c.nc)
    rows = r.gx.reshape(-1, 16)
    r.gx, r.gx_zero = rows[:-1], rows[-1]
    return r, q


def ratio(got, want, rtol, atol):
    """|got - want| / (atol max|want| + rtol |want|), the measure of tests/test_hip_parity.py::close."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return (got - want).abs() / (atol * max(1e-30, float(want.abs().max())) + rtol * want.abs())


# ------------------------------------------------------------------------------------------------
# unfused losses, pool, Adam
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def loss_inputs(name, nc):
    """Student / teacher logits [N,nc,H,W] of scale 2 (test_losses), labels that include the ignore class."""
    N, H, W = LOSS_CASES[name]
    c = types.SimpleNamespace(name=name, nc=nc, N=N, H=H, W=W, npix=N * H * W, plan=flat_plan(N * H * W))
    g = torch.Generator().manual_seed(100 * nc + 1)
    c.s, c.t = torch.randn(N, nc, H, W, generator=g) * 2.0, torch.randn(N, nc, H, W, generator=g) * 2.0
    c.lab = fx.make_batch(N, H, W, nc, seed=3)[1][:, 0].contiguous()
    c.cw = class_weights(nc)
    return c


def sparse_loss_pixels(c):
    return [7, 7 + LOSS_BOUND, c.npix - 1]


def sparse_loss_target(c):
    """Labels of non-zero weight at three pixels (one per round, and the last), the zero-weight class elsewhere."""
    lab = torch.full((c.npix,), c.nc - 1, dtype=torch.int64)
    for k, p in enumerate(sparse_loss_pixels(c)):
        lab[p] = (3 + 5 * k) % (c.nc - 1)
    return lab.reshape(c.N, c.H, c.W)


def loss_refs(c, target):
    """float64: CE and KLD values and d/dlogits (NCHW) of the unscaled losses."""
    s = c.s.double().requires_grad_(True)
    ce, _ = ce64(s, target, c.cw.double())
    ce.backward()
    dce = s.grad
    s2 = c.s.double().requires_grad_(True)
    kld = kld64(s2, c.t.double())
    kld.backward()
    return types.SimpleNamespace(ce=float(ce.detach()), kld=float(kld.detach()), dce=dce, dkld=s2.grad)


def confusion_ref(logits, target, nc, ignore):
    """[3,nc] int64 (tp, fp, fn) as csrc/loss.hip counts them, by bincount on the argmax of the same logits."""
    pred, y = logits.argmax(1).reshape(-1), target.reshape(-1)
    keep = y != ignore
    hit = keep & (pred == y)
    miss = keep & (pred != y)
    tp = torch.bincount(y[hit], minlength=nc)
    fp = torch.bincount(pred[miss & (pred != ignore)], minlength=nc)
    fn = torch.bincount(y[miss], minlength=nc)
    return torch.stack([tp, fp, fn])


@functools.lru_cache(maxsize=1)
def pool_inputs(name):
    """x [N,H,W,C]: multiples of 1/4 in [-2, 2], then ReLU -- tied 2 x 2 windows are common; gz [N,H/2,W/2,pitch]
    non-zero in every channel, the conv slice included."""
    (N, H, W, C), pitch, coff = POOL_CASES[name]
    g = torch.Generator().manual_seed(H + W + C)
    c = types.SimpleNamespace(name=name, N=N, H=H, W=W, C=C, pitch=pitch, coff=coff,
                              total=N * (H // 2) * (W // 2) * C)
    c.plan = flat_plan(c.total, MDIL_WG, POOL_MAX_BLOCKS)
    c.x = F.relu((torch.randn(N, H, W, C, generator=g).clamp(-2, 2) * 4).round() / 4)
    c.gz = torch.randn(N, H // 2, W // 2, pitch, generator=g) + 3.0
    return c


def pool_refs(c):
    """max_pool2d and its float64 autograd gradient (NHWC, fp32: every value is a copy of an input)."""
    x = c.x.permute(0, 3, 1, 2).double().requires_grad_(True)
    y = F.max_pool2d(x, 2, 2)
    y.backward(c.gz[..., c.coff:c.coff + c.C].permute(0, 3, 1, 2).double())
    return nhwc(y.detach()).float(), nhwc(x.grad).float()


def pool_tied_windows(c):
    """[total] bool in the kernel's item order (n, ho, wo, c): windows whose maximum occurs more than once."""
    x = c.x.reshape(c.N, c.H // 2, 2, c.W // 2, 2, c.C)
    m = x.amax((2, 4), keepdim=True)
    return ((x == m).sum((2, 4)) > 1).reshape(-1)


@functools.lru_cache(maxsize=1)
def adam_inputs(name):
    n = ADAM_CASES[name]
    g = torch.Generator().manual_seed(n)
    return types.SimpleNamespace(n=n, plan=flat_plan(n, MDIL_WG, ADAM_MAX_BLOCKS),
                                 p=torch.randn(n, generator=g), g=torch.randn(n, generator=g) * 1e-3)
