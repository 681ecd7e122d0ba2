"""Host-side mirror of how the weight-gradient kernels (csrc/wgrad.hip) split a launch into chunks, for
tests/test_wgrad_chunks_cpu.py and tests/test_wgrad_chunks_gpu.py, plus the draws, the float64 reference
and the case table of those tests.  CPU torch only.

Every weight-gradient kernel hands each chunk (a work-group, or a wave of one) a contiguous run of
stages (LDS-tiled ``wgrad_kernel``: PS pixels), quads (streaming ``wgrad2`` / ``wgradw`` / ``wgradx``:
16 pixels, 16 row pairs, 32 pixels of a row) or tiles (``wgrad16``: 16 pixels).  The register-prefetch
hand-over, the double-buffered coordinate table, the carried accumulators and bias sums, the row / image
wrap of the scalar descriptors and a ragged last stage in a later round run only where a chunk holds at
least TWO of them; the plans below say at which sizes that is.

With integer operands in {-3 .. 3} \\ {0} every product and partial sum of a weight gradient is an
integer below 2^24 (``exact_budget``), hence exact in fp32 in ANY summation order; the Winograd-form
kernels only add the constants +-1 and 1/2 (and M1 + M2 is even).  The HIP result must then equal the
float64 reference bit for bit."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

# ------------------------------------------------------------------------------------------------
# constants copied from csrc/wgrad.hip (pinned against its text in tests/test_wgrad_chunks_cpu.py)
# ------------------------------------------------------------------------------------------------
TARGET = 768                    # make_plan: work-groups per LDS-tiled launch
WG16_CHUNKS = 1024              # launch_wgrad16: work-groups (4 waves each)
STREAM_GROUPS = 256             # launch_wgrad2 / launch_wgradw: work-groups of a C = 64 launch
CPW = {(64, 3): 2, (64, 4): 2, (128, 3): 4, (128, 4): 2}      # wgrad2_kernel<C, NTAPS, CPW>
CPW_W = 2                       # wgradw_kernel / wgradx_kernel: chunks per work-group
# (cout, cin) of the conv -> (CO tile, CI tile, stem): WG_CONFIGS
WG_CONFIGS = {(64, 64): (64, 64, False), (128, 128): (64, 64, False), (64, 128): (64, 64, False),
              (16, 16): (16, 16, False), (48, 16): (48, 16, False), (16, 64): (16, 64, False),
              (20, 16): (20, 16, False), (27, 16): (28, 16, False), (13, 27): (13, 27, True)}
MAX_TAPS = 9


def cdiv(a, b):
    return -(-a // b)


def _r16(v):
    return (v + 15) // 16 * 16


def geom(N, HO, WO, HI, WI, taps, in_pitch, OH, OW, out_pitch, ihs=1, iws=1, ohs=1, oho=0, ows=1, owo=0,
         coff=0):
    """The fields of mdil_geom (same argument order as ops.make_geom) as a plain namespace: whatever the
    mirror reads from a geometry it reads by these names, so it takes the ctypes struct as well."""
    taps = list(taps)
    pad = [0] * (MAX_TAPS - len(taps))
    ip = (in_pitch, in_pitch) if isinstance(in_pitch, int) else tuple(in_pitch)
    return SimpleNamespace(N=N, HO=HO, WO=WO, HI=HI, WI=WI, ihs=ihs, iws=iws, ntaps=len(taps),
                           dh=[t[0] for t in taps] + pad, dw=[t[1] for t in taps] + pad,
                           src=[t[2] for t in taps] + pad, in_pitch=list(ip), OH=OH, OW=OW, ohs=ohs, oho=oho,
                           ows=ows, owo=owo, out_pitch=out_pitch, out_coff=coff)


# ------------------------------------------------------------------------------------------------
# which kernel takes a launch: wgrad16_eligible / wgrad2_eligible / wgradw_eligible, wgrad_impl
# ------------------------------------------------------------------------------------------------
def _plain_s1(g, c):
    return (g.ihs == 1 and g.iws == 1 and g.ohs == 1 and g.ows == 1 and not g.oho and not g.owo and
            g.HI == g.HO and g.WI == g.WO and g.OH == g.HO and g.OW == g.WO and not g.out_coff and
            g.out_pitch == c and g.in_pitch[0] == c)


def wgrad16_eligible(g, cin, cout):
    if cin != 16 or cout != 16 or g.ntaps != 3 or not _plain_s1(g, 16):
        return False
    if any(g.src[t] for t in range(3)):
        return False
    return g.N * g.HO * g.WO * 16 * 4 < (1 << 31)


def wgrad2_eligible(g, cin, cout, want_bias):
    """-> index of the tap without a shift, -1 when the streaming kernels do not cover the launch."""
    if cin != cout or cin not in (64, 128) or g.ntaps not in (3, 4):
        return -1
    if not _plain_s1(g, cin) or (g.WO & 15):
        return -1
    if g.N * g.HO * g.WO * cin * 4 >= (1 << 31):
        return -1
    center = -1
    for t in range(g.ntaps):
        if g.src[t] and g.in_pitch[1] != cin:
            return -1
        if g.dh[t] and g.dw[t]:
            return -1
        if not g.dh[t] and not g.dw[t] and center < 0:
            center = t
    if want_bias and center < 0:
        return -1
    return max(center, 0)


def wgradw_eligible(g, cin, cout):
    """-> (dilation, axis) of a 3-tap conv with complete pairs (axis 1: taps along W), else (0, None)."""
    if g.ntaps != 3 or wgrad2_eligible(g, cin, cout, False) < 0:
        return 0, None
    d, ax, idx = 0, -1, [-1, -1, -1]
    for t in range(3):
        if g.src[t] != g.src[0] or (g.dh[t] and g.dw[t]):
            return 0, None
        o = g.dh[t] if g.dh[t] else g.dw[t]
        if o == 0:
            idx[1] = t
            continue
        a = 1 if g.dw[t] else 0
        if ax >= 0 and a != ax:
            return 0, None
        ax = a
        if d and abs(o) != d:
            return 0, None
        d = abs(o)
        idx[0 if o < 0 else 2] = t
    if d <= 0 or min(idx) < 0:
        return 0, None
    if ax == 0:
        if g.HO % (2 * d):
            return 0, None
    elif (g.WO & 31) or d not in (1, 2, 4, 8, 16):
        return 0, None
    return d, ax


# ------------------------------------------------------------------------------------------------
# the four chunk plans
# ------------------------------------------------------------------------------------------------
def wg_cfg(cout, cin):
    """WgCfg of the tile configuration that serves a (cout, cin) conv."""
    co_t, ci_t, stem = WG_CONFIGS[(cout, cin)]
    co_p, ci_p = _r16(co_t), (32 if stem else _r16(ci_t))
    ps = 256 if co_p * ci_p <= 256 else (128 if co_p * ci_p <= 1024 else 64)
    mt, nt = co_p // 16, ci_p // 16
    return SimpleNamespace(CO_T=co_t, CI_T=ci_t, STEM=stem, CO_P=co_p, CI_P=ci_p, PS=ps,
                           nz_co=cdiv(cout, co_t), nz_ci=1 if stem else cdiv(cin, ci_t),
                           PIPE=(not stem) and co_t % 4 == 0,
                           TILE_SPLIT=mt % 2 == 0 and nt % 2 == 0 and mt * nt >= 16)


def lds_plan(npix, ntaps, cout, cin):
    """make_plan + ws_need of launch_wgrad<CO_T, CI_T, STEM>."""
    c = wg_cfg(cout, cin)
    ntaps = 1 if c.STEM else ntaps
    nz = c.nz_co * c.nz_ci
    stages = cdiv(npix, c.PS)
    nch = min(max(TARGET // (ntaps * nz), 1), stages)
    per = cdiv(stages, nch)
    chunks = cdiv(stages, per)
    ws = (chunks * ntaps * nz * c.CO_P * c.CI_P + chunks * c.nz_co * c.CO_P) * 4
    return SimpleNamespace(family="wgrad", sub=f"wgrad_kernel<{c.CO_T},{c.CI_T},{str(c.STEM).lower()}>", cfg=c,
                           unit="stages", unit_px=c.PS, total=stages, per_chunk=per, chunks=chunks, empty=0,
                           last_chunk=stages - (chunks - 1) * per, last_px=npix - (stages - 1) * c.PS,
                           ntaps=ntaps, nz=nz, ws_bytes=ws, row_cross=(), image_cross=())


def lds_chunks_from_workspace(nbytes, ntaps, cout, cin):
    """nchunks of an LDS-tiled launch, recovered from what mdil_wgrad_workspace asks for."""
    c = wg_cfg(cout, cin)
    ntaps = 1 if c.STEM else ntaps
    per_chunk = (ntaps * c.nz_co * c.nz_ci * c.CO_P * c.CI_P + c.nz_co * c.CO_P) * 4
    assert nbytes % per_chunk == 0, (nbytes, per_chunk)
    return nbytes // per_chunk


def stream_plan(sub, C, ntaps, N, H, W):
    """launch_wgrad2 (sub "wgrad2") / launch_wgradw (sub "wgradw": taps along H, work item = 16 row pairs;
    "wgradx": taps along W, work item = 32 pixels of a row).  A chunk is the run of ``per_chunk`` work items
    one wave streams; ``row_cross`` / ``image_cross`` list the chunks whose items lie in two (pair) rows /
    two images, i.e. whose loop runs advance() through a row end / an image end and rebuilds descriptors."""
    nz = (C // 64) ** 2
    if sub == "wgradw":
        per_row, rows, cpw, px = W >> 4, H >> 1, CPW_W, 32
    elif sub == "wgradx":
        per_row, rows, cpw, px = W >> 5, H, CPW_W, 32
    else:
        per_row, rows, cpw, px = W >> 4, H, CPW[(C, ntaps)], 16
    items = N * rows * per_row
    groups = min(STREAM_GROUPS // nz, cdiv(items, cpw))
    if nz > 1:
        groups = (groups + 7) // 8 * 8
    per = cdiv(items, groups * cpw)
    used = cdiv(items, per)
    span = lambda c, unit: (c * per) // unit != (min((c + 1) * per, items) - 1) // unit
    name = f"wgrad2_kernel<{C},{ntaps},{cpw}>" if sub == "wgrad2" else f"{sub}_kernel<{C}>"
    return SimpleNamespace(family="wgradw" if sub != "wgrad2" else "wgrad2", sub=name, unit="quads", unit_px=px,
                           total=items, per_chunk=per, chunks=groups * cpw, groups=groups, used=used,
                           empty=groups * cpw - used, short=1 if items % per else 0,
                           per_row=per_row, per_image=rows * per_row,
                           row_cross=tuple(c for c in range(used) if span(c, per_row)),
                           image_cross=tuple(c for c in range(used) if span(c, rows * per_row)))


def wg16_plan(npix):
    """launch_wgrad16: a chunk is a wave here (4 per work-group), ``empty`` the waves wholly past the end."""
    tiles = cdiv(npix, 16)
    groups = max(1, min(WG16_CHUNKS, cdiv(tiles, 4)))
    per = cdiv(tiles, groups * 4)
    used = cdiv(tiles, per)
    return SimpleNamespace(family="wgrad2", sub="wgrad16_kernel", unit="tiles", unit_px=16, total=tiles,
                           per_chunk=per, chunks=groups * 4, groups=groups, used=used, empty=groups * 4 - used,
                           last_px=npix - (tiles - 1) * 16, row_cross=(), image_cross=())


def plan_for(g, cin, cout, want_bias=True):
    """wgrad_impl's dispatch: the plan of the kernel that takes the launch.  ``family`` is the name the
    launch profiler reports (ops._PROF_WGRAD: wgrad16 shares "wgrad2"), ``sub`` the kernel."""
    if wgrad16_eligible(g, cin, cout):
        return wg16_plan(g.N * g.HO * g.WO)
    if wgrad2_eligible(g, cin, cout, want_bias) >= 0:
        d, ax = wgradw_eligible(g, cin, cout)
        if d:
            return stream_plan("wgradx" if ax else "wgradw", cin, 3, g.N, g.HO, g.WO)
        return stream_plan("wgrad2", cin, g.ntaps, g.N, g.HO, g.WO)
    return lds_plan(g.N * g.HO * g.WO, g.ntaps, cout, cin)


def plan_line(name, p):
    return (f"{name}: family {p.family} ({p.sub}), {p.chunks} chunks, {p.per_chunk} {p.unit} per chunk "
            f"({p.total} in all), {p.empty} empty chunks, row/image crossings {len(p.row_cross)}/{len(p.image_cross)}")


def second_unit_pixel(p, g):
    """(n, h, w) in the gout tensor of the first pixel of chunk 0's SECOND stage / quad / tile."""
    if p.sub.startswith("wgradw"):
        per_row = g.WO >> 4
        pr, w0 = 1 // per_row, (1 % per_row) << 4
        d = max(abs(g.dh[t]) for t in range(3))
        rr = pr % (g.HO >> 1)
        return pr // (g.HO >> 1), 2 * d * (rr // d) + rr % d, w0
    P = p.unit_px
    n, r = divmod(P, g.HO * g.WO)
    ho, wo = divmod(r, g.WO)
    return n, ho * g.ohs + g.oho, wo * g.ows + g.owo


# ------------------------------------------------------------------------------------------------
# draws
# ------------------------------------------------------------------------------------------------
INT_VALUES = (-3.0, -2.0, -1.0, 1.0, 2.0, 3.0)


def draw_int(shape, seed):
    """fp32, values in {-3, -2, -1, 1, 2, 3}: an omitted, doubled or mispaired pixel moves every element
    of the weight gradient it touches (no factor is ever 0)."""
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(INT_VALUES)[torch.randint(0, 6, tuple(shape), generator=g)]


def draw_normal(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def exact_budget(npix):
    """Largest |partial sum| any kernel can form: 36 = max |(dy0 + dy1)(d1 + d2)| of the Winograd operands."""
    return 36 * npix


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
def _case(name, kind, cin, cout, H, W, d=1, axis=None, family="wgrad", sub=None, cross=None, N=2):
    return SimpleNamespace(name=name, kind=kind, cin=cin, cout=cout, H=H, W=W, d=d, axis=axis, N=N,
                           family=family, sub=sub, cross=cross)


# kind: stem / down (DownFn, cout = all channels of the concatenated output), up (UpFn), out (OutFn),
# conv3 (a 3-tap C -> C conv built as test_tapconv_factorised does), adapter (the 1x3 + 1x1-adapter launch of
# NbFn's backward).  H x W is the size of the layer's INPUT.  cross: the streaming cases that must hold a
# chunk crossing a row end ("r") and an image end ("i").
CASES = [
    _case("stem", "stem", 3, 16, 444, 450),
    _case("down16-64", "down", 16, 64, 162, 146),
    _case("down64-128", "down", 64, 128, 106, 112),
    _case("up128-64", "up", 128, 64, 112, 111),
    _case("up64-16", "up", 64, 16, 222, 222),
    _case("head20", "out", 16, 20, 222, 222),
    _case("head27", "out", 16, 27, 222, 222),
    _case("wgrad2<64,3> 3x1 d1", "conv3", 64, 64, 67, 80, 1, "h", "wgrad2", "wgrad2_kernel<64,3,2>", "ri"),
    _case("wgrad2<64,3> 1x3 d2", "conv3", 64, 64, 67, 80, 2, "w", "wgrad2", "wgrad2_kernel<64,3,2>", "ri"),
    _case("wgrad2<64,4> 1x3 d2 + adapter", "adapter", 64, 64, 67, 80, 2, "w", "wgrad2", "wgrad2_kernel<64,4,2>", "ri"),
    _case("wgradw<64> 3x1 d1", "conv3", 64, 64, 134, 80, 1, "h", "wgradw", "wgradw_kernel<64>", "ri"),
    _case("wgradx<64> 1x3 d1", "conv3", 64, 64, 91, 96, 1, "w", "wgradw", "wgradx_kernel<64>", "ri"),
    _case("wgrad2<128,3> 3x1 d2", "conv3", 128, 128, 45, 48, 2, "h", "wgrad2", "wgrad2_kernel<128,3,4>", "ri"),
    _case("wgrad2<128,4> 1x3 d4 + adapter", "adapter", 128, 128, 23, 48, 4, "w", "wgrad2", "wgrad2_kernel<128,4,2>", "ri"),
    _case("wgradw<128> 3x1 d1", "conv3", 128, 128, 46, 48, 1, "h", "wgradw", "wgradw_kernel<128>", "ri"),
    # H % 2d == 0 makes the pair-quads of an image an even number: a dilated wgradw<128> chunk of two never
    # crosses an image end.  88 x 48 gives three quads per chunk = exactly one pair row (carried state, no
    # crossing); 80 x 48 gives two per chunk and three per row, so chunks cross the row ends and the q wrap
    _case("wgradw<128> 3x1 d4 88x48", "conv3", 128, 128, 88, 48, 4, "h", "wgradw", "wgradw_kernel<128>", ""),
    _case("wgradw<128> 3x1 d4 80x48", "conv3", 128, 128, 80, 48, 4, "h", "wgradw", "wgradw_kernel<128>", "r"),
    _case("wgradx<128> 1x3 d8", "conv3", 128, 128, 23, 160, 8, "w", "wgradw", "wgradx_kernel<128>", "ri"),
    _case("wgrad16 3x1", "conv3", 16, 16, 129, 255, 1, "h", "wgrad2", "wgrad16_kernel"),
    _case("wgrad16 1x3", "conv3", 16, 16, 129, 255, 1, "w", "wgrad2", "wgrad16_kernel"),
]
CASE_IDS = [c.name.replace(" ", "_") for c in CASES]

_PAR = {0: [(1, 0)], 1: [(0, 1), (2, 0)]}       # parity classes of a stride-2 transposed conv (ops._PAR)


def taps3(d, axis):
    return [((k - 1) * d, 0, 0) for k in range(3)] if axis == "h" else [(0, (k - 1) * d, 0) for k in range(3)]


def host_launches(c):
    """-> [(geometry, cin, cout)] of the weight-gradient launches the product makes for the case, built on
    the host as ops.DownFn / UpFn / OutFn / NbFn build them (the GPU test takes them from the product by
    capture and checks the same preconditions on those)."""
    N, H, W = c.N, c.H, c.W
    if c.kind == "stem":
        return [(geom(N, H // 2, W // 2, H, W, [(0, 0, 0)], 3, H // 2, W // 2, c.cout, ihs=2, iws=2), 27, c.cout - 3)]
    if c.kind == "down":
        taps = [(kh - 1, kw - 1, 0) for kh in range(3) for kw in range(3)]
        return [(geom(N, H // 2, W // 2, H, W, taps, c.cin, H // 2, W // 2, c.cout, ihs=2, iws=2), c.cin, c.cout - c.cin)]
    if c.kind == "up":
        out = []
        for a in (0, 1):
            for b in (0, 1):
                taps = [(dh, dw, 0) for _, dh in _PAR[a] for _, dw in _PAR[b]]
                out.append((geom(N, H, W, H, W, taps, c.cin, 2 * H, 2 * W, c.cout, ohs=2, oho=a, ows=2, owo=b),
                            c.cin, c.cout))
        return out
    if c.kind == "out":
        P = (c.cout + 3) // 4 * 4
        return [(geom(N, H, W, H, W, [(0, 0, 0)], c.cin, 2 * H, 2 * W, P, ohs=2, oho=a, ows=2, owo=b), c.cin, c.cout)
                for a in (0, 1) for b in (0, 1)]
    taps = taps3(c.d, c.axis) + ([(0, 0, 1)] if c.kind == "adapter" else [])
    return [(geom(N, H, W, H, W, taps, c.cin, H, W, c.cin), c.cin, c.cin)]


def gout_shape(c):
    """NHWC shape of the gout tensor the case's launches read, and the channels the launches own."""
    if c.kind in ("stem", "down"):
        return (c.N, c.H // 2, c.W // 2, c.cout), c.cout - c.cin
    if c.kind == "up":
        return (c.N, 2 * c.H, 2 * c.W, c.cout), c.cout
    if c.kind == "out":
        return (c.N, 2 * c.H, 2 * c.W, (c.cout + 3) // 4 * 4), c.cout
    return (c.N, c.H, c.W, c.cin), c.cin


def weight_shapes(c):
    """-> [(weight shape, bias length)]: the layer's parameters in PyTorch layout (adapter: 1x3 conv, 1x1)."""
    if c.kind in ("stem", "down"):
        return [((c.cout - c.cin, c.cin, 3, 3), c.cout - c.cin)]
    if c.kind == "up":
        return [((c.cin, c.cout, 3, 3), c.cout)]
    if c.kind == "out":
        return [((c.cin, c.cout, 2, 2), c.cout)]
    k = (3, 1) if c.axis == "h" else (1, 3)
    return [((c.cin, c.cin) + k, c.cin)] + ([((c.cin, c.cin, 1, 1), c.cin)] if c.kind == "adapter" else [])


def draw_case(c, draw, seed=0):
    """-> dict of NHWC fp32 operands: x (layer input; adapter: the 1x3 conv's input), x2 (adapter's input),
    gout (owned channels only, [N, OH, OW, owned]), w / b (+ w2 / b2), r (what the dgrad accumulates onto)."""
    (gs, owned) = gout_shape(c)
    t = {"x": draw((c.N, c.H, c.W, c.cin), seed + 1), "gout": draw(gs[:3] + (owned,), seed + 2)}
    for i, (ws, nb) in enumerate(weight_shapes(c)):
        sfx = "" if i == 0 else "2"
        t["w" + sfx], t["b" + sfx] = draw(ws, seed + 3 + 2 * i), draw((nb,), seed + 4 + 2 * i)
    if c.kind == "adapter":
        t["x2"] = draw((c.N, c.H, c.W, c.cin), seed + 7)
    if c.kind == "down":
        t["r"] = draw((c.N, c.H, c.W, c.cin), seed + 8)
    return t


# ------------------------------------------------------------------------------------------------
# float64 reference: the layer's own definition through autograd
# ------------------------------------------------------------------------------------------------
def _nchw(t):
    return t.permute(0, 3, 1, 2).double()


def layer_forward(c, x, w, b, x2=None, w2=None, b2=None):
    """The layer of the case on float64 NCHW tensors."""
    if c.kind in ("stem", "down"):
        return F.conv2d(x, w, b, stride=2, padding=1)
    if c.kind == "up":
        return F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)
    if c.kind == "out":
        return F.conv_transpose2d(x, w, b, stride=2)
    pad, dil = ((c.d, 0), (c.d, 1)) if c.axis == "h" else ((0, c.d), (1, c.d))
    y = F.conv2d(x, w, b, padding=pad, dilation=dil)
    if c.kind == "adapter":
        y = y + F.conv2d(x2, w2, b2)
    return y


def reference(c, t, gout=None, with_input=False):
    """float64 gradients of the case's layer for the operands ``t`` (draw_case): dict with dw, db (+ dw2,
    db2), and with ``with_input`` also out (NHWC forward output) and gx (NHWC input gradient).  ``gout``
    replaces t["gout"]."""
    gout = t["gout"] if gout is None else gout
    x = _nchw(t["x"]).requires_grad_(with_input)
    names = ["w", "b"] + (["w2", "b2"] if "w2" in t else [])
    p = {n: t[n].double().requires_grad_(True) for n in names}
    x2 = _nchw(t["x2"]) if "x2" in t else None
    y = layer_forward(c, x, p["w"], p["b"], x2, p.get("w2"), p.get("b2"))
    grads = torch.autograd.grad(y, [p[n] for n in names] + ([x] if with_input else []), _nchw(gout))
    res = {"d" + n: g for n, g in zip(names, grads)}
    if with_input:
        res["out"] = y.detach().permute(0, 2, 3, 1).contiguous()
        res["gx"] = grads[-1].permute(0, 2, 3, 1).contiguous()
    return res


def taps_inside(c, n, oh, ow):
    """-> bool [KH, KW]: the kernel taps whose input pixel lies inside the image for gout pixel (oh, ow)."""
    (ws, _) = weight_shapes(c)[0]
    kh_n, kw_n = ws[2], ws[3]
    ok = torch.zeros(kh_n, kw_n, dtype=torch.bool)
    for kh in range(kh_n):
        for kw in range(kw_n):
            if c.kind in ("stem", "down"):
                ih, iw, hit = 2 * oh - 1 + kh, 2 * ow - 1 + kw, True
            elif c.kind == "up":           # o = 2 i - 1 + k
                ih, iw = (oh + 1 - kh) // 2, (ow + 1 - kw) // 2
                hit = (oh + 1 - kh) % 2 == 0 and (ow + 1 - kw) % 2 == 0
            elif c.kind == "out":          # o = 2 i + k
                ih, iw, hit = (oh - kh) // 2, (ow - kw) // 2, (oh - kh) % 2 == 0 and (ow - kw) % 2 == 0
            else:
                ih = oh + ((kh - 1) * c.d if c.axis == "h" else 0)
                iw = ow + ((kw - 1) * c.d if c.axis == "w" else 0)
                hit = True
            ok[kh, kw] = hit and 0 <= ih < c.H and 0 <= iw < c.W
    return ok


def mismatch_report(what, got, want, show=4):
    """'' when equal, else the number of wrong elements per kernel tap and the first few got - want."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    if got.shape != want.shape:
        return f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    bad = got != want
    if not bad.any():
        return ""
    diff = (got - want)[bad]
    msg = f"{what}: {int(bad.sum())}/{bad.numel()} elements differ"
    if got.dim() == 4 and got.shape[2] * got.shape[3] <= 9:
        msg += "; per tap " + str(bad.reshape(got.shape[0], got.shape[1], -1).sum((0, 1)).tolist())
    idx = torch.nonzero(bad)[:show].tolist()
    return msg + f"; first at {idx}: got - want = {diff[:show].tolist()}"
