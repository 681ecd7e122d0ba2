"""The contract of ``mdil_tapconv`` (include/mdil_hip.h: geometry + seven-stage epilogue) as a float64
reference, the draws, the case table and the host mirror of the router (csrc/tapconv.hip::mdil_tapconv),
for tests/test_tapconv_contract_cpu.py and tests/test_tapconv_contract_gpu.py.  CPU torch only.

The suite otherwise meets this entry point only where the model calls it: a bias, at most a residual,
out_coff = 0, one pitch.  Here every route behind it -- the 14 LDS-tiled ``tapconv_kernel`` instantiations,
``c16conv``, the direct ``sconv`` form, Winograd F(2,3) ``wconv`` and F(4,3) ``w4conv`` -- runs the epilogue
forms E0 .. E10 below, in the geometries the product builds (part A), on stride-1 C -> C shapes (part B) and
once through its own route and once forced onto the LDS-tiled kernel (part C).

What "exact" rests on: with operands in {-3 .. 3} \\ {0}, scale in {-2, -1, 1, 2} and integer shift / residual
every product, partial sum and epilogue stage is an integer below 2^23 (``exact_budget``), hence exact in fp32
in ANY summation order and with or without fused multiply-adds.  F(2,3) only adds the constant 1/2 (its
transformed weights are multiples of 1/2, csrc/wconv.hip: ``(s02 +- g1) * 0.5f``), so it stays exact; F(4,3)
divides by 6 and 24 and is compared within the fp32 tolerance instead.  The HIP output must EQUAL the
reference over the WHOLE output buffer, which is wider than what a launch owns and pre-filled with a
sentinel: values and write footprint are proven together."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from tests import conditioning_cases as CC
from tests import wgrad_chunks as WC

SENTINEL = -7777.25          # not an integer: no exact result of the integer draw can equal it
FOREIGN = 1000.0             # input channels past cin (concat rows, the pad entry of 28-float rows)
ROUTES = ("tapconv", "c16conv", "sconv", "wconv", "w4conv")        # ops._PROF_CONV's names

# ------------------------------------------------------------------------------------------------
# constants copied from the sources (pinned against their text in tests/test_tapconv_contract_cpu.py)
# ------------------------------------------------------------------------------------------------
MDIL_WG = 256
# csrc/tapconv.hip:701-714, the TC(cin, cout, BM, stem) lines of mdil_tapconv
TC_LINES = ((64, 64, 128, False), (128, 128, 64, False), (16, 16, 128, False), (16, 48, 128, False),
            (48, 16, 128, False), (128, 64, 128, False), (64, 128, 64, False), (64, 16, 128, False),
            (16, 64, 128, False), (16, 20, 128, False), (20, 16, 128, False), (16, 27, 128, False),
            (27, 16, 128, False), (27, 13, 128, True))
C16_TN, C16_WAVES = 2, 4     # csrc/c16conv.hip:24-29: 16-pixel groups per wave tile, waves per work-group
C16_PXT = 16 * C16_TN


def cdiv(a, b):
    return -(-a // b)


def _r4(v):
    return (v + 3) // 4 * 4


def _r16(v):
    return (v + 15) // 16 * 16


def epilogue_path(cout):
    """Which of tapconv_kernel's three epilogue code paths an instantiation compiles (csrc/tapconv.hip:316,
    324, 370-378, 405): "scalar" (COUT % 4 != 0), "hoisted" (QINV: MDIL_WG % (COUT / 4) == 0, the per-thread
    bias / scale / shift vectors fetched before the transpose) or "per-iteration" loads."""
    if cout % 4:
        return "scalar"
    return "hoisted" if MDIL_WG % (cout // 4) == 0 else "per-iteration"


def lds_tiles(npix, bm):
    """Pixels of each work-group tile of an LDS-tiled launch (launch_tapconv: grid = cdiv(npix, BM))."""
    return [min(bm, npix - t * bm) for t in range(cdiv(npix, bm))]


def c16_plan(npix):
    """mdil_c16conv + launch_c16 (csrc/c16conv.hip:52-60, 153, 195-197): wave tiles, work-groups that own
    tiles, the grid padded to a multiple of 8, the XCD-major walk blockIdx -> work-group, and the valid
    pixels of the last tile's 16-pixel groups."""
    tiles = cdiv(npix, C16_PXT)
    nwg = cdiv(tiles, C16_WAVES)
    grid = (nwg + 7) // 8 * 8
    per = grid >> 3
    walk = [(b & 7) * per + (b >> 3) for b in range(grid)]
    p0 = (tiles - 1) * C16_PXT
    last = [max(0, min(16, npix - p0 - 16 * n)) for n in range(C16_TN)]
    return SimpleNamespace(tiles=tiles, nwg=nwg, grid=grid, walk=walk, empty=grid - nwg, last_groups=last)


# ------------------------------------------------------------------------------------------------
# the epilogue forms
# ------------------------------------------------------------------------------------------------
# "inplace": res aliases out (DownFn.backward's use): the buffer is pre-filled with the residual
FORMS = {
    "E0": (),
    "E1": ("bias",),
    "E2": ("bias", "bias2"),
    "E3": ("bias", "scale", "relu"),
    "E4": ("bias", "bias2", "scale", "res", "relu"),
    "E5": ("gate",),
    "E6": ("res",),
    "E7": ("res", "res_gate"),
    "E8": ("res", "gate"),
    "E9": ("bias", "relu", "gate"),
    "E10": ("res", "inplace"),
}
ALL_FORMS = tuple(FORMS)
BASE_FORMS = ("E0", "E1", "E3", "E5", "E7", "E9")


# ------------------------------------------------------------------------------------------------
# host mirror of the router
# ------------------------------------------------------------------------------------------------
def _plain_s1(g, c):
    """The geometry test shared by mdil_sconv_covers (csrc/sconv.hip:599-604) and mdil_c16conv_covers
    (csrc/c16conv.hip:167-172)."""
    if (g.ihs != 1 or g.iws != 1 or g.ohs != 1 or g.ows != 1 or g.oho or g.owo or g.HI != g.HO or
            g.WI != g.WO or g.OH != g.HO or g.OW != g.WO or g.out_coff or g.out_pitch != c or g.in_pitch[0] != c):
        return False
    return not any(g.src[t] and g.in_pitch[1] != c for t in range(g.ntaps))


def sconv_covers(g, cin, cout):
    """csrc/sconv.hip:596-606."""
    if cin != cout or cin not in (64, 128) or g.ntaps not in (3, 4):
        return False
    return _plain_s1(g, cin) and g.N * g.HO * g.WO * cin * 4 < (1 << 31)


def c16conv_covers(g, cin, cout):
    """csrc/c16conv.hip:165-175 without its epilogue test (``route`` applies that)."""
    if cin != 16 or cout != 16 or g.ntaps != 3:
        return False
    return _plain_s1(g, 16) and g.N * g.HO * g.WO * 16 * 4 < (1 << 31)


def wconv_plan(g, mult):
    """csrc/wino.h:123-175: a 3-tap conv along one axis (+ a centre tap from the other source) whose axis
    length holds complete groups of ``mult`` outputs (2: F(2,3), 4: F(4,3))."""
    ad = -1
    if g.ntaps == 4:
        s1 = [t for t in range(4) if g.src[t]]
        s0 = [t for t in range(4) if not g.src[t]]
        ad = s1[0] if len(s1) == 1 else (s0[0] if len(s0) == 1 else -1)
        if ad < 0 or g.dh[ad] or g.dw[ad]:
            return False
    elif g.ntaps != 3:
        return False
    conv = [t for t in range(g.ntaps) if t != ad]
    axis, delta, seen = -1, 0, set()
    for t in conv:
        if g.src[t] != g.src[conv[0]] or (g.dh[t] and g.dw[t]):
            return False
        if not g.dh[t] and not g.dw[t]:
            seen.add(0)
            continue
        ax, off = (1, g.dw[t]) if g.dw[t] else (0, g.dh[t])
        if (axis >= 0 and ax != axis) or (delta and abs(off) != delta):
            return False
        axis, delta = ax, abs(off)
        seen.add(1 if off > 0 else -1)
    if axis < 0 or delta <= 0 or seen != {-1, 0, 1}:
        return False
    return (g.WO if axis else g.HO) % (mult * delta) == 0


def route(g, cin, cout, form):
    """The kernel family that takes an ``mdil_tapconv`` call (csrc/tapconv.hip:684-698): the streaming
    kernels and c16conv keep ONE register set for "residual or gate" and decline both at once
    (csrc/sconv.hip:609, csrc/c16conv.hip:173); C = 64 with the adapter tap stays on F(2,3)
    (csrc/w4conv.hip:750)."""
    both = "res" in FORMS[form] and "gate" in FORMS[form]
    if sconv_covers(g, cin, cout) and not both:
        if wconv_plan(g, 4) and not (cin == 64 and g.ntaps == 4):
            return "w4conv"
        return "wconv" if wconv_plan(g, 2) else "sconv"
    if c16conv_covers(g, cin, cout) and not both:
        return "c16conv"
    return "tapconv"


# ------------------------------------------------------------------------------------------------
# draws
# ------------------------------------------------------------------------------------------------
SCALE_VALUES = (-2.0, -1.0, 1.0, 2.0)
GATE_VALUES = (-2.0, -1.0, -0.0, 0.0, 1.0, 2.0)


def _pick(values, shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(values)[torch.randint(0, len(values), tuple(shape), generator=g)]


def draw_scale(shape, seed):
    return _pick(SCALE_VALUES, shape, seed)


def draw_gate(shape, seed):
    """Both zeros are drawn: a gate applied with ``>=`` instead of ``>`` opens on either."""
    return _pick(GATE_VALUES, shape, seed)


def has_both_zeros(t):
    z = t == 0
    return bool((z & torch.signbit(t)).any()) and bool((z & ~torch.signbit(t)).any())


def exact_budget(c):
    """Largest magnitude any stage of the integer draw can reach: |acc| <= 3 * 3 * ntaps * cin, plus the
    two biases, times |scale| <= 2, plus |shift| and |res|."""
    return (3 * 3 * c.ref_ntaps * c.ref_cin + 3 + 3) * 2 + 3 + 3


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def epilogue(bias=None, scale=None, shift=None, res=None, res_gate=None, gate=None, relu=False, bias2=None):
    """The fields of mdil_epilogue, in the header's order."""
    return SimpleNamespace(bias=bias, scale=scale, shift=shift, res=res, res_gate=res_gate, gate=gate, relu=relu,
                           bias2=bias2)


def _out_index(g):
    oh = torch.arange(g.HO) * g.ohs + g.oho
    ow = torch.arange(g.WO) * g.ows + g.owo
    return oh[:, None], ow[None, :]


def conv_acc(g, cin, cout, in0, in1, W):
    """float64 [N, HO, WO, cout]: sum_t sum_ci in_src[t][n, ho ihs + dh[t], wo iws + dw[t], ci] W[t][co][ci],
    out-of-range input pixels reading as zero.  in0 / in1: [N, HI, WI, >= cin] whose pixel stride is the
    geometry's in_pitch (a view into a wider buffer is passed as that view); W: [ntaps][cout][cin]."""
    ins = (in0, in1)
    acc = torch.zeros(g.N, g.HO, g.WO, cout, dtype=torch.float64)
    for t in range(g.ntaps):
        x = ins[g.src[t]]
        assert tuple(x.shape[:3]) == (g.N, g.HI, g.WI) and x.shape[3] >= cin and x.stride(3) == 1
        assert x.stride(2) == g.in_pitch[g.src[t]], (x.stride(), g.in_pitch)
        hi = torch.arange(g.HO) * g.ihs + g.dh[t]
        wi = torch.arange(g.WO) * g.iws + g.dw[t]
        ok = ((hi >= 0) & (hi < g.HI))[:, None] & ((wi >= 0) & (wi < g.WI))[None, :]
        xs = x[:, hi.clamp(0, g.HI - 1)[:, None], wi.clamp(0, g.WI - 1)[None, :], :cin].double()
        xs = torch.where(ok[None, :, :, None], xs, torch.zeros((), dtype=torch.float64))
        acc += xs @ W[t].double().t()
    return acc


def apply_epilogue(g, cout, acc, epi, out_before):
    """The header's epilogue on ``acc`` [N, HO, WO, cout], stored into a copy of the whole output buffer
    [N, OH, OW, out_pitch] at (ho ohs + oho, wo ows + owo), channels [out_coff, out_coff + cout); res,
    res_gate and gate are addressed like out, the gates are strict > 0."""
    assert tuple(out_before.shape) == (g.N, g.OH, g.OW, g.out_pitch)
    oh, ow = _out_index(g)
    ch = slice(g.out_coff, g.out_coff + cout)
    at = lambda t: t[:, oh, ow, ch].double()
    v = acc.clone()
    if epi.bias is not None:
        v = v + epi.bias.double()
    if epi.bias2 is not None:
        v = v + epi.bias2.double()
    assert (epi.scale is None) == (epi.shift is None)
    if epi.scale is not None:
        v = v * epi.scale.double() + epi.shift.double()
    if epi.res is not None:
        r = at(epi.res)
        if epi.res_gate is not None:
            r = torch.where(at(epi.res_gate) > 0, r, torch.zeros_like(r))
        v = v + r
    if epi.relu:
        v = v.clamp_min(0.0)
    if epi.gate is not None:
        v = torch.where(at(epi.gate) > 0, v, torch.zeros_like(v))
    out = out_before.double().clone()
    out[:, oh, ow, ch] = v
    return out


def reference(g, cin, cout, in0, in1, W, epi, out_before):
    """float64 ``mdil_tapconv``: -> the whole output buffer after the call; every element the formula does
    not write keeps its old value."""
    return apply_epilogue(g, cout, conv_acc(g, cin, cout, in0, in1, W), epi, out_before)


def owned_mask(g, cout):
    """bool [N, OH, OW, out_pitch]: the elements a launch writes."""
    m = torch.zeros(g.N, g.OH, g.OW, g.out_pitch, dtype=torch.bool)
    oh, ow = _out_index(g)
    m[:, oh, ow, g.out_coff:g.out_coff + cout] = True
    return m


# ------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------
GRID = (3, 9, 11)            # part A: 297 pixels -> 128 / 128 / 41 at BM = 128, five tiles at BM = 64
IMAGE_ENDS = (99, 198)


def _s2_taps():
    return [(kh - 1, kw - 1, 0) for kh in range(3) for kw in range(3)]


def _class_taps(a, b):
    """ops._class_taps: taps and kernel positions kh * 3 + kw of output parity class (a, b)."""
    taps = [(dh, dw, 0) for _, dh in WC._PAR[a] for _, dw in WC._PAR[b]]
    return taps, [kh * 3 + kw for kh, _ in WC._PAR[a] for kw, _ in WC._PAR[b]]


def _mk(name, part, gargs, gkw, cin, cout, forms, layer, parity=False, in1=None, ref=None, expect=None, exact=True):
    """gargs / gkw: the arguments of wgrad_chunks.geom == ops.make_geom.  ref: (gargs, gkw, cin) of the
    geometry the reference uses when it is not the launch's (the stem's im2col-on-load).  in1: None,
    "plain" ([N, H, W, C]) or "wide" (channels 64.. of a 128-float row).  layer: how torch computes the same
    convolution (``layer_acc``).  expect: the producer named by the table the shape was taken from."""
    g = WC.geom(*gargs, **gkw)
    rg, rcin = (WC.geom(*ref[0], **ref[1]), ref[2]) if ref else (g, cin)
    return SimpleNamespace(name=name, part=part, gargs=gargs, gkw=gkw, g=g, cin=cin, cout=cout, forms=tuple(forms),
                           layer=layer, parity=parity, in1=in1, ref_g=rg, ref_cin=rcin, ref_ntaps=rg.ntaps,
                           stem=ref is not None, expect=expect)


def _part_a():
    N, HO, WO = GRID
    H2, W2 = 2 * HO, 2 * WO
    s2 = dict(ihs=2, iws=2)
    out = []
    # stride-2 3x3 forward into the concat row (ops.DownFn.forward); conv channels first, pooled ones behind
    for cin, cc in ((16, 48), (64, 64)):
        out.append(_mk(f"down{cin}-{cc}", "A", (N, HO, WO, H2, W2, _s2_taps(), cin, HO, WO, cin + cc), s2, cin, cc,
                       BASE_FORMS, ("conv_s2", 3)))
    out.append(_mk("down16-48-coff4", "A", (N, HO, WO, H2, W2, _s2_taps(), 16, HO, WO, 72), dict(s2, coff=4), 16, 48,
                   BASE_FORMS, ("conv_s2", 3)))
    for name, pitch, coff in (("stem27-13", 16, 0), ("stem27-13-coff4", 24, 4)):
        out.append(_mk(name, "A", (N, HO, WO, H2, W2, [(0, 0, 0)], 3, HO, WO, pitch), dict(s2, coff=coff), 27, 13,
                       BASE_FORMS, ("conv_s2", 3),
                       ref=((N, HO, WO, H2, W2, _s2_taps(), 3, HO, WO, pitch), dict(s2, coff=coff), 3)))
    # parity classes: transposed conv forward (ops.UpFn.forward), stride-2 dgrad (ops.DownFn.backward: the
    # input is the concat row), 2x2 head forward (ops.OutFn.forward's per-class route)
    for a in (0, 1):
        for b in (0, 1):
            taps, ktap = _class_taps(a, b)
            cls = dict(ohs=2, oho=a, ows=2, owo=b)
            for cin, cout in ((128, 64), (64, 16)):
                out.append(_mk(f"up{cin}-{cout}-class{a}{b}", "A", (N, HO, WO, HO, WO, taps, cin, H2, W2, cout), cls,
                               cin, cout, BASE_FORMS + ("E10",), ("convT_class", a, b, ktap), parity=True))
            for cc, pitch, cin in ((48, 64, 16), (64, 128, 64)):
                out.append(_mk(f"ddown{cc}-{cin}-class{a}{b}", "A", (N, HO, WO, HO, WO, taps, pitch, H2, W2, cin), cls,
                               cc, cin, BASE_FORMS + ("E6", "E10"), ("convT_class", a, b, ktap), parity=True))
            for nc in (20, 27):
                out.append(_mk(f"head16-{nc}-class{a}{b}", "A", (N, HO, WO, HO, WO, [(0, 0, 0)], 16, H2, W2, _r4(nc)),
                               cls, 16, nc, BASE_FORMS + ("E10",), ("headT_class", a, b), parity=True))
    out.append(_mk("up64-16-class11-coff4", "A", (N, HO, WO, HO, WO, _class_taps(1, 1)[0], 64, H2, W2, 24),
                   dict(ohs=2, oho=1, ows=2, owo=1, coff=4), 64, 16, BASE_FORMS + ("E10",),
                   ("convT_class", 1, 1, _class_taps(1, 1)[1]), parity=True))
    # dgrad of the transposed conv (ops.UpFn.backward) and of the 2x2 head (ops.OutFn.backward, k_pad = 32)
    for cout, cin in ((64, 128), (16, 64)):
        out.append(_mk(f"dup{cout}-{cin}", "A", (N, HO, WO, H2, W2, _s2_taps(), cout, HO, WO, cin), s2, cout, cin,
                       BASE_FORMS, ("conv_s2", 3)))
    for nc in (20, 27):
        taps = [(a, b, 0) for a in (0, 1) for b in (0, 1)]
        out.append(_mk(f"dhead{nc}-16", "A", (N, HO, WO, H2, W2, taps, _r4(nc), HO, WO, 16), s2, nc, 16, BASE_FORMS,
                       ("conv_s2", 2)))
    # C -> C: the LDS-tiled <64,64>, <128,128>, <16,16> kernels take a stride-1 call only when the streaming
    # kernels decline it: residual AND gate (E8), or an output row that is not C floats wide
    for C in (64, 128, 16):
        taps = WC.taps3(1, "w")
        out.append(_mk(f"s1-C{C}", "A", (N, HO, WO, HO, WO, taps, C, HO, WO, C), {}, C, C, ("E8",), ("conv3", 1, "w")))
        out.append(_mk(f"s1-C{C}-row{2 * C}", "A", (N, HO, WO, HO, WO, taps, C, HO, WO, 2 * C), {}, C, C, ALL_FORMS,
                       ("conv3", 1, "w")))
    return out


def _s1(name, part, C, N, H, W, d, axis, adapter, forms=ALL_FORMS, in1_pitch=None, out_pitch=None, expect=None):
    taps = WC.taps3(d, axis) + ([(0, 0, 1)] if adapter else [])
    ip = C if in1_pitch is None else (C, in1_pitch)
    return _mk(name, part, (N, H, W, H, W, taps, ip, H, W, out_pitch or C), {}, C, C, forms, ("conv3", d, axis),
               in1=None if not adapter else ("plain" if in1_pitch is None else "wide"), expect=expect)


def _part_b():
    out = []
    for (prod, (C, N, H, W, d, axis), adapter), cid in zip(CC.CONV_CASES, CC.CONV_IDS):
        out.append(_s1(cid, "B", C, N, H, W, d, axis, adapter, expect=prod))
    # c16conv: 189 px = 6 wave tiles, 2 work-groups in a grid of 8, 13 valid pixels in the last group;
    # 2,442 px = 77 tiles, 20 work-groups in a grid of 24 (the XCD-major walk is a real permutation), the
    # last tile has 10 valid pixels in its first group and none in its second
    for axis in ("h", "w"):
        out.append(_s1(f"c16conv-3x9x7-d2{axis}", "B", 16, 3, 9, 7, 2, axis, False, expect="c16conv"))
        out.append(_s1(f"c16conv-2x33x37-d1{axis}", "B", 16, 2, 33, 37, 1, axis, False, expect="c16conv"))
    # d = 16 on a 9-row image: both side taps are out of range at every pixel
    out.append(_s1("c16conv-3x9x7-d16h", "B", 16, 3, 9, 7, 16, "h", False, expect="c16conv"))
    out.append(_s1("sconv-C64-2x9x7-d16h", "B", 64, 2, 9, 7, 16, "h", False, expect="sconv"))
    # the router's fall-backs: a second source with a foreign pitch, a wide output row
    out.append(_s1("fallback-C64-in1-pitch128", "B", 64, 2, 9, 7, 1, "w", True, in1_pitch=128, expect="tapconv"))
    out.append(_s1("fallback-C16-row32", "B", 16, 3, 9, 7, 1, "w", False, out_pitch=32, expect="tapconv"))
    return out


# part C: own route against the LDS-tiled kernel (forced by a 2C-float output row), N(0, 1) draw, bit for bit
IDENTITY_FORMS = tuple(f for f in ALL_FORMS if f != "E8")       # E8 is the LDS-tiled kernel on both sides
IDENTITY_CASES = (("c16conv", 16, 3, 9, 7, 2, "h"), ("c16conv", 16, 2, 33, 37, 1, "w"),
                  ("sconv", 64, 1, 7, 9, 1, "w"), ("sconv", 128, 1, 7, 9, 1, "w"))


def _part_c():
    out = []
    for fam, C, N, H, W, d, axis in IDENTITY_CASES:
        name = f"identity-{fam}-C{C}-{N}x{H}x{W}-d{d}{axis}"
        own = _s1(name, "C", C, N, H, W, d, axis, False, forms=IDENTITY_FORMS, expect=fam)
        own.forced = _s1(name + f"-row{2 * C}", "C", C, N, H, W, d, axis, False, forms=IDENTITY_FORMS, out_pitch=2 * C,
                         expect="tapconv")
        out.append(own)
    return out


CASES = _part_a() + _part_b()
IDENTITY = _part_c()
BY_NAME = {c.name: c for c in CASES + IDENTITY}
assert len(BY_NAME) == len(CASES) + len(IDENTITY)
PARAMS = [(c.name, f) for c in CASES for f in c.forms]
IDENTITY_PARAMS = [(c.name, f) for c in IDENTITY for f in c.forms]


def expected_route(c, form):
    return route(c.g, c.cin, c.cout, form)


# ------------------------------------------------------------------------------------------------
# operands of a (case, form, draw)
# ------------------------------------------------------------------------------------------------
def _seed(c, k):
    return 7 * sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) % 100003 + 101 * k


def _draws(draw):
    """-> (data, scale, shift, gate, weight / bias factor) draw functions of (shape, seed)."""
    if draw == "int":
        return WC.draw_int, draw_scale, WC.draw_int, draw_gate, 1.0
    assert draw == "normal"
    return (WC.draw_normal, lambda s, seed: 1 + 0.1 * WC.draw_normal(s, seed), lambda s, seed: 0.1 * WC.draw_normal(s, seed),
            WC.draw_normal, 0.1)       # weights and biases scaled as test_tapconv_factorised scales them


@functools.lru_cache(maxsize=4)
def inputs(name, draw):
    """Inputs and weights of a case, shared by its forms: in0 [N, HI, WI, in_pitch[0]] with FOREIGN in the
    channels past cin, in1 (a view where the case says so), the dense weight w [cout][cin][ntaps] (the stem:
    [13][3][9]) and the float64 accumulator of the reference."""
    c = BY_NAME[name]
    g, rg = c.g, c.ref_g
    data, _, _, _, wf = _draws(draw)
    t = SimpleNamespace()
    t.in0 = torch.full((g.N, g.HI, g.WI, g.in_pitch[0]), FOREIGN)
    t.in0[..., :c.ref_cin] = data((g.N, g.HI, g.WI, c.ref_cin), _seed(c, 1))
    t.in1 = t.in1_base = None
    if c.in1 == "plain":
        t.in1 = t.in1_base = data((g.N, g.HI, g.WI, c.cin), _seed(c, 2))
    elif c.in1 == "wide":
        t.in1_base = torch.full((g.N, g.HI, g.WI, g.in_pitch[1]), FOREIGN)
        t.in1 = t.in1_base[..., g.in_pitch[1] - c.cin:]
        t.in1.copy_(data((g.N, g.HI, g.WI, c.cin), _seed(c, 2)))
    t.w = data((c.cout, c.ref_cin, c.ref_ntaps), _seed(c, 3)) * wf
    t.W = t.w.permute(2, 0, 1).contiguous()                      # [ntaps][cout][cin]
    t.acc = conv_acc(rg, c.ref_cin, c.cout, t.in0, t.in1, t.W)
    return t


def operands(c, form, draw):
    """-> (inputs, epilogue of host tensors, out_before).  res / res_gate / gate fill the whole output buffer
    (they are addressed like out); "inplace" makes res the output buffer itself."""
    g = c.g
    data, dscale, dshift, dgate, wf = _draws(draw)
    f = FORMS[form]
    shape = (g.N, g.OH, g.OW, g.out_pitch)
    vec = lambda fn, k, s=1.0: fn((c.cout,), _seed(c, k)) * s
    e = epilogue(relu="relu" in f)
    if "bias" in f:
        e.bias = vec(data, 4, wf)
    if "bias2" in f:
        e.bias2 = vec(data, 5, wf)
    if "scale" in f:
        e.scale, e.shift = vec(dscale, 6), vec(dshift, 7)
    if "res_gate" in f:
        e.res_gate = dgate(shape, _seed(c, 9))
    if "gate" in f:
        e.gate = dgate(shape, _seed(c, 10))
    if "inplace" in f:
        out_before = data(shape, _seed(c, 8))
        e.res = out_before
    else:
        out_before = torch.full(shape, SENTINEL)
        if "res" in f:
            e.res = data(shape, _seed(c, 8))
    return inputs(c.name, draw), e, out_before


def expected(c, form, draw):
    """-> (inputs, epilogue, out_before, float64 out_after)."""
    t, e, before = operands(c, form, draw)
    return t, e, before, apply_epilogue(c.g, c.cout, t.acc, e, before)


# ------------------------------------------------------------------------------------------------
# the same convolutions by torch (tests/test_tapconv_contract_cpu.py proves the reference against these)
# ------------------------------------------------------------------------------------------------
def _nchw(t):
    return t.permute(0, 3, 1, 2).double()


def layer_acc(c, in0, in1, w):
    """float64 [N, HO, WO, cout] of the case's launch through F.conv2d / F.conv_transpose2d.  w: the dense
    draw [cout][cin][ntaps].  A parity class is the transposed conv whose kernel is zero outside the
    class's taps, read at the class's output pixels."""
    kind = c.layer[0]
    g = c.ref_g
    x = _nchw(in0[..., :c.ref_cin])
    w = w.double()
    if kind == "conv_s2":                   # k x k, stride 2; padding 1 for the 3 x 3 forms
        k = c.layer[1]
        y = F.conv2d(x, w.reshape(c.cout, c.ref_cin, k, k), stride=2, padding=1 if k == 3 else 0)
    elif kind == "convT_class":
        _, a, b, ktap = c.layer
        full = torch.zeros(c.ref_cin, c.cout, 9, dtype=torch.float64)
        full[:, :, ktap] = w.permute(1, 0, 2)
        y = F.conv_transpose2d(x, full.reshape(c.ref_cin, c.cout, 3, 3), stride=2, padding=1, output_padding=1)
        y = y[:, :, a::2, b::2]
    elif kind == "headT_class":
        _, a, b = c.layer
        full = torch.zeros(c.ref_cin, c.cout, 4, dtype=torch.float64)
        full[:, :, a * 2 + b] = w[:, :, 0].t()
        y = F.conv_transpose2d(x, full.reshape(c.ref_cin, c.cout, 2, 2), stride=2)[:, :, a::2, b::2]
    else:
        _, d, axis = c.layer
        k, pad, dil = ((3, 1), (d, 0), (d, 1)) if axis == "h" else ((1, 3), (0, d), (1, d))
        y = F.conv2d(x, w[:, :, :3].reshape(c.cout, c.cin, *k), padding=pad, dilation=dil)
        if g.ntaps == 4:
            y = y + F.conv2d(_nchw(in1[..., :c.cin]), w[:, :, 3].reshape(c.cout, c.cin, 1, 1))
    assert tuple(y.shape) == (g.N, c.cout, g.HO, g.WO), (c.name, tuple(y.shape))
    return y.permute(0, 2, 3, 1).contiguous()
