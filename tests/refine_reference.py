"""The refinement add-on's model (include/mdil_refine.h) in torch on the host, the dtype a parameter:
evaluated in float64 it is the reference of tests/test_refine_gpu.py, in float32 the yardstick that
says how far an honest fp32 evaluation lies from it.  Shifted slices over the window; nothing here
touches the package or a device.

    Q0 = softmax(l);  m_i(c) = sum_j k(i,j) Q_j(c);  Q <- softmax(l + m), T times
    k(i,j) = (w_a/Z_a) exp(-|dp|^2/(2 theta_a^2) - |I_i - I_j|^2/(2 theta_b^2)) + (w_s/Z_s) exp(-|dp|^2/(2 theta_g^2))
"""
import functools
import math

import torch
import torch.nn.functional as F


def taps(p):
    """[(dy, dx, |dp|^2)] in the summation order: dy ascending, then dx ascending, without (0, 0)."""
    r, d = p.radius, p.dilation
    return [(dy, dx, float((dy * dy + dx * dx) * d * d)) for dy in range(-r, r + 1) for dx in range(-r, r + 1)
            if (dy, dx) != (0, 0)]


def normalisers(p):
    """(Z_a, Z_s): the sums of the two spatial factors over the full window."""
    za = sum(math.exp(-d2 / (2.0 * p.theta_alpha ** 2)) for _, _, d2 in taps(p))
    zs = sum(math.exp(-d2 / (2.0 * p.theta_gamma ** 2)) for _, _, d2 in taps(p))
    return za, zs


def head_logits(x, w, b, dtype):
    """x [N,16,H,W], w [16,nc,2,2], b [nc] -> logits [N,nc,2H,2W] in ``dtype``."""
    return F.conv_transpose2d(x.to(dtype), w.to(dtype), b.to(dtype), stride=2)


def mean_field(logits, image, p, dtype=torch.float64):
    """logits [N,nc,Hl,Wl], image [N,3,Hl,Wl] -> Q^T [N,nc,Hl,Wl] in ``dtype``."""
    l, img = logits.to(dtype), image.to(dtype)
    Hl, Wl = l.shape[2:]
    q = F.softmax(l, 1)
    if p.iterations == 0:
        return q
    za, zs = normalisers(p)
    ca, cs = p.w_appearance / za, p.w_smooth / zs
    d = p.dilation
    window = []
    for dy, dx, d2 in taps(p):
        oy, ox = dy * d, dx * d
        y0, y1, x0, x1 = max(0, -oy), min(Hl, Hl - oy), max(0, -ox), min(Wl, Wl - ox)
        if y0 >= y1 or x0 >= x1:
            continue
        here = (slice(None), slice(None), slice(y0, y1), slice(x0, x1))
        there = (slice(None), slice(None), slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
        di2 = ((img[here] - img[there]) ** 2).sum(1, keepdim=True)
        k = ca * torch.exp(-d2 / (2.0 * p.theta_alpha ** 2) - di2 / (2.0 * p.theta_beta ** 2)) + \
            cs * math.exp(-d2 / (2.0 * p.theta_gamma ** 2))
        window.append((here, there, k))
    for _ in range(p.iterations):
        m = torch.zeros_like(q)
        for here, there, k in window:
            m[here] += k * q[there]
        q = F.softmax(l + m, 1)
    return q


def block_image(N, Hl, Wl, seed):
    """f32 [N,3,Hl,Wl] in [0, 1]: 6 x 6 blocks drawn from 5 random colours plus 0.02 Gaussian noise,
    so that the appearance kernel takes values across (0, 1] (a uniform random image zeroes it)."""
    g = torch.Generator().manual_seed(seed)
    colours = torch.rand(5, 3, generator=g)
    hb, wb = (Hl + 5) // 6, (Wl + 5) // 6
    idx = torch.randint(0, 5, (N, hb, wb), generator=g)
    img = colours[idx].repeat_interleave(6, 1).repeat_interleave(6, 2)[:, :Hl, :Wl].permute(0, 3, 1, 2)
    return (img + 0.02 * torch.randn(N, 3, Hl, Wl, generator=g)).clamp(0.0, 1.0).contiguous()


@functools.lru_cache(maxsize=None)
def image_for(shape):
    """The guide image of the head case ``shape`` = (N, H, W); shared, never modified."""
    N, H, W = shape
    return block_image(N, 2 * H, 2 * W, 1000 + 7 * H + W)
