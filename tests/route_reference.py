"""The fp64 reference of the routing tests (tests/test_route_cpu.py, tests/test_route_gpu.py): the
stem as ``F.conv2d`` (stride 2, padding 1) plus ``F.max_pool2d(2)`` in double, its per-image moments,
the per-pixel entropy / confidence / margin of a head from ``log_softmax``, the statistics score as
a plain loop, and the photometric routing case.  Nothing here touches a device.

The photometric case.  Three domains of ``ProceduralSeg`` at 16 x 32 that differ as cameras do:
domain d's images times a gain plus an offset, (1, 0), (0.45, 0), (0.6, 0.35).  The statistics of
domain d are the channel means and (population) variances of the stem over 8 images of seed 3 + d;
12 images of seed 12 + d are routed.  Procedural domains WITHOUT gain and offset differ only in
their class colours and do not separate by stem statistics; nothing is asserted on them."""
import functools
import math

import torch
import torch.nn.functional as F

from tests.head_cases import SHAPES

PHOTOMETRIC = ((1.0, 0.0), (0.45, 0.0), (0.6, 0.35))
SIZE = (16, 32)
STEM_CHANNELS = 16                                # 13 conv + 3 pool
STAT_IMAGES, STAT_SEED, ROUTED_IMAGES, ROUTED_SEED = 8, 3, 12, 12
MIN_GAP = 0.1
STEM_SEED = 0                                     # torch.manual_seed(0), then the model: HC.tiny_model's stem
# the images of HC.SHAPES, and one more: 34 x 62 gives 17 x 31 = 527 positions per image, three
# work-groups of 256 with 15 positions in the last; 514 x 514 (257 x 257 = 66,049 positions) is the
# smallest even square beyond 256 work-groups of 256, where the loop strides
STEM_SHAPES = tuple((n, 2 * h, 2 * w) for n, h, w in SHAPES) + ((2, 34, 62),)
STRIDE_SHAPE = (1, 514, 514)


def stem_params(seed=STEM_SEED):
    """The ``Conv2d(3, 13, 3, 2, 1)`` the model builds first after ``torch.manual_seed(seed)``."""
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(3, 13, (3, 3), stride=2, padding=1, bias=True)
    torch.set_rng_state(state)
    return conv.weight.detach().clone(), conv.bias.detach().clone()


@functools.lru_cache(maxsize=None)
def stem_case(shape):
    """Seeded images [N,3,Hi,Wi] in [0, 1) (as the loaders give them) and stem parameters that are not
    the model's: w ~ 0.3 N(0,1), b ~ 0.2 N(0,1).  Shared, never modified."""
    g = torch.Generator().manual_seed(1000 + shape[1] + shape[2])
    return (torch.rand(shape[0], 3, shape[1], shape[2], generator=g), torch.randn(13, 3, 3, 3, generator=g) * 0.3,
            torch.randn(13, generator=g) * 0.2)


def stem64(images, w, b):
    """-> (activation f64 [N,16,H,W], S [N,13,H,W]: |b| + sum |x||w| of the conv channels)."""
    x = images.double()
    act = torch.cat([F.conv2d(x, w.double(), b.double(), stride=2, padding=1), F.max_pool2d(x, 2)], 1)
    S = F.conv2d(x.abs(), w.double().abs(), b.double().abs(), stride=2, padding=1)
    return act, S


def moments(act):
    """[N,16,H,W] -> [N,16,2]: sum a and sum a^2 per image and channel, in the dtype of ``act``."""
    return torch.stack([act.sum((2, 3)), (act * act).sum((2, 3))], 2)


def head_stats64(logits):
    """Per pixel, in the dtype of ``logits`` [N,nc,h,w]: (conf, ent, margin) = top probability,
    -sum p log p, top minus second probability."""
    z = F.log_softmax(logits, 1)
    p = z.exp()
    top = p.topk(2, dim=1)[0]
    return top[:, 0], -(p * z).sum(1), top[:, 0] - top[:, 1]


def stats_scores_loop(moments_, pixels, mean, var, eps):
    """The statistics score as a hand-written fp64 loop -> list [N][T]."""
    out = []
    for n in range(moments_.shape[0]):
        row = []
        for t in range(mean.shape[0]):
            score = 0.0
            for c in range(mean.shape[1]):
                mu = float(moments_[n, c, 0]) / pixels
                vi = float(moments_[n, c, 1]) / pixels - mu * mu + eps
                vt = float(var[t, c]) + eps
                score += 0.5 * (math.log(vt / vi) + (vi + (mu - float(mean[t, c])) ** 2) / vt - 1.0)
            row.append(score)
        out.append(row)
    return out


def domain_images(d, n, seed):
    from mdil_ss_amd.dataset import ProceduralSeg
    ds = ProceduralSeg(n, SIZE[0], SIZE[1], 20, seed=seed, domain=d)
    gain, offset = PHOTOMETRIC[d]
    return torch.stack([ds[i][0] for i in range(n)]) * gain + offset


def gaps(scores):
    """[N,T] -> [N]: (second - best) / second, the relative gap of the two lowest scores."""
    low = scores.topk(2, dim=1, largest=False)[0]
    return (low[:, 1] - low[:, 0]) / low[:, 1]


@functools.lru_cache(maxsize=None)
def photometric_case(eps=1e-3):
    """-> dict: ``images`` f32 [36,3,16,32] (domain-major), ``true`` [36], ``mean`` / ``var`` f64 [3,16],
    ``scores`` f64 [36,3], ``choice`` [36], ``gap`` [36]; the stem is ``stem_params()``."""
    w, b = stem_params()
    stat = [stem64(domain_images(d, STAT_IMAGES, STAT_SEED + d), w, b)[0] for d in range(3)]
    mean = torch.stack([a.mean((0, 2, 3)) for a in stat])
    var = torch.stack([(a * a).mean((0, 2, 3)) for a in stat]) - mean * mean
    images = torch.cat([domain_images(d, ROUTED_IMAGES, ROUTED_SEED + d) for d in range(3)])
    true = torch.arange(3).repeat_interleave(ROUTED_IMAGES)
    act = stem64(images, w, b)[0]
    pixels = act.shape[2] * act.shape[3]
    scores = torch.tensor(stats_scores_loop(moments(act), pixels, mean, var, eps), dtype=torch.float64)
    return dict(images=images, true=true, mean=mean, var=var, eps=eps, scores=scores, choice=scores.argmin(1),
                gap=gaps(scores), w=w, b=b)
