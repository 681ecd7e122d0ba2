// libmdil_refine.so: image-guided mean-field refinement of the head's softmax, fused with
// Decoder.output_conv (gfx950).  One kernel, launched T + 1 times (once for T = 0):
//
//   l_i(c)  = bias[c] + sum_ci x[n, h, w, ci] * W[ci][c][a][b]         i = (n, 2h+a, 2w+b);  Hl = 2H, Wl = 2W
//   Q0      = softmax_c(l)
//   m_i(c)  = sum_j k(i,j) Q^{t-1}_j(c),   Q^t_i = softmax_c(l_i(c) + m_i(c))            t = 1..T
//   j       = i + (dy d, dx d), dy, dx in [-r, r] without (0,0), inside the image
//   k(i,j)  = ca exp(sa[dy,dx] - |I_i - I_j|^2 / (2 theta_b^2)) + ks[dy,dx]
//   label   = argmax_c (l + m) of step T,  confidence = max_c Q^T = 1 / sum_c exp(u_c - u_max)
//
// The logits are never stored: every launch forms the unary again from the 16 feature channels
// (16 nc FMAs against (2r+1)^2 nc for the messages), with stage_head's table and logits4's chain
// for the pixel's own parity (bias first, ci ascending: the bits of predict_head.hip's logits).
//
// Arithmetic contract.
//   * The window's constants come from the host in double and are rounded once: ca = w_a / Z_a,
//     sa[t] = -(dy^2+dx^2) d^2 / (2 theta_a^2), ks[t] = (w_s / Z_s) exp(-(dy^2+dx^2) d^2 / (2 theta_g^2)),
//     1 / (2 theta_b^2); Z_a, Z_s are the sums of the spatial factors over the full window.
//   * Per neighbour: g = I_i - I_j per channel, q = fma(g2,g2, fma(g1,g1, g0*g0)),
//     k = fma(ca, __expf(fma(-q, 1/(2 theta_b^2), sa[t])), ks[t]).  __expf here: the hardware exp2 of
//     x * log2(e), relative error about |x| 2^-24 + 1 ulp on a factor <= 1 -- an underflow to 0 is harmless.
//   * m(c) = fma(k, Q_j(c), m(c)) from 0, dy ascending, then dx ascending: one chain per class, one
//     lane per pixel, no cross-lane reduction.  A neighbour outside the image enters as Q = 0 with a
//     finite k, and the centre (0,0) with k = 0 (sa = -1e30, ks = 0) and a finite Q: both leave the
//     chain's bits as they are (the sums are never negative zero), and the walk has no branch.
//   * u(c) = l(c) + m(c); the argmax is taken of u (vote: lowest index on a tie), so with k = 0 the
//     label is predict_head's; s = sum_c expf(u(c) - u_max), c ascending, with the accurate expf (as
//     predict_head's confidence); Q(c) = expf(u(c) - u_max) / s;  confidence = 1.f / s.
//
// Tiling.  A dilation d splits the logit grid into d*d interleaved sub-grids (y % d, x % d); inside
// one, the window is a dense (2r+1)^2 block.  A work-group of 256 lanes owns a tile of 8 rows x 32
// columns of one sub-grid of one image and stages its halo, (8+2r) x (32+2r) pixels, in LDS, pixel
// by pixel: the image as [pixel][4] (r, g, b, 0) and Q^{t-1} as [pixel][S], the classes padded to a
// multiple of four with zeros and the stride S (in floats) chosen so that S / 4 is odd: then the 16
// lanes of a ds_read_b128 group, whose pixels are S floats apart, cover the 64 banks once.  A lane
// owns one pixel and keeps its sums in registers; a neighbour costs one address add, one 16-byte
// read of the image, one of the window's constants (a broadcast) and one per four classes of Q,
// all at immediate offsets and in flight together.  The kernel is instantiated per count of class
// groups G = ceil(nc / 4) = 1..8, so that the walk over the classes is straight-line code.
// LDS at r = 5: 756 pixels x (4 + S) floats -- 73 KB at nc = 20 (S = 20), 121 KB at nc = 32 (S = 36) --
// dynamic, beside the head's tables (256 G + 1.2 KB) and, in the last launch, the counters
// (128 G^2 B): two work-groups of a step fit a CU's 160 KB up to nc = 20.
// The launch that writes Q0 and the T = 0 launch stage no tile and use d = 1.
//
// Counters (last launch only).  confusion[0] counts (target, argmax l), confusion[1] (target, label),
// in a [2][nc][nc] histogram of 32-bit LDS counters; a work-group adds its non-zero entries to the
// 64-bit matrices with global integer atomics after a barrier, as fullres_head.hip does (a tile has
// 256 pixels: no counter can wrap).  Plain stores of bytes, floats and float4 otherwise.
#include "../../include/mdil_refine.h"
#include "head_common.h"

#include <math.h>

namespace {

static_assert(MDIL_REFINE_MAX_CLASSES == 32, "the kernel is instantiated for 1 to 8 groups of four classes");
constexpr int kMaxR = MDIL_REFINE_MAX_RADIUS;
constexpr int kTileH = 8, kTileW = 32;                // one sub-grid tile; a lane per pixel
constexpr int kWG = kTileH * kTileW;                  // 256 lanes, 4 wavefronts of two tile rows each
constexpr int kTaps = (2 * kMaxR + 1) * (2 * kMaxR + 1);
constexpr char kFn[] = "refine_head";

typedef unsigned long long u64;
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));    // 16 bytes at any float's address

// The window's constants, by value in the kernel arguments; the kernel copies them to LDS.
struct Window {
  float sa[kTaps];                                    // -(dy^2+dx^2) d^2 / (2 theta_a^2)
  float ks[kTaps];                                    // (w_s / Z_s) exp(-(dy^2+dx^2) d^2 / (2 theta_g^2))
  float ca, inv2tb;                                   // w_a / Z_a, 1 / (2 theta_b^2)
};

struct Args {
  const float* x;
  const float* w;
  const float* bias;
  const float* image;
  const float* q_in;                                  // Q^{t-1} [N][Hl][Wl][nc]; NULL: no messages
  float* q_out;                                       // Q^t, or NULL
  unsigned char* label;
  float* confidence;
  const unsigned char* target;
  u64* confusion;
  u64* bad_targets;
  u64* changed;
  int H, W, nc, r, d, ignore_index, tiles_y, tiles_x;
};

constexpr int groups(int nc) { return (nc + 3) / 4; }
// Floats between two pixels of the Q tile for G class groups: 4 G, or 4 G + 4 where G is even.
constexpr int q_stride(int G) { return (G & 1) ? 4 * G : 4 * G + 4; }
inline int halo_pixels(int r) { return (kTileH + 2 * r) * (kTileW + 2 * r); }

// One logit of class c for the pixel's own parity k = a*2+b: logits4's chain (bias first, ci
// ascending), element k.
__device__ __forceinline__ float logit1(const f32x4 (&xv)[4], const float (*Wc)[4], float b, int k) {
  float acc = b;
#pragma unroll
  for (int ci = 0; ci < 16; ++ci) acc = __builtin_fmaf(xv[ci >> 2][ci & 3], Wc[ci][k], acc);
  return acc;
}

template <int G, bool FINAL>
__global__ __launch_bounds__(kWG) void refine_kernel(const Args a, const Window win) {
  constexpr int NC = 4 * G;                                          // the classes, padded
  constexpr int S = q_stride(G);
  __shared__ __attribute__((aligned(16))) float Wl[NC][16][4];      // [c][ci][a*2+b]
  __shared__ float Bl[NC];
  __shared__ uint32_t Pl[NC];                                        // stage_head's palette slot, unused
  __shared__ f32x2 Wt[kTaps];                                        // (sa, ks) per tap
  __shared__ uint32_t hist[FINAL ? 2 * NC * NC : 1];                 // [plane][target][prediction]
  __shared__ uint32_t bad_l, changed_l;
  extern __shared__ __attribute__((aligned(16))) float tile[];       // Is[HP][4], then Qs[HP][S]

  const int nc = a.nc, r = a.r, d = a.d;
  const int Hl = 2 * a.H, Wlog = 2 * a.W;
  int b = blockIdx.x;
  const int txi = b % a.tiles_x;
  b /= a.tiles_x;
  const int tyi = b % a.tiles_y;
  b /= a.tiles_y;
  const int sx = b % d;
  b /= d;
  const int sy = b % d;
  const int n = b / d;
  const int Hs = (Hl - sy + d - 1) / d, Ws = (Wlog - sx + d - 1) / d;   // this sub-grid's size
  const int ty0 = tyi * kTileH, tx0 = txi * kTileW;
  if (ty0 >= Hs || tx0 >= Ws) return;                    // uniform: the smaller sub-grids have fewer tiles

  stage_head<kWG, false>(a.w, a.bias, nullptr, nullptr, nullptr, nc, Wl, Bl, Pl, nullptr);
  if (FINAL) {
    for (int i = threadIdx.x; i < 2 * nc * nc; i += kWG) hist[i] = 0u;
    if (threadIdx.x == 0) bad_l = changed_l = 0u;
  }

  const bool msg = a.q_in != nullptr;
  const int SW = kTileW + 2 * r, SH = kTileH + 2 * r;
  f32x4* Is = reinterpret_cast<f32x4*>(tile);
  float* Qs = tile + 4 * SH * SW;
  if (msg) {
    for (int t = threadIdx.x; t < kTaps; t += kWG) {
      f32x2 v = {win.sa[t], win.ks[t]};
      Wt[t] = v;
    }
    const bool vec = nc == NC;
    const long long plane = (long long)Hl * Wlog;
    for (int p = threadIdx.x; p < SH * SW; p += kWG) {
      const int hy = p / SW, hx = p - hy * SW;
      const int suby = ty0 - r + hy, subx = tx0 - r + hx;
      const int y = suby * d + sy, xx = subx * d + sx;
      const bool inside = suby >= 0 && subx >= 0 && y < Hl && xx < Wlog;
      f32x4 iv = {0.f, 0.f, 0.f, 0.f};
      f32x4* qd = reinterpret_cast<f32x4*>(Qs + p * S);
      if (inside) {
        const float* ip = a.image + ((long long)n * 3 * Hl + y) * Wlog + xx;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) iv[ch] = ip[ch * plane];
        const float* q = a.q_in + (((long long)n * Hl + y) * Wlog + xx) * nc;
        if (vec) {
#pragma unroll
          for (int g = 0; g < G; ++g) qd[g] = *reinterpret_cast<const f32x4*>(q + 4 * g);
        } else {                                        // a pixel's record is only 4-byte aligned
#pragma unroll
          for (int g = 0; g < G - 1; ++g) qd[g] = *reinterpret_cast<const f32x4u*>(q + 4 * g);
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = 4 * (G - 1) + e < nc ? q[4 * (G - 1) + e] : 0.f;
          qd[G - 1] = v;
        }
      } else {
#pragma unroll
        for (int g = 0; g < G; ++g) qd[g] = iv;
      }
      Is[p] = iv;
    }
  }
  __syncthreads();

  const int ly = threadIdx.x / kTileW, lx = threadIdx.x % kTileW;
  const int suby = ty0 + ly, subx = tx0 + lx;
  const bool valid = suby < Hs && subx < Ws;
  if (valid) {
    const int y = suby * d + sy, xx = subx * d + sx;
    const long long pix = ((long long)n * Hl + y) * Wlog + xx;

    float m[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) m[c] = 0.f;

    if (msg) {
      const int centre = (ly + r) * SW + lx + r;
      const f32x4 ic = Is[centre];
      const int side = 2 * r + 1;
      for (int dy = -r; dy <= r; ++dy) {
        for (int dx = -r; dx <= r; ++dx) {
          const int j = centre + dy * SW + dx;
          const f32x4 in = Is[j];
          const f32x2 wt = Wt[(dy + r) * side + dx + r];
          const f32x4* qj = reinterpret_cast<const f32x4*>(Qs + j * S);
          f32x4 qv[G];
#pragma unroll
          for (int g = 0; g < G; ++g) qv[g] = qj[g];
          const float g0 = ic[0] - in[0], g1 = ic[1] - in[1], g2 = ic[2] - in[2];
          const float q = __builtin_fmaf(g2, g2, __builtin_fmaf(g1, g1, g0 * g0));
          const float k = __builtin_fmaf(win.ca, __expf(__builtin_fmaf(-q, win.inv2tb, wt[0])), wt[1]);
#pragma unroll
          for (int g = 0; g < G; ++g) {
#pragma unroll
            for (int e = 0; e < 4; ++e) m[4 * g + e] = __builtin_fmaf(k, qv[g][e], m[4 * g + e]);
          }
        }
      }
    }

    // the unary on the pixel's own parity, the two argmaxes, the softmax
    const float* xp = a.x + (((long long)n * a.H + (y >> 1)) * a.W + (xx >> 1)) * 16;
    f32x4 xv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xv[k] = *reinterpret_cast<const f32x4*>(xp + k * 4);
    const int par = (y & 1) * 2 + (xx & 1);
    float best = 0.f, plain = 0.f;
    int bi = 0, pi = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c < nc) {
        const float l = logit1(xv, Wl[c], Bl[c], par);
        if (FINAL) vote(c, l, plain, pi);
        m[c] = l + m[c];
        vote(c, m[c], best, bi);
      }
    }
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c < nc) {
        m[c] = expf(m[c] - best);
        s += m[c];
      }
    }

    if (a.q_out) {
      float* qo = a.q_out + pix * nc;
      if (nc == NC) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = m[4 * g + e] / s;
          *reinterpret_cast<f32x4*>(qo + 4 * g) = v;
        }
      } else {
#pragma unroll
        for (int g = 0; g < G - 1; ++g) {
          f32x4u v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = m[4 * g + e] / s;
          *reinterpret_cast<f32x4u*>(qo + 4 * g) = v;
        }
#pragma unroll
        for (int c = NC - 4; c < NC; ++c)
          if (c < nc) qo[c] = m[c] / s;
      }
    }

    if (FINAL) {
      a.label[pix] = (unsigned char)bi;
      if (a.confidence) a.confidence[pix] = 1.f / s;
      if (a.changed && bi != pi) atomicAdd(&changed_l, 1u);
      if (a.target) {
        const int t = (int)a.target[pix];
        if (t != a.ignore_index) {
          if (t < nc) {
            atomicAdd(&hist[t * nc + pi], 1u);
            atomicAdd(&hist[(nc + t) * nc + bi], 1u);
          } else {
            atomicAdd(&bad_l, 1u);
          }
        }
      }
    }
  }

  if (FINAL && (a.target || a.changed)) {                // uniform over the work-group
    __syncthreads();
    if (a.target) {
      for (int i = threadIdx.x; i < 2 * nc * nc; i += kWG) {
        const uint32_t v = hist[i];
        if (v) atomicAdd(a.confusion + i, (u64)v);
      }
    }
    if (threadIdx.x == 0) {
      if (a.target && bad_l) atomicAdd(a.bad_targets, (u64)bad_l);
      if (a.changed && changed_l) atomicAdd(a.changed, (u64)changed_l);
    }
  }
}

inline bool finite_pos(const char* name, float v) {
  if (isfinite(v) && v > 0.f) return true;
  set_error("%s: %s=%g must be finite and > 0", kFn, name, (double)v);
  return false;
}

inline bool finite_nonneg(const char* name, float v) {
  if (isfinite(v) && v >= 0.f) return true;
  set_error("%s: %s=%g must be finite and >= 0", kFn, name, (double)v);
  return false;
}

// The sizes both entry points judge.  -> the bytes of one Q buffer, or -1 with the message set.
inline long long q_bytes(const char* fn, int N, int H, int W, int nc, int iterations) {
  if (N <= 0 || H <= 0 || W <= 0) {
    set_error("%s: bad argument (N %d H %d W %d)", fn, N, H, W);
    return -1;
  }
  if (!classes_ok(fn, nc, MDIL_REFINE_MIN_CLASSES, MDIL_REFINE_MAX_CLASSES)) return -1;
  if (iterations < 0 || iterations > MDIL_REFINE_MAX_ITERATIONS) {
    set_error("%s: iterations=%d outside [0, %d]", fn, iterations, MDIL_REFINE_MAX_ITERATIONS);
    return -1;
  }
  if (H > (1 << 28) || W > (1 << 28) || (long long)N * H > MDIL_REFINE_MAX_PIXELS / 4 / W) {
    set_error("%s: too large (N %d, features %d x %d: at most 2^40 output pixels)", fn, N, H, W);
    return -1;
  }
  return (long long)N * H * W * 4 * nc * (long long)sizeof(float);
}

inline long long workspace_need(long long one, int iterations) {
  return iterations == 0 ? 0 : iterations == 1 ? one : 2 * one;
}

template <int G, bool FINAL>
bool launch_g(const Args& a, const Window& win, long long blocks, bool msg, hipStream_t stream) {
  const size_t lds = msg ? (size_t)halo_pixels(a.r) * (4 + q_stride(G)) * sizeof(float) : 0;
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&refine_kernel<G, FINAL>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      set_error("%s: %zu bytes of LDS refused: %s", kFn, lds, hipGetErrorString(e));
      return false;
    }
  }
  hipLaunchKernelGGL((refine_kernel<G, FINAL>), dim3((unsigned)blocks), dim3(kWG), lds, stream, a, win);
  return launched(kFn);
}

// One launch of the kernel instantiated for groups(nc); the caller bounds the grid.
template <bool FINAL>
bool launch(const Args& a, const Window& win, int N, bool msg, hipStream_t stream) {
  const long long blocks = (long long)N * a.d * a.d * a.tiles_y * a.tiles_x;
  switch (groups(a.nc)) {
    case 1: return launch_g<1, FINAL>(a, win, blocks, msg, stream);
    case 2: return launch_g<2, FINAL>(a, win, blocks, msg, stream);
    case 3: return launch_g<3, FINAL>(a, win, blocks, msg, stream);
    case 4: return launch_g<4, FINAL>(a, win, blocks, msg, stream);
    case 5: return launch_g<5, FINAL>(a, win, blocks, msg, stream);
    case 6: return launch_g<6, FINAL>(a, win, blocks, msg, stream);
    case 7: return launch_g<7, FINAL>(a, win, blocks, msg, stream);
    default: return launch_g<8, FINAL>(a, win, blocks, msg, stream);
  }
}

}  // namespace

API int mdil_refine_version(void) { return 100; }
API const char* mdil_refine_last_error(void) { return g_err; }

API long long mdil_refine_workspace_bytes(int N, int H, int W, int nc, int iterations) {
  const long long one = q_bytes("refine_workspace_bytes", N, H, W, nc, iterations);
  return one < 0 ? -1 : workspace_need(one, iterations);
}

API int mdil_refine_head(const float* features, const float* weight, const float* bias, const float* image, int N,
                         int H, int W, int nc, int iterations, int radius, int dilation, float w_app,
                         float w_smooth, float theta_alpha, float theta_beta, float theta_gamma, void* workspace,
                         long long workspace_bytes, unsigned char* label, float* confidence, float* q_out,
                         const unsigned char* target, int ignore_index, long long* confusion,
                         long long* bad_targets, long long* changed, void* stream) {
  if (!features || !weight || !bias || !label || N <= 0 || H <= 0 || W <= 0) {
    set_error("refine_head: bad argument (features %p weight %p bias %p label %p N %d H %d W %d)",
              (const void*)features, (const void*)weight, (const void*)bias, (void*)label, N, H, W);
    return MDIL_REFINE_ERR_INVALID;
  }
  const long long one = q_bytes(kFn, N, H, W, nc, iterations);
  if (one < 0) return MDIL_REFINE_ERR_INVALID;
  if (radius < 1 || radius > MDIL_REFINE_MAX_RADIUS) {
    set_error("refine_head: radius=%d outside [1, %d]", radius, MDIL_REFINE_MAX_RADIUS);
    return MDIL_REFINE_ERR_INVALID;
  }
  if (dilation < 1 || dilation > MDIL_REFINE_MAX_DILATION) {
    set_error("refine_head: dilation=%d outside [1, %d]", dilation, MDIL_REFINE_MAX_DILATION);
    return MDIL_REFINE_ERR_INVALID;
  }
  if (!finite_pos("theta_alpha", theta_alpha) || !finite_pos("theta_beta", theta_beta) ||
      !finite_pos("theta_gamma", theta_gamma) || !finite_nonneg("w_app", w_app) ||
      !finite_nonneg("w_smooth", w_smooth))
    return MDIL_REFINE_ERR_INVALID;
  if (iterations > 0 && !image) {
    set_error("refine_head: bad argument (image %p with iterations %d)", (const void*)image, iterations);
    return MDIL_REFINE_ERR_INVALID;
  }
  if (!scoring_ok(kFn, target, confusion, bad_targets, ignore_index)) return MDIL_REFINE_ERR_INVALID;
  if (((uintptr_t)features & 15) || ((uintptr_t)image & 3) || ((uintptr_t)workspace & 15) ||
      ((uintptr_t)confidence & 3) || ((uintptr_t)q_out & 15) || ((uintptr_t)confusion & 7) ||
      ((uintptr_t)bad_targets & 7) || ((uintptr_t)changed & 7)) {
    set_error("refine_head: alignment (features, workspace and q_out 16 B; image and confidence 4 B; "
              "confusion, bad_targets and changed 8 B)");
    return MDIL_REFINE_ERR_INVALID;
  }
  const long long need = workspace_need(one, iterations);
  if (need > 0 && (!workspace || workspace_bytes < need)) {
    set_error("refine_head: %d iterations need a workspace of %lld bytes (got %p, %lld bytes)", iterations, need,
              workspace, workspace_bytes);
    return MDIL_REFINE_ERR_INVALID;
  }

  // the window's constants, in double, rounded once
  Window win;
  const int side = 2 * radius + 1;
  double za = 0.0, zs = 0.0;
  for (int dy = -radius; dy <= radius; ++dy) {
    for (int dx = -radius; dx <= radius; ++dx) {
      if (dy == 0 && dx == 0) continue;
      const double d2 = (double)(dy * dy + dx * dx) * dilation * dilation;
      za += exp(-d2 / (2.0 * theta_alpha * theta_alpha));
      zs += exp(-d2 / (2.0 * theta_gamma * theta_gamma));
    }
  }
  for (int t = 0; t < kTaps; ++t) win.sa[t] = win.ks[t] = 0.f;
  for (int dy = -radius; dy <= radius; ++dy) {
    for (int dx = -radius; dx <= radius; ++dx) {
      const double d2 = (double)(dy * dy + dx * dx) * dilation * dilation;
      const int t = (dy + radius) * side + dx + radius;
      win.sa[t] = (float)(-d2 / (2.0 * theta_alpha * theta_alpha));
      win.ks[t] = zs > 0.0 ? (float)((double)w_smooth / zs * exp(-d2 / (2.0 * theta_gamma * theta_gamma))) : 0.f;
    }
  }
  // the centre tap is walked like the others with k = 0: exp2 of -1e30 log2(e) is 0, and fma(0, Q, m) is m
  win.sa[radius * side + radius] = -1e30f;
  win.ks[radius * side + radius] = 0.f;
  win.ca = za > 0.0 ? (float)((double)w_app / za) : 0.f;
  win.inv2tb = (float)(1.0 / (2.0 * (double)theta_beta * theta_beta));

  Args a;
  a.x = features;
  a.w = weight;
  a.bias = bias;
  a.image = image;
  a.label = label;
  a.confidence = confidence;
  a.target = target;
  a.confusion = reinterpret_cast<u64*>(confusion);
  a.bad_targets = reinterpret_cast<u64*>(bad_targets);
  a.changed = reinterpret_cast<u64*>(changed);
  a.H = H;
  a.W = W;
  a.nc = nc;
  a.r = radius;
  a.ignore_index = ignore_index;
  const int Hl = 2 * H, Wl = 2 * W;
  auto geometry = [&](int d) {
    a.d = d;
    a.tiles_y = ((Hl + d - 1) / d + kTileH - 1) / kTileH;
    a.tiles_x = ((Wl + d - 1) / d + kTileW - 1) / kTileW;
    return (long long)N * d * d * a.tiles_y * a.tiles_x <= 0x7fffffffLL;
  };
  if (!geometry(1) || !geometry(dilation)) {
    set_error("refine_head: too large (N %d, features %d x %d: more than 2^31 - 1 tiles)", N, H, W);
    return MDIL_REFINE_ERR_INVALID;
  }

  float* buf[2] = {static_cast<float*>(workspace),
                   iterations >= 2 ? reinterpret_cast<float*>(static_cast<char*>(workspace) + one) : nullptr};
  const hipStream_t s = (hipStream_t)stream;
  if (iterations == 0) {                                   // plain prediction
    geometry(1);
    a.q_in = nullptr;
    a.q_out = q_out;
    return launch<true>(a, win, N, false, s) ? MDIL_REFINE_OK : MDIL_REFINE_ERR_LAUNCH;
  }
  geometry(1);
  a.q_in = nullptr;
  a.q_out = buf[0];
  if (!launch<false>(a, win, N, false, s)) return MDIL_REFINE_ERR_LAUNCH;
  geometry(dilation);
  int cur = 0;
  for (int t = 1; t < iterations; ++t) {
    a.q_in = buf[cur];
    a.q_out = buf[cur ^ 1];
    if (!launch<false>(a, win, N, true, s)) return MDIL_REFINE_ERR_LAUNCH;
    cur ^= 1;
  }
  a.q_in = buf[cur];
  a.q_out = q_out;
  return launch<true>(a, win, N, true, s) ? MDIL_REFINE_OK : MDIL_REFINE_ERR_LAUNCH;
}
