// libmdil_ensemble.so: multi-scale / flip ensembles.  Per view Decoder.output_conv, the un-mirroring
// and the bilinear resize of the logits to Ho x Wo; then the vote over the views, the per-pixel
// argmax and the confusion matrix against a target of that size, all in one kernel (gfx950).
//
//   l_v[n, 2h+a, 2w+b, c] = bias[c] + sum_ci x_v[n, h, w, ci] * W[ci][c][a][b]     Hl = 2H_v, Wl = 2W_v
//   l'_v[y, j]            = mirrored ? l_v[y, Wl - 1 - j] : l_v[y, j]
//   U_v,c[n, yo, xo]      = wy0 wx0 l'[y0, x0] + wy0 wx1 l'[y0, x0+1] + wy1 wx0 l'[y0+1, x0] + wy1 wx1 l'[y0+1, x0+1]
//   PROB:  S_c = sum_v softmax_c(U_v)        LOGIT:  S_c = sum_v U_v,c
//   label = id_map[argmax_c S_c],  colour = palette[argmax_c S_c],  confusion[target][argmax] += 1
//
// Unfused, every view at batch 6 writes 1 GB of resized logits at 2048x1024, a softmax pass and an
// accumulate pass over it; here K x 50 MB of features come in and 12.6 MB of labels go out.
//
// Source coordinates (include/mdil_ensemble.h) are integers, exactly as in fullres_head.hip:
// y0 = num / den, rem = num % den with num = (2 yo + 1) Hl - Ho, den = 2 Ho; rem = 0 where num < 0
// or y0 = Hl - 1 (clamped edges: full weight on y0).
//
// Order of operations per view (the direct route: fullres_head.hip's own, steps 1 to 4), and the
// roundings on the longest path to a resized logit:
//   1. wy1 = (float)rem / (float)den, wy0 = (float)(den - rem) / (float)den: operands exact
//      (< 2^24), one correctly rounded division each; wx0, wx1 alike.  wy0 is NOT 1 - wy1.  (1 + 1)
//   2. wt[a][b'] = wy[a] * wx[b']: one product.  a is the parity of the logit row, b' the parity
//      of the column of l' (of the VIEW's own grid, mirrored or not).                          (1)
//   3. s[ci][a*2+b'] = wt[a][b'] * x[ci], x the feature pixel under that neighbour: column j >> 1
//      of a plain view, W_v - 1 - (j >> 1) of a mirrored one.                                  (1)
//   4. U_c = fma chain from bias[c] over ci ascending, inside ci over a*2+b' ascending:
//      acc = fma(s[ci][k], T[c][ci][k], acc), 64 FMAs, one rounding each; T[c][ci][a*2+b'] is
//      W[ci][c][a][b'] for a plain view and W[ci][c][a][1-b'] for a mirrored one (column j of l'
//      is column Wl - 1 - j of l, whose parity is the other one).                             (64)
//   A term of the sum carries 4 roundings before the chain and at most 64 in it:
//   k = 68 roundings, |U_v,c - exact| <= gamma_68 * (|bias_c| + bilinear(sum_ci |x| |W|)).
//   A mirrored view therefore runs, operation by operation, what a plain view with the features
//   flipped along W and the kernel columns swapped runs: the labels are bit-for-bit the same.
//   One plain view in LOGIT mode is fullres_head.hip's arithmetic: the same bytes.
//   5. PROB only, two passes over the view's U_c kept in LDS:  m = max_c U_c;
//      a_c = U_c - m (1 rounding);  e_c = exp2(a_c * log2(e)) (the product: 1 rounding; log2(e)
//      rounded to fp32: relative 2^-26; v_exp_f32: 1 ulp = 2 u relative);  sum = e_0 + e_1 + ...
//      classes ascending (nc - 1 roundings);  r = 1.0f / sum (IEEE division, correctly rounded:
//      1 u -- not v_rcp_f32);  p_c = e_c * r (1 rounding).
//      The argument of the exponential is off by at most 2.3 u |a_c| relative, which moves e_c by
//      2.3 u |a_c| e_c and p_c by less than 2.3 u * 0.54 since |a| 2^-|a| < 0.54; the exponential
//      adds 2 u, the reciprocal and the product 1 u each; the sum is off by (nc - 1) u from its
//      additions and by the e-weighted mean of the terms' errors, at most (2.3 * 2.5 + 2) u for 32
//      classes.  With p <= 1:
//      softmax: 48 u   (absolute error the softmax arithmetic itself adds to one p_v,c; 44 u counted)
//   6. S_c = first view's U_c / p_c, then S_c = S_c + U_c / p_c, views ascending (nviews - 1
//      roundings), in LDS.
//   7. argmax over S: strictly greater replaces, so the lowest class keeps a tie; a NaN replaces any
//      number and is never replaced.  id_map / palette are looked up after it.
//   8. confidence.  PROB: S_max / (float)nviews.  LOGIT: 1 / sum_c exp2(((S_c - S_max) /
//      (float)nviews) * log2(e)), classes ascending -- the winner's softmax of S / nviews, with
//      the same exponential and division as step 5.
//
// Layout.  A lane owns two horizontally adjacent output pixels of one row.  They share the row's
// y0, weights and feature rows; per view the four scaled feature pixels of each sit in 2 x 64
// registers (parity slots picked with ?: while LOADING, no register array is indexed at run
// time), and each class is one walk over T[c][ci][a*2+b'] in LDS -- one broadcast 16-byte read per
// (class, channel) feeds the 8 FMAs of the pair.  The class count is a run-time loop bound, so the
// per-class accumulators S_c (and, in PROB mode, the view's U_c / e_c) cannot be registers: they
// live in LDS as float2 [nc][64], one 8-byte slot per lane and class, conflict-free, touched by
// their own lane only (no barrier).  A work-group is ONE wavefront, so that this LDS (32 KB for 32
// classes in PROB mode, plus both weight tables) stays below 64 KB and several work-groups share a
// compute unit.  Work-group-uniform grid-stride loop with 64-bit indices and a bounded grid.
//
// Confusion.  As in fullres_head.hip: a [nc][nc] histogram of 32-bit counters in LDS (LDS atomics),
// added to the 64-bit matrix with global atomic adds after the loop (and every 2^20 trips).
#include "../../include/mdil_ensemble.h"
#include "head_common.h"

namespace {

constexpr int kWG = 64;                              // one wavefront
constexpr int kMaxC = MDIL_ENSEMBLE_MAX_CLASSES;
constexpr int kMaxV = MDIL_ENSEMBLE_MAX_VIEWS;
constexpr int kMaxBlocks = 8192;                     // beyond 524,288 items (of 2 pixels) the loop strides
constexpr float kLog2e = 1.44269504088896340736f;
constexpr int kFlushEvery = 1 << 20;                 // trips; a trip adds at most 128 counts per work-group
constexpr char kFn[] = "ensemble_head";

struct ViewTable {
  const float* x[kMaxV];
  int H[kMaxV];
  int W[kMaxV];
  int mirrored[kMaxV];
};

template <bool PROB>
__global__ __launch_bounds__(kWG) void ensemble_head_kernel(
    const ViewTable views, int nviews, const float* __restrict__ w, const float* __restrict__ bias,
    long long nitems, int nc, int Ho, int Wo, const unsigned char* __restrict__ id_map,
    const unsigned char* __restrict__ palette, const unsigned char* __restrict__ target,
    int ignore_index, unsigned char* __restrict__ label, unsigned char* __restrict__ colour,
    float* __restrict__ confidence, unsigned long long* __restrict__ confusion,
    unsigned long long* __restrict__ bad_targets) {
  // dynamic: T plain [nc][16][4], T mirrored [nc][16][4], S float2 [nc][64], PROB: E float2 [nc][64]
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  __shared__ float Bl[kMaxC];
  __shared__ uint32_t Pl[kMaxC];                                     // r | g << 8 | b << 16
  __shared__ uint32_t Il[kMaxC];                                     // byte written for class c
  __shared__ uint32_t hist[kMaxC * kMaxC];                           // [target][prediction]
  __shared__ uint32_t bad;
  float* const Tp = dyn;
  float* const Tm = dyn + nc * 64;
  f32x2* const Sl = reinterpret_cast<f32x2*>(dyn + nc * 128) + threadIdx.x;          // [c * kWG]
  f32x2* const El = Sl + nc * kWG;                                                   // PROB only
  for (int i = threadIdx.x; i < nc * 64; i += kWG) {     // head_common.h's stage_head, for two flat tables
    const int k = i & 3, ci = (i >> 2) & 15, c = i >> 6;
    Tp[i] = w[(ci * nc + c) * 4 + k];
    Tm[i] = w[(ci * nc + c) * 4 + (k ^ 1)];
  }
  for (int c = threadIdx.x; c < nc; c += kWG) {
    Bl[c] = bias[c];
    Pl[c] = colour ? (uint32_t)palette[3 * c] | (uint32_t)palette[3 * c + 1] << 8 |
                         (uint32_t)palette[3 * c + 2] << 16
                   : 0u;
    Il[c] = id_map ? (uint32_t)id_map[c] : (uint32_t)c;
  }
  confusion_zero<kWG>(hist, bad, nc);
  __syncthreads();

  const long long G = ((long long)Wo + 1) >> 1;          // items per output row
  const float fnv = (float)nviews;
  int trips = 0;

  // the trip count is the same for every lane of the work-group (barriers inside)
  for (long long base = (long long)blockIdx.x * kWG; base < nitems;
       base += (long long)gridDim.x * kWG) {
    const long long item = base + threadIdx.x;
    if (item < nitems) {
      const long long r = item / G;                        // n * Ho + yo
      const int g = (int)(item - r * G);
      const long long n = r / Ho;
      const int yo = (int)(r - n * Ho);
      const int xa = 2 * g, xb = min(2 * g + 1, Wo - 1);

#pragma unroll 1
      for (int v = 0; v < nviews; ++v) {
        const float* __restrict__ x = views.x[v];
        const int H = views.H[v], W = views.W[v];
        const bool mir = views.mirrored[v] != 0;
        const int Hl = 2 * H, Wl = 2 * W;
        int y0;
        float wy0, wy1;
        axis(yo, Hl, Ho, y0, wy0, wy1);
        const bool oddy = y0 & 1;
        const int h0 = y0 >> 1, h1 = min((y0 + 1) >> 1, H - 1);
        const long long rowoff[2] = {(n * H + (oddy ? h1 : h0)) * W, (n * H + (oddy ? h0 : h1)) * W};
        const float wy[2] = {oddy ? wy1 : wy0, oddy ? wy0 : wy1};

        f32x4 s0[16], s1[16];
        gather(x, rowoff, wy, xa, Wl, Wo, W, mir, s0);
        __builtin_amdgcn_sched_barrier(0);                 // one pixel's 16 loads in flight at a time
        gather(x, rowoff, wy, xb, Wl, Wo, W, mir, s1);
        __builtin_amdgcn_sched_barrier(0);
        const float* const T = mir ? Tm : Tp;
        float m0 = -INFINITY, m1 = -INFINITY;
        for (int c = 0; c < nc; ++c) {
          float u0 = Bl[c], u1 = u0;
#pragma unroll
          for (int ci = 0; ci < 16; ++ci) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(T + (c * 16 + ci) * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              u0 = __builtin_fmaf(s0[ci][k], wv[k], u0);
              u1 = __builtin_fmaf(s1[ci][k], wv[k], u1);
            }
          }
          if (PROB) {
            m0 = fmaxf(m0, u0);
            m1 = fmaxf(m1, u1);
            El[c * kWG] = f32x2{u0, u1};
          } else if (v == 0) {
            Sl[c * kWG] = f32x2{u0, u1};
          } else {
            const f32x2 sv = Sl[c * kWG];
            Sl[c * kWG] = f32x2{sv[0] + u0, sv[1] + u1};
          }
        }
        if (PROB) {
          float sum0 = 0.f, sum1 = 0.f;
          for (int c = 0; c < nc; ++c) {
            const f32x2 u = El[c * kWG];
            const float e0 = __builtin_amdgcn_exp2f((u[0] - m0) * kLog2e);
            const float e1 = __builtin_amdgcn_exp2f((u[1] - m1) * kLog2e);
            sum0 = c == 0 ? e0 : sum0 + e0;
            sum1 = c == 0 ? e1 : sum1 + e1;
            El[c * kWG] = f32x2{e0, e1};
          }
          const float r0 = 1.0f / sum0, r1 = 1.0f / sum1;
          for (int c = 0; c < nc; ++c) {
            const f32x2 e = El[c * kWG];
            const float p0 = e[0] * r0, p1 = e[1] * r1;
            if (v == 0) {
              Sl[c * kWG] = f32x2{p0, p1};
            } else {
              const f32x2 sv = Sl[c * kWG];
              Sl[c * kWG] = f32x2{sv[0] + p0, sv[1] + p1};
            }
          }
        }
      }

      float best[2] = {0.f, 0.f};
      int bi[2] = {0, 0};
      for (int c = 0; c < nc; ++c) {
        const f32x2 sv = Sl[c * kWG];
        vote(c, sv[0], best[0], bi[0]);
        vote(c, sv[1], best[1], bi[1]);
      }
      float conf[2] = {0.f, 0.f};
      if (confidence) {
        if (PROB) {
          conf[0] = best[0] / fnv;
          conf[1] = best[1] / fnv;
        } else {
          float sum0 = 0.f, sum1 = 0.f;
          for (int c = 0; c < nc; ++c) {
            const f32x2 sv = Sl[c * kWG];
            const float e0 = __builtin_amdgcn_exp2f(((sv[0] - best[0]) / fnv) * kLog2e);
            const float e1 = __builtin_amdgcn_exp2f(((sv[1] - best[1]) / fnv) * kLog2e);
            sum0 = c == 0 ? e0 : sum0 + e0;
            sum1 = c == 0 ? e1 : sum1 + e1;
          }
          conf[0] = 1.0f / sum0;
          conf[1] = 1.0f / sum1;
        }
      }

      const long long o = r * Wo + 2LL * g;                // first pixel of the item
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (2 * g + j < Wo) {
          const int p = bi[j];
          label[o + j] = (unsigned char)Il[p];
          if (colour) {
            const uint32_t pc = Pl[p];
            unsigned char* cp = colour + (o + j) * 3;
            cp[0] = (unsigned char)pc;
            cp[1] = (unsigned char)(pc >> 8);
            cp[2] = (unsigned char)(pc >> 16);
          }
          if (confidence) confidence[o + j] = conf[j];
          if (target) {
            const int t = (int)target[o + j];
            if (t != ignore_index) {
              if (t < nc)
                atomicAdd(&hist[t * nc + p], 1u);
              else
                atomicAdd(&bad, 1u);
            }
          }
        }
      }
    }

    const bool last = base + (long long)gridDim.x * kWG >= nitems;
    if (target && (last || ++trips == kFlushEvery)) {       // uniform over the work-group
      trips = 0;
      __syncthreads();
      for (int i = threadIdx.x; i < nc * nc; i += kWG) {
        const uint32_t cnt = hist[i];
        if (cnt) {
          atomicAdd(confusion + i, (unsigned long long)cnt);
          hist[i] = 0u;
        }
      }
      if (threadIdx.x == 0 && bad) {
        atomicAdd(bad_targets, (unsigned long long)bad);
        bad = 0u;
      }
      __syncthreads();
    }
  }
}

}  // namespace

API int mdil_ensemble_version(void) { return 100; }
API const char* mdil_ensemble_last_error(void) { return g_err; }

API int mdil_ensemble_head(const mdil_ensemble_view* views, int nviews, const float* w, const float* bias,
                           int N, int nc, int Ho, int Wo, int mode, const unsigned char* id_map,
                           const unsigned char* palette, const unsigned char* target, int ignore_index,
                           unsigned char* label, unsigned char* colour, float* confidence,
                           long long* confusion, long long* bad_targets, void* stream) {
  if (nviews < 1 || nviews > MDIL_ENSEMBLE_MAX_VIEWS) {
    set_error("ensemble_head: nviews=%d outside [1, %d]", nviews, MDIL_ENSEMBLE_MAX_VIEWS);
    return MDIL_ENSEMBLE_ERR_INVALID;
  }
  if (!views || !w || !bias || !label || N <= 0 || Ho <= 0 || Wo <= 0) {
    set_error("ensemble_head: bad argument (views %p w %p bias %p label %p N %d Ho %d Wo %d)",
              (const void*)views, (const void*)w, (const void*)bias, (void*)label, N, Ho, Wo);
    return MDIL_ENSEMBLE_ERR_INVALID;
  }
  if (!classes_ok(kFn, nc, MDIL_ENSEMBLE_MIN_CLASSES, MDIL_ENSEMBLE_MAX_CLASSES)) return MDIL_ENSEMBLE_ERR_INVALID;
  if (mode != MDIL_ENSEMBLE_MODE_PROB && mode != MDIL_ENSEMBLE_MODE_LOGIT) {
    set_error("ensemble_head: mode=%d is neither MDIL_ENSEMBLE_MODE_PROB (0) nor _LOGIT (1)", mode);
    return MDIL_ENSEMBLE_ERR_INVALID;
  }
  if (!out_size_ok(kFn, Ho, Wo, MDIL_ENSEMBLE_MAX_SIZE)) return MDIL_ENSEMBLE_ERR_INVALID;
  if ((long long)N * Ho > MDIL_ENSEMBLE_MAX_PIXELS / Wo) {
    set_error("ensemble_head: too large (N %d, output %d x %d: at most 2^40 pixels)", N, Ho, Wo);
    return MDIL_ENSEMBLE_ERR_INVALID;
  }
  ViewTable table = {};
  for (int v = 0; v < nviews; ++v) {
    const mdil_ensemble_view& V = views[v];
    if (!V.x || V.H <= 0 || V.W <= 0) {
      set_error("ensemble_head: view %d: bad argument (x %p H %d W %d)", v, (const void*)V.x, V.H, V.W);
      return MDIL_ENSEMBLE_ERR_INVALID;
    }
    if (V.H > (1 << 29) || V.W > (1 << 29) || (long long)N * V.H > MDIL_ENSEMBLE_MAX_PIXELS / V.W) {
      set_error("ensemble_head: view %d: too large (N %d, features %d x %d: at most 2^40 pixels)", v, N,
                V.H, V.W);
      return MDIL_ENSEMBLE_ERR_INVALID;
    }
    if ((uintptr_t)V.x & 15) {
      set_error("ensemble_head: view %d: alignment (x 16 B)", v);
      return MDIL_ENSEMBLE_ERR_INVALID;
    }
    table.x[v] = V.x;
    table.H[v] = V.H;
    table.W[v] = V.W;
    table.mirrored[v] = V.mirrored != 0;
  }
  if (!colour_ok(kFn, colour, palette) || !scoring_ok(kFn, target, confusion, bad_targets, ignore_index))
    return MDIL_ENSEMBLE_ERR_INVALID;
  if (((uintptr_t)label & 3) || ((uintptr_t)colour & 3) || ((uintptr_t)target & 3) ||
      ((uintptr_t)confidence & 3) || ((uintptr_t)confusion & 7) || ((uintptr_t)bad_targets & 7)) {
    set_error("ensemble_head: alignment (label, colour, target and confidence 4 B; confusion and bad_targets 8 B)");
    return MDIL_ENSEMBLE_ERR_INVALID;
  }
  const bool prob = mode == MDIL_ENSEMBLE_MODE_PROB;
  const long long nitems = (long long)N * Ho * (((long long)Wo + 1) >> 1);
  const int grid = bounded_grid(nitems, kWG, kMaxBlocks);
  // two weight tables of nc * 64 floats, then nc * 64 float2 once (S) or twice (S and E): at most 48 KB
  const size_t lds = (size_t)nc * 64 * sizeof(float) * (2 + (prob ? 4 : 2));
  auto* cf = reinterpret_cast<unsigned long long*>(confusion);
  auto* bt = reinterpret_cast<unsigned long long*>(bad_targets);
  if (prob)
    hipLaunchKernelGGL(ensemble_head_kernel<true>, dim3(grid), dim3(kWG), lds, (hipStream_t)stream, table,
                       nviews, w, bias, nitems, nc, Ho, Wo, id_map, palette, target, ignore_index, label,
                       colour, confidence, cf, bt);
  else
    hipLaunchKernelGGL(ensemble_head_kernel<false>, dim3(grid), dim3(kWG), lds, (hipStream_t)stream, table,
                       nviews, w, bias, nitems, nc, Ho, Wo, id_map, palette, target, ignore_index, label,
                       colour, confidence, cf, bt);
  return launched(kFn) ? MDIL_ENSEMBLE_OK : MDIL_ENSEMBLE_ERR_LAUNCH;
}
