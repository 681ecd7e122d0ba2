// libmdil_fullres.so: Decoder.output_conv, a bilinear resize of the logits to Ho x Wo, the
// per-pixel argmax and the confusion matrix against a target of that size, fused (gfx950).
//
//   l[n, 2h+a, 2w+b, c] = bias[c] + sum_ci x[n, h, w, ci] * W[ci][c][a][b]        Hl = 2H, Wl = 2W
//   U_c[n, yo, xo]      = wy0 wx0 l[y0, x0] + wy0 wx1 l[y0, x0+1] + wy1 wx0 l[y0+1, x0] + wy1 wx1 l[y0+1, x0+1]
//   label = id_map[argmax_c U_c],  colour = palette[argmax_c U_c],  confusion[target][argmax] += 1
//
// At batch 6 the logits are 252 MB and, resized to 2048x1024, 1 GB that the unfused path writes and
// reads back to keep one byte per pixel; here 50 MB of features come in and 12.6 MB of labels go out.
//
// Source coordinates (include/mdil_fullres.h) are integers: y0 = num / den, rem = num % den with
// num = (2 yo + 1) Hl - Ho, den = 2 Ho, so no coordinate is ever rounded; rem = 0 where num < 0 or
// y0 = Hl - 1 (clamped edges: full weight on y0).
//
// Order of operations, and the roundings on the longest path to a compared logit:
//   1. wy1 = (float)rem / (float)den, wy0 = (float)(den - rem) / (float)den: operands exact
//      (< 2^24), one correctly rounded division each; wx0, wx1 alike.  wy0 is NOT 1 - wy1.  (1 + 1)
//   2. wt[a][b] = wy[a] * wx[b]: one product.                                                  (1)
//      The rows y0, y0+1 have the two parities a of the transposed conv, the columns x0, x0+1 the
//      two parities b, so the four neighbours are the four kernel positions (a, b), each once.
//   3. s[ci][a*2+b] = wt[a][b] * x_ab[ci], x_ab the feature pixel under the neighbour of parity
//      (a, b): one product.                                                                    (1)
//   4. U_c = fma chain from bias[c] over ci ascending, inside ci over a*2+b ascending:
//      acc = fma(s[ci][k], W[ci][c][k], acc), 64 FMAs, one rounding each.                     (64)
//   A term of the sum carries 4 roundings before the chain (two quotients, their product, the
//   scaling) and at most 64 in it:
//   k = 68 roundings, |U_c - exact| <= gamma_68 * (|bias_c| + bilinear(sum_ci |x| |W|)).
//   5. argmax: strictly greater replaces, so the lowest class keeps a tie; a NaN replaces any
//      number and is never replaced.  id_map / palette are looked up after it.
//
// Layout.  A lane owns four horizontally adjacent output pixels of one row (one 4-byte label
// store, three 4-byte colour stores, one 4-byte target load when Wo is a multiple of 4; bytes
// otherwise).  They share the row's y0, weights and feature rows.  They are worked off as two
// pairs: the four scaled feature pixels of each pixel of a pair sit in 2 x 64 registers (the
// parity slots are picked with ?: on y0 & 1 / x0 & 1 while LOADING, so no register array is
// indexed at run time), and each class is one walk over Wl[c][ci][a*2+b] in LDS -- one broadcast
// 16-byte read per (class, channel) feeds the 8 FMAs of the pair.  64 FMAs per class and pixel.
// The class count is a run-time loop bound.  Work-group-uniform grid-stride loop over the lanes'
// items with 64-bit indices and a bounded grid.
//
// Confusion.  Each work-group counts into a [nc][nc] histogram of 32-bit counters in LDS (LDS
// atomics) and adds its non-zero entries to the 64-bit matrix with global atomic adds after its
// loop (and every 2^20 trips, before a counter could wrap).  Every item is visited by exactly one
// lane once, so every pixel is counted once whatever the grid is.
#include "../../include/mdil_fullres.h"
#include "head_common.h"

namespace {

constexpr int kWG = 256;                             // 4 wavefronts of 64 lanes
constexpr int kMaxC = MDIL_FULLRES_MAX_CLASSES;
constexpr int kMaxBlocks = 2048;                     // beyond 524,288 items (of 4 pixels) the loop strides
constexpr int kFlushEvery = 1 << 20;                 // trips; a trip adds at most 1024 counts per work-group
constexpr char kFn[] = "fullres_head";

__global__ __launch_bounds__(kWG, 2) void fullres_head_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
    long long nitems, int H, int W, int nc, int Ho, int Wo,
    const unsigned char* __restrict__ id_map, const unsigned char* __restrict__ palette,
    const unsigned char* __restrict__ target, int ignore_index, unsigned char* __restrict__ label,
    unsigned char* __restrict__ colour, unsigned long long* __restrict__ confusion,
    unsigned long long* __restrict__ bad_targets) {
  __shared__ __attribute__((aligned(16))) float Wl[kMaxC][16][4];   // [c][ci][a*2+b]
  __shared__ float Bl[kMaxC];
  __shared__ uint32_t Pl[kMaxC];                                     // r | g << 8 | b << 16
  __shared__ uint32_t Il[kMaxC];                                     // byte written for class c
  __shared__ uint32_t hist[kMaxC * kMaxC];                           // [target][prediction]
  __shared__ uint32_t bad;
  stage_head<kWG, true>(w, bias, palette, colour, id_map, nc, Wl, Bl, Pl, Il);
  confusion_zero<kWG>(hist, bad, nc);
  __syncthreads();

  const int Hl = 2 * H, Wlog = 2 * W;
  const long long G = ((long long)Wo + 3) >> 2;          // items per output row
  const bool packed = (Wo & 3) == 0;                      // every item's four pixels exist and are 4-byte aligned
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

      int y0;
      float wy0, wy1;
      axis(yo, Hl, Ho, y0, wy0, wy1);
      const bool oddy = y0 & 1;
      const int h0 = y0 >> 1, h1 = min((y0 + 1) >> 1, H - 1);
      const long long rowoff[2] = {(n * H + (oddy ? h1 : h0)) * W, (n * H + (oddy ? h0 : h1)) * W};
      const float wy[2] = {oddy ? wy1 : wy0, oddy ? wy0 : wy1};

      uint32_t preds = 0;                                  // four train ids, one per byte
#pragma unroll 1
      for (int half = 0; half < 2; ++half) {
        f32x4 s0[16], s1[16];
        const int xa = min(4 * g + 2 * half, Wo - 1), xb = min(4 * g + 2 * half + 1, Wo - 1);
        gather(x, rowoff, wy, xa, Wlog, Wo, W, false, s0);
        __builtin_amdgcn_sched_barrier(0);                 // one pixel's 16 loads in flight at a time
        gather(x, rowoff, wy, xb, Wlog, Wo, W, false, s1);
        __builtin_amdgcn_sched_barrier(0);
        float best0 = 0.f, best1 = 0.f;
        int bi0 = 0, bi1 = 0;
        for (int c = 0; c < nc; ++c) {
          float u0 = Bl[c], u1 = u0;
#pragma unroll
          for (int ci = 0; ci < 16; ++ci) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(Wl[c][ci]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              u0 = __builtin_fmaf(s0[ci][k], wv[k], u0);
              u1 = __builtin_fmaf(s1[ci][k], wv[k], u1);
            }
          }
          // head_common.h's vote, spelled out: calling it changes this kernel's register allocation
          // (254 -> 222 VGPRs) and instruction mix.  Strictly greater keeps the lowest index of a
          // tie; a NaN replaces any number and is never replaced; class 0 always enters
          const bool t0 = c == 0 || u0 > best0 || (u0 != u0 && best0 == best0);
          const bool t1 = c == 0 || u1 > best1 || (u1 != u1 && best1 == best1);
          best0 = t0 ? u0 : best0;
          bi0 = t0 ? c : bi0;
          best1 = t1 ? u1 : best1;
          bi1 = t1 ? c : bi1;
        }
        preds |= ((uint32_t)bi0 | (uint32_t)bi1 << 8) << (16 * half);
      }

      const long long o = r * Wo + 4LL * g;                // first pixel of the item
      uint32_t tg = 0;
      if (target) {
        if (packed) {
          tg = *reinterpret_cast<const uint32_t*>(target + o);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (4 * g + j < Wo) tg |= (uint32_t)target[o + j] << (8 * j);
        }
      }
      uint32_t lab = 0, pc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t p = (preds >> (8 * j)) & 0xffu;
        lab |= Il[p] << (8 * j);
        pc[j] = Pl[p];
        if (target && 4 * g + j < Wo) {
          const int t = (int)((tg >> (8 * j)) & 0xffu);
          if (t != ignore_index) {
            if (t < nc)
              atomicAdd(&hist[t * nc + (int)p], 1u);
            else
              atomicAdd(&bad, 1u);
          }
        }
      }
      if (packed) {
        *reinterpret_cast<uint32_t*>(label + o) = lab;
        if (colour) {
          uint32_t* cp = reinterpret_cast<uint32_t*>(colour + o * 3);
          cp[0] = pc[0] | pc[1] << 24;
          cp[1] = pc[1] >> 8 | pc[2] << 16;
          cp[2] = pc[2] >> 16 | pc[3] << 8;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (4 * g + j < Wo) {
            label[o + j] = (unsigned char)(lab >> (8 * j));
            if (colour) {
              unsigned char* cp = colour + (o + j) * 3;
              cp[0] = (unsigned char)pc[j];
              cp[1] = (unsigned char)(pc[j] >> 8);
              cp[2] = (unsigned char)(pc[j] >> 16);
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
        const uint32_t v = hist[i];
        if (v) {
          atomicAdd(confusion + i, (unsigned long long)v);
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

API int mdil_fullres_version(void) { return 100; }
API const char* mdil_fullres_last_error(void) { return g_err; }

API int mdil_fullres_head(const float* x, const float* w, const float* bias, int N, int H, int W,
                          int nc, int Ho, int Wo, const unsigned char* id_map,
                          const unsigned char* palette, const unsigned char* target,
                          int ignore_index, unsigned char* label, unsigned char* colour,
                          long long* confusion, long long* bad_targets, void* stream) {
  if (!x || !w || !bias || !label || N <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) {
    set_error("fullres_head: bad argument (x %p w %p bias %p label %p N %d H %d W %d Ho %d Wo %d)",
              (const void*)x, (const void*)w, (const void*)bias, (void*)label, N, H, W, Ho, Wo);
    return MDIL_FULLRES_ERR_INVALID;
  }
  if (!classes_ok(kFn, nc, MDIL_FULLRES_MIN_CLASSES, MDIL_FULLRES_MAX_CLASSES) ||
      !out_size_ok(kFn, Ho, Wo, MDIL_FULLRES_MAX_SIZE))
    return MDIL_FULLRES_ERR_INVALID;
  if (H > (1 << 29) || W > (1 << 29) || (long long)N * H > MDIL_FULLRES_MAX_PIXELS / W ||
      (long long)N * Ho > MDIL_FULLRES_MAX_PIXELS / Wo) {
    set_error("fullres_head: too large (N %d, features %d x %d, output %d x %d: at most 2^40 pixels)",
              N, H, W, Ho, Wo);
    return MDIL_FULLRES_ERR_INVALID;
  }
  if (!colour_ok(kFn, colour, palette) || !scoring_ok(kFn, target, confusion, bad_targets, ignore_index))
    return MDIL_FULLRES_ERR_INVALID;
  if (((uintptr_t)x & 15) || ((uintptr_t)label & 3) || ((uintptr_t)colour & 3) ||
      ((uintptr_t)target & 3) || ((uintptr_t)confusion & 7) || ((uintptr_t)bad_targets & 7)) {
    set_error("fullres_head: alignment (x 16 B; label, colour and target 4 B; confusion and bad_targets 8 B)");
    return MDIL_FULLRES_ERR_INVALID;
  }
  const long long nitems = (long long)N * Ho * (((long long)Wo + 3) >> 2);
  const int grid = bounded_grid(nitems, kWG, kMaxBlocks);
  hipLaunchKernelGGL(fullres_head_kernel, dim3(grid), dim3(kWG), 0, (hipStream_t)stream, x, w, bias,
                     nitems, H, W, nc, Ho, Wo, id_map, palette, target, ignore_index, label, colour,
                     reinterpret_cast<unsigned long long*>(confusion),
                     reinterpret_cast<unsigned long long*>(bad_targets));
  return launched(kFn) ? MDIL_FULLRES_OK : MDIL_FULLRES_ERR_LAUNCH;
}
