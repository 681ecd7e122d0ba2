// libmdil_drift.so: two checkpoints compared at their heads, fused (gfx950).  Both
// Decoder.output_conv, both softmaxes, the per-pixel KL divergence, both argmaxes, the
// class-transition counts, both confusion matrices and the retained / forgotten / gained counts in
// one pass over the two 16-channel feature maps.
//
//   l^M[n, 2h+a, 2w+b, c] = bias^M[c] + sum_ci x^M[n, h, w, ci] * W^M[ci][c][a][b]        M in {A, B}
//   label_M = argmax_c l^M,  z^M_c = l^M_c - max - log sum_c exp(l^M_c - max),  p^M_c = exp(z^M_c)
//   kl = sum_c p^A_c (z^A_c - z^B_c),  kd = sum_c p^A_c (z^A_c - p^B_c)
//
// At batch 6 and 1024x512 the two logit tensors are 252 MB each that the unfused route writes and
// reads back several times; here 100 MB of features come in and 4 to 38 MB of maps go out.
//
// Layout (predict_head.hip's).  A lane owns one feature pixel of BOTH models: 2 x 16 channels (eight
// 16-byte loads) stay in registers and it walks the classes, forming the four logits (a, b) of one
// class and model at a time with predict_head's FMA chain (bias first, ci ascending: the same
// bits, so the labels are that kernel's labels).  Both heads sit in LDS as Wl[c][ci][a*2+b]: one
// broadcast 16-byte read gives the four parity weights of a (class, input channel) pair.  No logit
// is kept: the walk is repeated with the same chain -- once for the maxima and the labels, and, only
// when kl_map or sums is asked for, once for sum exp(l - max) and once for z, p and the two sums
// over the classes (c ascending, fp32).  That is 2 x 64 x nc FMAs per feature pixel and walk.
// Stores: the two adjacent pixels 2w, 2w+1 of output rows 2h and 2h+1 as one packed store per row and
// map (2 B label_a, label_b, change; 8 B kl_map); the target is read the same way.  Work-group-uniform
// grid-stride loop over feature pixels (wave reductions and barriers inside) with 64-bit indices
// and a bounded grid.
//
// Counters.  Each work-group counts into 32-bit histograms in LDS (LDS atomics) and adds its
// non-zero entries to the 64-bit matrices with global atomic adds after its loop (and every 2^20
// trips, before a counter could wrap).  Integer adds commute: the result is exact in any order.
//
// Sums.  No floating-point atomics.  sums[c], c < nc: per trip and class present in the wave, the
// lanes' (at most four) fp32 kl values of that class are added in fp64 (pixel order), reduced over
// the wave by a fixed xor-shuffle tree, and added by lane 0 to the wave's own fp64 slot in LDS.
// sums[nc]: a lane adds its kd values to an fp64 register (pixel order over its trips); one tree
// at the end.  After the loop the four waves' slots are added in wave order and stored to the
// caller's workspace, one row of nc + 1 doubles per work-group.  A second launch (head_common.h's
// fold_kernel, nc + 1 wavefronts) adds the rows -- lane l the rows l, l + 64, ... ascending, then
// the same tree -- and adds the total to sums[c].  The grid is a function of N * H * W, so the order is fixed by the shape.
#include "../../include/mdil_drift.h"
#include "head_common.h"

namespace {

constexpr int kWG = 256;                             // 4 wavefronts of 64 lanes
constexpr int kWaves = kWG / 64;
constexpr int kMaxC = MDIL_DRIFT_MAX_CLASSES;
constexpr int kMaxBlocks = 2048;                     // beyond 524,288 feature pixels the loop strides
constexpr int kFlushEvery = 1 << 20;                 // trips; a trip adds at most 1024 counts per histogram
constexpr long long kMaxPixels = 1LL << 38;          // feature pixels: 4 * npix and the trip count stay small
constexpr char kFn[] = "drift_head";

struct DriftArgs {
  const float *xa, *wa, *ba, *xb, *wb, *bb;
  long long npix;
  int W, nc;
  const unsigned char* target;
  int ignore_index;
  unsigned char *label_a, *label_b;
  float* kl_map;
  unsigned char* change;
  unsigned long long *transition, *confusion_a, *confusion_b, *outcome, *bad_targets;
  double* workspace;                                 // NULL without sums
};

__device__ __forceinline__ void flush(uint32_t* hist, unsigned long long* out, int n) {
  if (!out) return;
  for (int i = threadIdx.x; i < n; i += kWG) {
    const uint32_t v = hist[i];
    if (v) {
      atomicAdd(out + i, (unsigned long long)v);
      hist[i] = 0u;
    }
  }
}

// 2 waves per SIMD: 207 VGPRs, no scratch (unbounded the allocator takes 280 and one wave; at 3 it spills)
__global__ __launch_bounds__(kWG, 2) void drift_head_kernel(const DriftArgs p) {
  __shared__ __attribute__((aligned(16))) float WlA[kMaxC][16][4];  // [c][ci][a*2+b]
  __shared__ __attribute__((aligned(16))) float WlB[kMaxC][16][4];
  __shared__ float BlA[kMaxC], BlB[kMaxC];
  __shared__ uint32_t Pl[kMaxC];                      // stage_head's palette slot: no colour map here
  __shared__ uint32_t hT[kMaxC * kMaxC];              // [label_a][label_b]
  __shared__ uint32_t hA[kMaxC * kMaxC];              // [target][label_a]
  __shared__ uint32_t hB[kMaxC * kMaxC];              // [target][label_b]
  __shared__ uint32_t hO[kMaxC * 4];                  // [target][both right, forgotten, gained, both wrong]
  __shared__ uint32_t bad;
  __shared__ double wsum[kWaves][kMaxC + 1];          // a wave's own slots: only its lane 0 adds
  const int nc = p.nc;
  stage_head<kWG, false>(p.wa, p.ba, nullptr, nullptr, nullptr, nc, WlA, BlA, Pl, nullptr);
  stage_head<kWG, false>(p.wb, p.bb, nullptr, nullptr, nullptr, nc, WlB, BlB, Pl, nullptr);
  confusion_zero<kWG>(hT, bad, nc);
  for (int i = threadIdx.x; i < nc * nc; i += kWG) hA[i] = hB[i] = 0u;
  for (int i = threadIdx.x; i < nc * 4; i += kWG) hO[i] = 0u;
  for (int i = threadIdx.x; i < kWaves * (kMaxC + 1); i += kWG) (&wsum[0][0])[i] = 0.0;
  __syncthreads();

  const unsigned char* __restrict__ target = p.target;
  const bool soft = p.kl_map || p.workspace;          // the two extra walks
  const bool counting = p.transition || p.confusion_a || p.confusion_b || p.outcome || p.bad_targets;
  const int W = p.W, ignore_index = p.ignore_index;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double kd_acc = 0.0;
  int trips = 0;

  // the trip count is the same for every lane of the work-group (wave reductions and barriers inside)
  for (long long base = (long long)blockIdx.x * kWG; base < p.npix; base += (long long)gridDim.x * kWG) {
    const long long q = base + threadIdx.x;
    int cls[4] = {-1, -1, -1, -1};                    // class whose sum the pixel's kl enters; -1: none
    float kl[4] = {0.f, 0.f, 0.f, 0.f};
    if (q < p.npix) {
      f32x4 xa[4], xb[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        xa[k] = *reinterpret_cast<const f32x4*>(p.xa + q * 16 + k * 4);
        xb[k] = *reinterpret_cast<const f32x4*>(p.xb + q * 16 + k * 4);
      }

      // walk 1: maxima and labels
      float ma[4], mb[4];
      int ia[4] = {0, 0, 0, 0}, ib[4] = {0, 0, 0, 0};
      {
        const f32x4 la = logits4(xa, WlA[0], BlA[0]), lb = logits4(xb, WlB[0], BlB[0]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          ma[k] = la[k];
          mb[k] = lb[k];
        }
      }
      for (int c = 1; c < nc; ++c) {
        const f32x4 la = logits4(xa, WlA[c], BlA[c]), lb = logits4(xb, WlB[c], BlB[c]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {                 // c >= 1: class 0 entered above
          vote(c, la[k], ma[k], ia[k]);
          vote(c, lb[k], mb[k], ib[k]);
        }
      }

      float kd[4] = {0.f, 0.f, 0.f, 0.f};
      if (soft) {
        // walk 2: log sum exp(l - max), the same logits again
        float sa[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < nc; ++c) {
          const f32x4 la = logits4(xa, WlA[c], BlA[c]), lb = logits4(xb, WlB[c], BlB[c]);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            sa[k] += expf(la[k] - ma[k]);
            sb[k] += expf(lb[k] - mb[k]);
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          sa[k] = logf(sa[k]);
          sb[k] = logf(sb[k]);
        }
        // walk 3: z, p and the two sums over the classes, c ascending
        for (int c = 0; c < nc; ++c) {
          const f32x4 la = logits4(xa, WlA[c], BlA[c]), lb = logits4(xb, WlB[c], BlB[c]);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float za = (la[k] - ma[k]) - sa[k], zb = (lb[k] - mb[k]) - sb[k];
            const float pa = expf(za), pb = expf(zb);
            kl[k] += pa * (za - zb);
            kd[k] += pa * (za - pb);
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) kd_acc += (double)kd[k];   // every pixel: the trainer's KLD masks nothing
      }

      const long long r = q / W;                               // n * H + h
      const long long o0 = (2 * r * 2 * W) + 2 * (q - r * W);  // pixel (2h, 2w); row below: + 2W
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const long long o = o0 + (long long)a * 2 * W;
        const uint32_t tg = target ? (uint32_t)*reinterpret_cast<const uint16_t*>(target + o) : 0u;
        uint32_t code[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int k = a * 2 + b;
          const int t = (int)((tg >> (8 * b)) & 0xffu);
          const bool counted = !target || (t < nc && t != ignore_index);
          const bool ar = ia[k] == t, br = ib[k] == t;
          code[b] = !target ? (uint32_t)(ia[k] != ib[k])
                            : !counted ? 255u
                                       : ar ? (br ? 0u : 1u) : br ? 2u : ia[k] == ib[k] ? 3u : 4u;
          cls[k] = counted ? (target ? t : ia[k]) : -1;
          if (counting) {
            if (counted) {
              if (p.transition) atomicAdd(&hT[ia[k] * nc + ib[k]], 1u);
              if (target) {
                if (p.confusion_a) atomicAdd(&hA[t * nc + ia[k]], 1u);
                if (p.confusion_b) atomicAdd(&hB[t * nc + ib[k]], 1u);
                if (p.outcome) atomicAdd(&hO[t * 4 + (int)min(code[b], 3u)], 1u);
              }
            } else if (t != ignore_index && p.bad_targets) {   // not counted: there is a target
              atomicAdd(&bad, 1u);
            }
          }
        }
        if (p.label_a) *reinterpret_cast<uint16_t*>(p.label_a + o) = (uint16_t)(ia[a * 2] | ia[a * 2 + 1] << 8);
        if (p.label_b) *reinterpret_cast<uint16_t*>(p.label_b + o) = (uint16_t)(ib[a * 2] | ib[a * 2 + 1] << 8);
        if (p.change) *reinterpret_cast<uint16_t*>(p.change + o) = (uint16_t)(code[0] | code[1] << 8);
        if (p.kl_map) {
          float2 v;
          v.x = kl[a * 2];
          v.y = kl[a * 2 + 1];
          *reinterpret_cast<float2*>(p.kl_map + o) = v;
        }
      }
    }

    if (p.workspace) {                                 // uniform over the work-group: every lane is here
      for (int c = 0; c < nc; ++c) {
        const bool has = cls[0] == c || cls[1] == c || cls[2] == c || cls[3] == c;
        if (__ballot(has)) {                           // uniform over the wave
          double v = 0.0;
#pragma unroll
          for (int k = 0; k < 4; ++k) v += cls[k] == c ? (double)kl[k] : 0.0;
          v = wave_sum(v);
          if (lane == 0) wsum[wave][c] += v;
        }
      }
    }

    const bool last = base + (long long)gridDim.x * kWG >= p.npix;
    if (counting && (last || ++trips == kFlushEvery)) {  // uniform over the work-group
      trips = 0;
      __syncthreads();
      flush(hT, p.transition, nc * nc);
      flush(hA, p.confusion_a, nc * nc);
      flush(hB, p.confusion_b, nc * nc);
      flush(hO, p.outcome, nc * 4);
      if (threadIdx.x == 0 && bad) {
        atomicAdd(p.bad_targets, (unsigned long long)bad);
        bad = 0u;
      }
      __syncthreads();
    }
  }

  if (p.workspace) {
    const double v = wave_sum(kd_acc);
    if (lane == 0) wsum[wave][nc] = v;
    __syncthreads();
    if ((int)threadIdx.x <= nc) {
      double t = wsum[0][threadIdx.x];
#pragma unroll
      for (int i = 1; i < kWaves; ++i) t += wsum[i][threadIdx.x];
      p.workspace[(long long)blockIdx.x * (nc + 1) + threadIdx.x] = t;
    }
  }
}

}  // namespace

API int mdil_drift_version(void) { return 100; }
API const char* mdil_drift_last_error(void) { return g_err; }

API long long mdil_drift_workspace_bytes(int N, int H, int W, int nc) {
  if (!shape_ok(N, H, W, kMaxPixels) || nc < MDIL_DRIFT_MIN_CLASSES || nc > MDIL_DRIFT_MAX_CLASSES) return -1;
  return (long long)bounded_grid((long long)N * H * W, kWG, kMaxBlocks) * (nc + 1) * (long long)sizeof(double);
}

API int mdil_drift_head(const float* xa, const float* wa, const float* ba, const float* xb, const float* wb,
                        const float* bb, int N, int H, int W, int nc, const unsigned char* target,
                        int ignore_index, unsigned char* label_a, unsigned char* label_b, float* kl_map,
                        unsigned char* change, long long* transition, long long* confusion_a,
                        long long* confusion_b, long long* outcome, long long* bad_targets, double* sums,
                        void* workspace, long long workspace_bytes, void* stream) {
  if (!xa || !wa || !ba || !xb || !wb || !bb || N <= 0 || H <= 0 || W <= 0) {
    set_error("drift_head: bad argument (xa %p wa %p ba %p xb %p wb %p bb %p N %d H %d W %d)", (const void*)xa,
              (const void*)wa, (const void*)ba, (const void*)xb, (const void*)wb, (const void*)bb, N, H, W);
    return MDIL_DRIFT_ERR_INVALID;
  }
  if (!classes_ok(kFn, nc, MDIL_DRIFT_MIN_CLASSES, MDIL_DRIFT_MAX_CLASSES)) return MDIL_DRIFT_ERR_INVALID;
  if (!shape_ok(N, H, W, kMaxPixels)) {
    set_error("drift_head: too large (N %d, features %d x %d: at most 2^38 pixels, W below 2^30)", N, H, W);
    return MDIL_DRIFT_ERR_INVALID;
  }
  if (!ignore_ok(kFn, ignore_index)) return MDIL_DRIFT_ERR_INVALID;
  if (!target && (confusion_a || confusion_b || outcome)) {
    set_error("drift_head: confusion_a, confusion_b and outcome need a target");
    return MDIL_DRIFT_ERR_INVALID;
  }
  if (((uintptr_t)xa & 15) || ((uintptr_t)xb & 15) || ((uintptr_t)target & 1) || ((uintptr_t)label_a & 1) ||
      ((uintptr_t)label_b & 1) || ((uintptr_t)change & 1) || ((uintptr_t)kl_map & 7) ||
      ((uintptr_t)transition & 7) || ((uintptr_t)confusion_a & 7) || ((uintptr_t)confusion_b & 7) ||
      ((uintptr_t)outcome & 7) || ((uintptr_t)bad_targets & 7) || ((uintptr_t)sums & 7) ||
      ((uintptr_t)workspace & 7)) {
    set_error("drift_head: alignment (xa and xb 16 B; target, label_a, label_b and change 2 B; kl_map, the "
              "counters, sums and workspace 8 B)");
    return MDIL_DRIFT_ERR_INVALID;
  }
  const long long npix = (long long)N * H * W;
  const int grid = bounded_grid(npix, kWG, kMaxBlocks);
  const long long need = (long long)grid * (nc + 1) * (long long)sizeof(double);
  if (!workspace_ok(kFn, sums, workspace, workspace_bytes, need)) return MDIL_DRIFT_ERR_INVALID;
  DriftArgs p;
  p.xa = xa, p.wa = wa, p.ba = ba, p.xb = xb, p.wb = wb, p.bb = bb;
  p.npix = npix, p.W = W, p.nc = nc;
  p.target = target, p.ignore_index = ignore_index;
  p.label_a = label_a, p.label_b = label_b, p.kl_map = kl_map, p.change = change;
  p.transition = reinterpret_cast<unsigned long long*>(transition);
  p.confusion_a = reinterpret_cast<unsigned long long*>(confusion_a);
  p.confusion_b = reinterpret_cast<unsigned long long*>(confusion_b);
  p.outcome = reinterpret_cast<unsigned long long*>(outcome);
  p.bad_targets = reinterpret_cast<unsigned long long*>(bad_targets);
  p.workspace = sums ? static_cast<double*>(workspace) : nullptr;
  hipLaunchKernelGGL(drift_head_kernel, dim3(grid), dim3(kWG), 0, (hipStream_t)stream, p);
  if (!launched(kFn)) return MDIL_DRIFT_ERR_LAUNCH;
  if (sums) {
    hipLaunchKernelGGL(fold_kernel<>, dim3(nc + 1), dim3(64), 0, (hipStream_t)stream, p.workspace, grid, nc + 1,
                       sums);
    if (!launched(kFn)) return MDIL_DRIFT_ERR_LAUNCH;
  }
  return MDIL_DRIFT_OK;
}
