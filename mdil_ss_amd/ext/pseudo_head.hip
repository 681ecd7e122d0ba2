// libmdil_pseudo.so: class-balanced pseudo-labels (gfx950).  Three kernels:
//
//   pseudo_head    Decoder.output_conv + argmax + the winner's softmax confidence, quantised to 16
//                  bits, + a [class][high byte] histogram of it.  predict_head.hip's kernel with two
//                  more outputs; the logits are never stored.
//   pseudo_refine  stored maps -> per class the histogram of the LOW byte inside one chosen high byte
//   pseudo_apply   stored maps -> the thresholded label map and its counters
//
//   l[n, 2h+a, 2w+b, c] = bias[c] + sum_ci x[n, h, w, ci] * W[ci][c][a][b]
//   label = argmax_c l,  conf = 1 / sum_c exp(l_c - l_max),  q = min(65535, (uint32)(conf * 65536.0f))
//
// Same chain as predict_head.hip, so label and conf are its bits: logits4 (bias first, ci
// ascending), vote, then a second walk that RECOMPUTES the logits, s += expf(l_c - l_max) with c
// ascending, conf = 1.f / s.  conf * 65536.0f is exact (a power of two, no overflow) and the cast
// truncates; conf = 1 gives 65536, clamped to 65535.  A NaN conf gives q = 0 and is counted.
//
// Why two bytes and two levels.  The k-th largest confidence of a class over a whole split is an
// order statistic of billions of values.  With q in 16 bits it is found EXACTLY from two 256-bin
// histograms: level 1 (here, in the head kernel) counts the high byte, the host walks it down to
// the byte that holds rank k; level 2 (pseudo_refine, over the stored q) counts the low byte of the
// pixels inside that high byte.  No sort, no floating-point reduction.
//
// Layout of pseudo_head.  As predict_head: a thread owns one feature pixel (16 channels in
// registers, four 16-byte loads), walks the classes over Wl[c][ci][a*2+b] in LDS (broadcast 16-byte
// reads), and writes the two adjacent pixels 2w, 2w+1 of output rows 2h, 2h+1 as one packed store
// per row and map (2 B label, 4 B qconf).  Grid-stride loop over feature pixels, 64-bit indices,
// bounded grid.  The work-group is 1024 lanes (16 waves, one work-group per CU) and the grid at most
// 256 of them, so that the [nc][256] histogram in LDS is flushed by few work-groups: a flush is up
// to nc * 256 global atomics, and 256 work-groups bound them at 2 M for any input size.
//
// LDS (static): 32 x 256 x 4 B = 32 KB of counters beside the 8.3 KB of head tables -- 41 KB, under
// the 64 KB a work-group may declare.  Counting: 32-bit LDS atomics; the (up to four) pixels of a
// thread that fall into one bin are added as one atomic (a trained head puts most of a class into
// bin 255, where every lane of a wave would otherwise queue four times on one address).  Flush: the
// non-zero counters, once per work-group after its loop (and every 2^19 trips, before a counter
// could wrap), by 64-bit integer global atomics.  No floating-point atomic anywhere.
//
// pseudo_refine / pseudo_apply.  A lane owns 8 consecutive pixels: one 8-byte label load, one
// 16-byte qconf load (and one 8-byte target load / out store); the last item of an odd-sized map
// goes byte by byte.  Counters live in LDS as above.  Runs of equal keys inside a lane's 8 pixels
// are added as one atomic: label maps are piecewise constant, so seen / kept / confusion mostly
// take one atomic per lane instead of eight on the same address.
#include "../../include/mdil_pseudo.h"
#include "map_common.h"

namespace {

constexpr int kMaxC = MDIL_PSEUDO_MAX_CLASSES;
constexpr int kHeadWG = 1024;                        // 16 wavefronts: one work-group per CU
constexpr int kHeadMaxBlocks = 256;                  // beyond 262,144 feature pixels the loop strides
constexpr int kMapWG = 256;                          // refine / apply: 4 wavefronts
constexpr int kMapMaxBlocks = 512;                   // beyond 131,072 items (of 8 pixels) the loop strides
constexpr int kFlushEvery = 1 << 19;                 // trips; a trip adds at most 4096 counts per work-group
constexpr char kFnHead[] = "pseudo_head";
constexpr char kFnRefine[] = "pseudo_refine";
constexpr char kFnApply[] = "pseudo_apply";

// The quantisation rule.  conf * 65536 is exact; the comparison keeps a NaN out of the cast.
__device__ __forceinline__ uint32_t quantise(float conf, uint32_t& nan_count) {
  if (conf != conf) {
    ++nan_count;
    return 0u;
  }
  const float v = conf * 65536.0f;
  return v >= 65535.0f ? 65535u : (uint32_t)v;
}

__global__ __launch_bounds__(kHeadWG) void pseudo_head_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
    long long npix, int W, int nc, unsigned char* __restrict__ label, unsigned short* __restrict__ qconf,
    u64* __restrict__ hist, u64* __restrict__ nonfinite) {
  __shared__ __attribute__((aligned(16))) float Wl[kMaxC][16][4];   // [c][ci][a*2+b]
  __shared__ float Bl[kMaxC];
  __shared__ uint32_t Pl[kMaxC];                                     // stage_head's palette slot, unused
  __shared__ uint32_t Hl[kMaxC * 256];                               // [label][q >> 8]
  __shared__ uint32_t nan_l;
  stage_head<kHeadWG, false>(w, bias, nullptr, nullptr, nullptr, nc, Wl, Bl, Pl, nullptr);
  for (int i = threadIdx.x; i < nc * 256; i += kHeadWG) Hl[i] = 0u;
  if (threadIdx.x == 0) nan_l = 0u;
  __syncthreads();

  int trips = 0;
  // the trip count is the same for every lane of the work-group (barriers inside)
  for (long long base = (long long)blockIdx.x * kHeadWG; base < npix;
       base += (long long)gridDim.x * kHeadWG) {
    const long long p = base + threadIdx.x;
    if (p < npix) {
      f32x4 xv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) xv[k] = *reinterpret_cast<const f32x4*>(x + p * 16 + k * 4);

      const f32x4 l0 = logits4(xv, Wl[0], Bl[0]);
      float best[4] = {l0[0], l0[1], l0[2], l0[3]};
      int bi[4] = {0, 0, 0, 0};
      for (int c = 1; c < nc; ++c) {
        const f32x4 l = logits4(xv, Wl[c], Bl[c]);
#pragma unroll
        for (int k = 0; k < 4; ++k) vote(c, l[k], best[k], bi[k]);   // c >= 1: class 0 entered above
      }

      const long long r = p / W;                                   // n * H + h
      const long long o0 = (2 * r * 2 * W) + 2 * (p - r * W);      // pixel (2h, 2w); row below: + 2W
      if (label) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
          *reinterpret_cast<uint16_t*>(label + o0 + (long long)a * 2 * W) =
              (uint16_t)(bi[a * 2] | bi[a * 2 + 1] << 8);
      }

      if (qconf || hist) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < nc; ++c) {
          const f32x4 l = logits4(xv, Wl[c], Bl[c]);
#pragma unroll
          for (int k = 0; k < 4; ++k) s[k] += expf(l[k] - best[k]);
        }
        uint32_t q[4], nans = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = quantise(1.f / s[k], nans);
        if (qconf) {
#pragma unroll
          for (int a = 0; a < 2; ++a)
            *reinterpret_cast<uint32_t*>(qconf + o0 + (long long)a * 2 * W) = q[a * 2] | q[a * 2 + 1] << 16;
        }
        if (hist) {
          Run run(Hl);
#pragma unroll
          for (int k = 0; k < 4; ++k) run.add(bi[k] * 256 + (int)(q[k] >> 8));
          run.done();
        }
        if (nans) atomicAdd(&nan_l, nans);
      }
    }

    const bool last = base + (long long)gridDim.x * kHeadWG >= npix;
    if (last || ++trips == kFlushEvery) {                          // uniform over the work-group
      trips = 0;
      __syncthreads();
      flush_counters<kHeadWG>(Hl, nc * 256, hist);
      if (threadIdx.x == 0 && nan_l) {
        if (nonfinite) atomicAdd(nonfinite, (u64)nan_l);
        nan_l = 0u;
      }
      __syncthreads();
    }
  }
}

// Eight labels / q values of item `item`: packed loads where the item is whole, bytes otherwise.
// -> how many of them exist (1 to 8).
__device__ __forceinline__ int load_item(const unsigned char* __restrict__ label,
                                         const unsigned short* __restrict__ qconf, long long item,
                                         long long npix, uint32_t (&lab)[kPerItem], uint32_t (&q)[kPerItem]) {
  const long long o = item * kPerItem;
  if (o + kPerItem <= npix) {
    const uint2 lv = *reinterpret_cast<const uint2*>(label + o);
    const uint4 qv = *reinterpret_cast<const uint4*>(qconf + o);
    const uint32_t lw[2] = {lv.x, lv.y}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
    for (int j = 0; j < kPerItem; ++j) {
      lab[j] = (lw[j >> 2] >> (8 * (j & 3))) & 0xffu;
      q[j] = (qw[j >> 1] >> (16 * (j & 1))) & 0xffffu;
    }
    return kPerItem;
  }
  const int n = (int)(npix - o);
#pragma unroll
  for (int j = 0; j < kPerItem; ++j) {
    lab[j] = j < n ? (uint32_t)label[o + j] : 0u;
    q[j] = j < n ? (uint32_t)qconf[o + j] : 0u;
  }
  return n;
}

__global__ __launch_bounds__(kMapWG) void pseudo_refine_kernel(
    const unsigned char* __restrict__ label, const unsigned short* __restrict__ qconf, long long npix,
    long long nitems, int nc, const int* __restrict__ sel, u64* __restrict__ hist2,
    u64* __restrict__ bad_labels) {
  __shared__ uint32_t Hl[kMaxC * 256];                               // [label][q & 255]
  __shared__ int Sl[kMaxC];
  __shared__ uint32_t bad_l;
  for (int i = threadIdx.x; i < nc * 256; i += kMapWG) Hl[i] = 0u;
  for (int c = threadIdx.x; c < nc; c += kMapWG) Sl[c] = sel[c];
  if (threadIdx.x == 0) bad_l = 0u;
  __syncthreads();

  int trips = 0;
  for (long long base = (long long)blockIdx.x * kMapWG; base < nitems;
       base += (long long)gridDim.x * kMapWG) {
    const long long item = base + threadIdx.x;
    if (item < nitems) {
      uint32_t lab[kPerItem], q[kPerItem];
      const int n = load_item(label, qconf, item, npix, lab, q);
      uint32_t bad = 0u;
      Run run(Hl);
#pragma unroll
      for (int j = 0; j < kPerItem; ++j) {
        if (j < n) {
          if (lab[j] >= (uint32_t)nc)
            ++bad;
          else if ((int)(q[j] >> 8) == Sl[lab[j]])
            run.add((int)(lab[j] * 256u + (q[j] & 255u)));
        }
      }
      run.done();
      if (bad) atomicAdd(&bad_l, bad);
    }

    const bool last = base + (long long)gridDim.x * kMapWG >= nitems;
    if (last || ++trips == kFlushEvery) {                          // uniform over the work-group
      trips = 0;
      __syncthreads();
      flush_counters<kMapWG>(Hl, nc * 256, hist2);
      if (threadIdx.x == 0 && bad_l) {
        atomicAdd(bad_labels, (u64)bad_l);
        bad_l = 0u;
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(kMapWG) void pseudo_apply_kernel(
    const unsigned char* __restrict__ label, const unsigned short* __restrict__ qconf, long long npix,
    long long nitems, int nc, const int* __restrict__ thr, const unsigned char* __restrict__ id_map,
    int drop_id, const unsigned char* __restrict__ target, int ignore_index, unsigned char* __restrict__ out,
    u64* __restrict__ seen, u64* __restrict__ kept, u64* __restrict__ confusion,
    u64* __restrict__ bad_targets, u64* __restrict__ bad_labels) {
  __shared__ uint32_t Cl[kMaxC * kMaxC];                             // [target][label], kept pixels
  __shared__ uint32_t Sl[kMaxC], Kl[kMaxC];                          // seen, kept
  __shared__ int Tl[kMaxC];                                          // thr
  __shared__ uint32_t Il[kMaxC];                                     // byte written for class c
  __shared__ uint32_t bad_t, bad_l;
  for (int i = threadIdx.x; i < nc * nc; i += kMapWG) Cl[i] = 0u;
  for (int c = threadIdx.x; c < nc; c += kMapWG) {
    Sl[c] = Kl[c] = 0u;
    Tl[c] = thr[c];
    Il[c] = id_map ? (uint32_t)id_map[c] : (uint32_t)c;
  }
  if (threadIdx.x == 0) bad_t = bad_l = 0u;
  __syncthreads();

  int trips = 0;
  for (long long base = (long long)blockIdx.x * kMapWG; base < nitems;
       base += (long long)gridDim.x * kMapWG) {
    const long long item = base + threadIdx.x;
    if (item < nitems) {
      uint32_t lab[kPerItem], q[kPerItem], tg[kPerItem];
      const int n = load_item(label, qconf, item, npix, lab, q);
      const long long o = item * kPerItem;
      if (target) {
        if (n == kPerItem) {
          const uint2 tv = *reinterpret_cast<const uint2*>(target + o);
          const uint32_t tw[2] = {tv.x, tv.y};
#pragma unroll
          for (int j = 0; j < kPerItem; ++j) tg[j] = (tw[j >> 2] >> (8 * (j & 3))) & 0xffu;
        } else {
#pragma unroll
          for (int j = 0; j < kPerItem; ++j) tg[j] = j < n ? (uint32_t)target[o + j] : 0u;
        }
      }
      uint32_t ob[kPerItem], nbad_l = 0u, nbad_t = 0u;
      Run seen_run(Sl), kept_run(Kl), conf_run(Cl);
#pragma unroll
      for (int j = 0; j < kPerItem; ++j) {
        ob[j] = (uint32_t)drop_id;
        if (j < n) {
          const bool lab_ok = lab[j] < (uint32_t)nc;
          bool keep = false;
          if (lab_ok) {
            keep = (int)q[j] >= Tl[lab[j]];
            seen_run.add((int)lab[j]);
            if (keep) {
              kept_run.add((int)lab[j]);
              ob[j] = Il[lab[j]];
            }
          } else {
            ++nbad_l;
          }
          if (target && (int)tg[j] != ignore_index) {
            if (tg[j] >= (uint32_t)nc)
              ++nbad_t;
            else if (keep)
              conf_run.add((int)(tg[j] * (uint32_t)nc + lab[j]));
          }
        }
      }
      seen_run.done();
      kept_run.done();
      conf_run.done();
      if (nbad_l) atomicAdd(&bad_l, nbad_l);
      if (nbad_t) atomicAdd(&bad_t, nbad_t);
      if (out) {
        if (n == kPerItem) {
          uint2 ov;
          ov.x = ob[0] | ob[1] << 8 | ob[2] << 16 | ob[3] << 24;
          ov.y = ob[4] | ob[5] << 8 | ob[6] << 16 | ob[7] << 24;
          *reinterpret_cast<uint2*>(out + o) = ov;
        } else {
#pragma unroll
          for (int j = 0; j < kPerItem; ++j)
            if (j < n) out[o + j] = (unsigned char)ob[j];
        }
      }
    }

    const bool last = base + (long long)gridDim.x * kMapWG >= nitems;
    if (last || ++trips == kFlushEvery) {                          // uniform over the work-group
      trips = 0;
      __syncthreads();
      flush_counters<kMapWG>(Sl, nc, seen);
      flush_counters<kMapWG>(Kl, nc, kept);
      flush_counters<kMapWG>(Cl, nc * nc, confusion);
      if (threadIdx.x == 0) {
        if (bad_t && bad_targets) atomicAdd(bad_targets, (u64)bad_t);
        if (bad_l && bad_labels) atomicAdd(bad_labels, (u64)bad_l);
        bad_t = bad_l = 0u;
      }
      __syncthreads();
    }
  }
}

inline bool maps_ok(const char* fn, const void* label, const void* qconf, long long npix) {
  if (!label || !qconf || npix <= 0) {
    set_error("%s: bad argument (label %p qconf %p npix %lld)", fn, label, qconf, npix);
    return false;
  }
  if (npix > MDIL_PSEUDO_MAX_PIXELS) {
    set_error("%s: too large (npix %lld: at most 2^40 pixels)", fn, npix);
    return false;
  }
  return true;
}

}  // namespace

API int mdil_pseudo_version(void) { return 100; }
API const char* mdil_pseudo_last_error(void) { return g_err; }

API int mdil_pseudo_head(const float* x, const float* w, const float* bias, int N, int H, int W, int nc,
                         unsigned char* label, unsigned short* qconf, long long* hist, long long* nonfinite,
                         void* stream) {
  if (!x || !w || !bias || N <= 0 || H <= 0 || W <= 0) {
    set_error("pseudo_head: bad argument (x %p w %p bias %p N %d H %d W %d)", (const void*)x, (const void*)w,
              (const void*)bias, N, H, W);
    return MDIL_PSEUDO_ERR_INVALID;
  }
  if (!label && !qconf && !hist) {
    set_error("pseudo_head: nothing to write (label, qconf and hist are all NULL)");
    return MDIL_PSEUDO_ERR_INVALID;
  }
  if (!classes_ok(kFnHead, nc, MDIL_PSEUDO_MIN_CLASSES, MDIL_PSEUDO_MAX_CLASSES)) return MDIL_PSEUDO_ERR_INVALID;
  if (((uintptr_t)x & 15) || ((uintptr_t)label & 1) || ((uintptr_t)qconf & 3) || ((uintptr_t)hist & 7) ||
      ((uintptr_t)nonfinite & 7)) {
    set_error("pseudo_head: alignment (x 16 B, label 2 B, qconf 4 B, hist and nonfinite 8 B)");
    return MDIL_PSEUDO_ERR_INVALID;
  }
  if (2LL * W > 0x7fffffffLL || (long long)N * H > MDIL_PSEUDO_MAX_PIXELS / 4 / W) {
    set_error("pseudo_head: too large (N %d, features %d x %d: at most 2^40 output pixels)", N, H, W);
    return MDIL_PSEUDO_ERR_INVALID;
  }
  const long long npix = (long long)N * H * W;
  const int grid = bounded_grid(npix, kHeadWG, kHeadMaxBlocks);
  hipLaunchKernelGGL(pseudo_head_kernel, dim3(grid), dim3(kHeadWG), 0, (hipStream_t)stream, x, w, bias, npix,
                     W, nc, label, qconf, reinterpret_cast<u64*>(hist), reinterpret_cast<u64*>(nonfinite));
  return launched(kFnHead) ? MDIL_PSEUDO_OK : MDIL_PSEUDO_ERR_LAUNCH;
}

API int mdil_pseudo_refine(const unsigned char* label, const unsigned short* qconf, long long npix, int nc,
                           const int* sel, long long* hist2, long long* bad_labels, void* stream) {
  if (!maps_ok(kFnRefine, label, qconf, npix)) return MDIL_PSEUDO_ERR_INVALID;
  if (!sel || !hist2 || !bad_labels) {
    set_error("pseudo_refine: bad argument (sel %p hist2 %p bad_labels %p)", (const void*)sel, (void*)hist2,
              (void*)bad_labels);
    return MDIL_PSEUDO_ERR_INVALID;
  }
  if (!classes_ok(kFnRefine, nc, MDIL_PSEUDO_MIN_CLASSES, MDIL_PSEUDO_MAX_CLASSES)) return MDIL_PSEUDO_ERR_INVALID;
  if (((uintptr_t)label & 7) || ((uintptr_t)qconf & 15) || ((uintptr_t)sel & 3) || ((uintptr_t)hist2 & 7) ||
      ((uintptr_t)bad_labels & 7)) {
    set_error("pseudo_refine: alignment (label 8 B, qconf 16 B, sel 4 B, hist2 and bad_labels 8 B)");
    return MDIL_PSEUDO_ERR_INVALID;
  }
  const long long nitems = (npix + kPerItem - 1) / kPerItem;
  const int grid = bounded_grid(nitems, kMapWG, kMapMaxBlocks);
  hipLaunchKernelGGL(pseudo_refine_kernel, dim3(grid), dim3(kMapWG), 0, (hipStream_t)stream, label, qconf, npix,
                     nitems, nc, sel, reinterpret_cast<u64*>(hist2), reinterpret_cast<u64*>(bad_labels));
  return launched(kFnRefine) ? MDIL_PSEUDO_OK : MDIL_PSEUDO_ERR_LAUNCH;
}

API int mdil_pseudo_apply(const unsigned char* label, const unsigned short* qconf, long long npix, int nc,
                          const int* thr, const unsigned char* id_map, int drop_id, const unsigned char* target,
                          int ignore_index, unsigned char* out, long long* seen, long long* kept,
                          long long* confusion, long long* bad_targets, long long* bad_labels, void* stream) {
  if (!maps_ok(kFnApply, label, qconf, npix)) return MDIL_PSEUDO_ERR_INVALID;
  if (!thr) {
    set_error("pseudo_apply: bad argument (thr %p)", (const void*)thr);
    return MDIL_PSEUDO_ERR_INVALID;
  }
  if (!classes_ok(kFnApply, nc, MDIL_PSEUDO_MIN_CLASSES, MDIL_PSEUDO_MAX_CLASSES)) return MDIL_PSEUDO_ERR_INVALID;
  if (drop_id < 0 || drop_id > 255) {
    set_error("pseudo_apply: drop_id=%d outside [0, 255]", drop_id);
    return MDIL_PSEUDO_ERR_INVALID;
  }
  if (target && (!confusion || !bad_targets)) {
    set_error("pseudo_apply: a target needs a confusion matrix and a bad_targets counter");
    return MDIL_PSEUDO_ERR_INVALID;
  }
  if (!ignore_ok(kFnApply, ignore_index)) return MDIL_PSEUDO_ERR_INVALID;
  if (((uintptr_t)label & 7) || ((uintptr_t)qconf & 15) || ((uintptr_t)thr & 3) || ((uintptr_t)target & 7) ||
      ((uintptr_t)out & 7) || ((uintptr_t)seen & 7) || ((uintptr_t)kept & 7) || ((uintptr_t)confusion & 7) ||
      ((uintptr_t)bad_targets & 7) || ((uintptr_t)bad_labels & 7)) {
    set_error("pseudo_apply: alignment (qconf 16 B; label, target, out and the counters 8 B; thr 4 B)");
    return MDIL_PSEUDO_ERR_INVALID;
  }
  const long long nitems = (npix + kPerItem - 1) / kPerItem;
  const int grid = bounded_grid(nitems, kMapWG, kMapMaxBlocks);
  hipLaunchKernelGGL(pseudo_apply_kernel, dim3(grid), dim3(kMapWG), 0, (hipStream_t)stream, label, qconf, npix,
                     nitems, nc, thr, id_map, drop_id, target, ignore_index, out, reinterpret_cast<u64*>(seen),
                     reinterpret_cast<u64*>(kept), reinterpret_cast<u64*>(confusion),
                     reinterpret_cast<u64*>(bad_targets), reinterpret_cast<u64*>(bad_labels));
  return launched(kFnApply) ? MDIL_PSEUDO_OK : MDIL_PSEUDO_ERR_LAUNCH;
}
