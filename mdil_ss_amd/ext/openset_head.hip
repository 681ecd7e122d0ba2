// libmdil_openset.so: which pixels does the head not know (gfx950).  Two kernels:
//
//   openset_head   Decoder.output_conv + argmax + four "unknown" scores per pixel (1 - p_top, -max logit,
//                  free energy, entropy), the 16-bit order-preserving code of one of them as a map, and per
//                  score a [group][code] histogram.  route_head.hip's chain with other outputs; the logits
//                  are never stored.
//   openset_apply  stored maps -> the label map with a reject id, the 8-bit score map, their counters
//
// The chain is route_head.hip's, through the same helpers of map_common.h (Wp[a*2+b][c][ci] in LDS, the logits of
// one parity in registers, vote, then c ascending: d_c, one hardware exp2, s, A), so `label` is predict_head's bits and
// `ent` route_head's.  From m, s, A:  conf = 1 / s,  logs = logf(s),  ent = logs - A conf, and
//      msp = (s - 1) conf,  maxlogit = -m,  energy = -(m + logs),  entropy = ent,      each + 0.0f.
// The code of a score is the high half of the usual radix-sort key of its bits (sign flipped for positive
// numbers, all bits for negative ones): monotone, no parameter, no range to choose.
//
// Layout of openset_head.  A lane owns one feature pixel (16 channels in registers) and walks its four
// parities.  The grid is bounded and the loop over feature pixels strides; its trip count is the same for
// every lane of a wave (a lane past the end computes a clamped pixel and writes nothing), because the
// histogram step below talks to the whole wave.
//
// The histogram is 4 x 2 x 65536 64-bit counters, 4 MiB: it lives in global memory and is added to with
// 64-bit integer atomics (relaxed, agent scope).  Two stages keep most adds away from it:
//   1. In the wave, lanes that hold the same (kind, group, code) are merged: the lowest lane that still has
//      something to add broadcasts its key (readlane), a ballot finds every lane with that key, the leader
//      carries their number as ONE add, and the matched lanes retire.  After kMergeRounds rounds whatever is
//      left goes on as adds of 1: an image region of one texture merges in a round or two, white noise pays
//      kMergeRounds ballots and then what it would have paid anyway.
//   2. In the work-group, an add goes to a direct-mapped table of kCacheSlots (key, 32-bit count) pairs in LDS
//      (map_common.h's cached_add and flush_cache): the slot is claimed by a compare-and-swap on its key; a
//      slot that another key holds sends the add to global memory instead.  After its loop the work-group adds
//      its occupied slots to the global table.  The grid is at most kHeadMaxBlocks work-groups, so a code that
//      every pixel shares costs that many global atomics, not one per wave and parity (measured first without
//      this stage: 0.6 ms on all-zero features, 2.7 ms on the network's, against 0.08 ms for the kernel without
//      a histogram).
// A slot's count cannot wrap: a work-group sees at most 2^40 / 4 / kHeadMaxBlocks feature pixels of a full
// grid, four adds of one kind each: under 2^31.  Integer sums: the result does not depend on the order of arrival.
//
// openset_apply.  pseudo_apply's layout: a lane owns 8 consecutive pixels (one 8-byte label load, one
// 16-byte code load, 8-byte target load / out and score stores; the last item of an odd-sized map goes byte
// by byte); the counters live in LDS as 32-bit integers, runs of equal keys inside a lane's 8 pixels are one
// LDS atomic, and a work-group flushes its non-zero counters once by 64-bit global atomics.
#include "../../include/mdil_openset.h"
#include "map_common.h"

#include <float.h>

namespace {

constexpr int kMaxC = MDIL_OPENSET_MAX_CLASSES;
constexpr int kKinds = MDIL_OPENSET_KINDS;
constexpr int kCodes = MDIL_OPENSET_CODES;
constexpr int kHeadWG = 256;                         // 4 wavefronts of 64 lanes
constexpr int kHeadMaxBlocks = 768;                  // three per CU (LDS, registers); beyond 196,608 feature pixels the loop strides
constexpr int kCacheSlots = 4096;                    // LDS table of (key, count): 32 KB
constexpr int kMergeRounds = 8;                      // ballot rounds per (parity, kind) before plain atomics
constexpr int kMapWG = 256;
constexpr int kMapMaxBlocks = 512;                   // beyond 131,072 items (of 8 pixels) the loop strides
constexpr int kFlushEvery = 1 << 19;                 // trips; a trip adds at most 2048 counts per work-group
constexpr char kFnHead[] = "openset_head";
constexpr char kFnApply[] = "openset_apply";

// The 16-bit code of a score: order-preserving over all floats (NaNs aside, which never get here).
__device__ __forceinline__ uint32_t code16(float u) {
  const uint32_t bits = __float_as_uint(u);
  const uint32_t key = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  return key >> 16;
}

// One add per distinct `slot` among the lanes of the wave with `active`: every lane of the wave calls it
// (the caller's loop is wave-uniform).  slot < 2^31.
__device__ __forceinline__ void wave_merged_add(u64* __restrict__ hist, uint32_t* tags, uint32_t* counts,
                                                uint32_t slot, bool active) {
  const int lane = threadIdx.x & 63;
  u64 todo = __ballot(active);
  for (int round = 0; round < kMergeRounds && todo; ++round) {
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
    const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)slot, leader);
    const u64 same = __ballot(active && slot == s0);
    if (lane == leader) cached_add<kCacheSlots>(hist, tags, counts, s0, (uint32_t)__popcll(same));
    active = active && slot != s0;
    todo &= ~same;
  }
  if (active) cached_add<kCacheSlots>(hist, tags, counts, slot, 1u);
}

// 2 waves per SIMD like route_head: the 32 logits of a parity stay in registers
__global__ __launch_bounds__(kHeadWG, 2) void openset_head_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, long long npix, int W,
    int nc, const unsigned char* __restrict__ target, const unsigned char* __restrict__ group_lut, int const_group,
    int kinds, int map_kind, unsigned char* __restrict__ label, unsigned short* __restrict__ code,
    u64* __restrict__ hist, u64* __restrict__ nonfinite) {
  __shared__ __attribute__((aligned(16))) float Wp[4][kMaxC][16];   // [a*2+b][c][ci]
  __shared__ float Bl[kMaxC];
  __shared__ uint32_t Gl[256];                                       // group of a target byte
  __shared__ uint32_t Tl[kCacheSlots], Cl[kCacheSlots];              // the histogram's table: key, count
  __shared__ uint32_t nf;
  static_assert(MDIL_OPENSET_MAX_PIXELS / 4 / kHeadMaxBlocks * 4 <= 0x80000000LL, "a slot's count could wrap");
  stage_parity<kHeadWG>(w, bias, nc, Wp, Bl);
  if (hist) {
    for (int i = threadIdx.x; i < kCacheSlots; i += kHeadWG) {
      Tl[i] = kEmptySlot;
      Cl[i] = 0u;
    }
  }
  for (int i = threadIdx.x; i < 256; i += kHeadWG) Gl[i] = target ? (uint32_t)group_lut[i] : (uint32_t)const_group;
  if (threadIdx.x == 0) nf = 0u;
  __syncthreads();

  uint32_t bad = 0u;
  // the trip count is the same for every lane of the work-group
  for (long long base = (long long)blockIdx.x * kHeadWG; base < npix; base += (long long)gridDim.x * kHeadWG) {
    const bool valid = base + threadIdx.x < npix;
    const long long p = valid ? base + threadIdx.x : npix - 1;     // a lane past the end: a clamped pixel, no writes
    f32x4 xv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xv[k] = *reinterpret_cast<const f32x4*>(x + p * 16 + k * 4);
    const long long r = p / W;                                     // n * H + h
    const long long o0 = (2 * r * 2 * W) + 2 * (p - r * W);        // pixel (2h, 2w); row below: + 2W
    uint32_t groups = 0u;                                          // byte a*2+b
    if (target) groups = quad_bytes(target, o0, W);
    uint32_t labels = 0u, codes_top = 0u, codes_bottom = 0u;       // byte a*2+b; the two pixels of a row

#pragma unroll 1
    for (int par = 0; par < 4; ++par) {
      float d[kMaxC];
      parity_logits<kMaxC>(xv, Wp, Bl, par, nc, d);                  // predict_head.hip's chain, per parity
      float m = 0.f;
      int bi = 0;
#pragma unroll
      for (int c = 0; c < kMaxC; ++c)
        if (c < nc) vote(c, d[c], m, bi);
      labels |= (uint32_t)bi << (8 * par);
      if (!code && !hist && !nonfinite) continue;                  // label alone: no score is formed

      float s = 0.f, A = 0.f;
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) {
        if (c < nc) {
          float v = d[c] - m;
          v = v == -INFINITY ? -FLT_MAX : v;                       // 0 * d_c stays 0; a NaN stays a NaN
          const float e = __builtin_amdgcn_exp2f(__fmul_rn(v, kLog2e));
          s += e;
          A = __builtin_fmaf(e, v, A);
        }
      }
      const float logs = logf(s);
      const float conf = 1.0f / s;
      const float ent = __fsub_rn(logs, __fmul_rn(A, conf));
      const bool finite = is_finite(s) && is_finite(m);
      float score[kKinds];
      score[0] = __fadd_rn(__fmul_rn(__fsub_rn(s, 1.0f), conf), 0.0f);
      score[1] = __fadd_rn(-m, 0.0f);
      score[2] = __fadd_rn(-__fadd_rn(m, logs), 0.0f);
      score[3] = __fadd_rn(ent, 0.0f);
      uint32_t cd[kKinds];
#pragma unroll
      for (int k = 0; k < kKinds; ++k) cd[k] = code16(score[k]);

      if (code) {
        uint32_t mine = cd[0];
#pragma unroll
        for (int k = 1; k < kKinds; ++k) mine = map_kind == k ? cd[k] : mine;
        mine = finite ? mine : (uint32_t)MDIL_OPENSET_NONFINITE_CODE;
        if (par < 2)
          codes_top |= mine << (16 * (par & 1));
        else
          codes_bottom |= mine << (16 * (par & 1));
      }
      bad += valid && !finite ? 1u : 0u;
      if (hist) {
        const uint32_t g = target ? Gl[(groups >> (8 * par)) & 0xffu] : (uint32_t)const_group;
        const bool counts = valid && finite && g < 2u;
#pragma unroll
        for (int k = 0; k < kKinds; ++k)
          if (kinds >> k & 1)                                      // uniform over the grid
            wave_merged_add(hist, Tl, Cl, ((uint32_t)(k * 2) + (g & 1u)) * (uint32_t)kCodes + cd[k], counts);
      }
    }

    if (valid && label) {
      *reinterpret_cast<uint16_t*>(label + o0) = (uint16_t)(labels & 0xffffu);
      *reinterpret_cast<uint16_t*>(label + o0 + 2LL * W) = (uint16_t)(labels >> 16);
    }
    if (valid && code) {
      *reinterpret_cast<uint32_t*>(code + o0) = codes_top;
      *reinterpret_cast<uint32_t*>(code + o0 + 2LL * W) = codes_bottom;
    }
  }

  if (bad) atomicAdd(&nf, bad);
  __syncthreads();                                                 // every lane of the work-group is here
  if (nonfinite && threadIdx.x == 0 && nf) atomicAdd(nonfinite, (u64)nf);
  if (hist) flush_cache<kHeadWG, kCacheSlots>(hist, Tl, Cl);
}

__global__ __launch_bounds__(kMapWG) void openset_apply_kernel(
    const unsigned char* __restrict__ label, const unsigned short* __restrict__ code, long long npix, long long nitems,
    int nc, int thr, const unsigned char* __restrict__ id_map, int unknown_id, const unsigned char* __restrict__ cdf_lut,
    const unsigned char* __restrict__ target, const unsigned char* __restrict__ group_lut,
    unsigned char* __restrict__ out, unsigned char* __restrict__ score, u64* __restrict__ seen,
    u64* __restrict__ rejected, u64* __restrict__ detect, u64* __restrict__ confusion, u64* __restrict__ bad_targets,
    u64* __restrict__ bad_labels) {
  __shared__ uint32_t Cl[kMaxC * kMaxC];                             // [target][label], accepted pixels of group 0
  __shared__ uint32_t Sl[kMaxC], Rl[kMaxC];                          // seen, rejected
  __shared__ uint32_t Dl[4];                                         // [group][rejected]
  __shared__ uint32_t Il[kMaxC];                                     // byte written for class c
  __shared__ uint32_t Gl[256];                                       // group of a target byte
  __shared__ uint32_t bad_t, bad_l;
  for (int i = threadIdx.x; i < nc * nc; i += kMapWG) Cl[i] = 0u;
  for (int c = threadIdx.x; c < nc; c += kMapWG) {
    Sl[c] = Rl[c] = 0u;
    Il[c] = id_map ? (uint32_t)id_map[c] : (uint32_t)c;
  }
  for (int i = threadIdx.x; i < 256; i += kMapWG) Gl[i] = target ? (uint32_t)group_lut[i] : 2u;
  if (threadIdx.x < 4) Dl[threadIdx.x] = 0u;
  if (threadIdx.x == 0) bad_t = bad_l = 0u;
  __syncthreads();

  int trips = 0;
  for (long long base = (long long)blockIdx.x * kMapWG; base < nitems; base += (long long)gridDim.x * kMapWG) {
    const long long item = base + threadIdx.x;
    if (item < nitems) {
      const long long o = item * kPerItem;
      const int n = o + kPerItem <= npix ? kPerItem : (int)(npix - o);
      uint32_t lab[kPerItem], cd[kPerItem], tg[kPerItem];
      load_bytes(label, o, n, lab);
      if (n == kPerItem) {
        const uint4 cv = *reinterpret_cast<const uint4*>(code + o);
        const uint32_t cw[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
        for (int j = 0; j < kPerItem; ++j) cd[j] = (cw[j >> 1] >> (16 * (j & 1))) & 0xffffu;
      } else {
#pragma unroll
        for (int j = 0; j < kPerItem; ++j) cd[j] = j < n ? (uint32_t)code[o + j] : 0u;
      }
      if (target) load_bytes(target, o, n, tg);

      uint32_t ob[kPerItem], sb[kPerItem], nbad_l = 0u, nbad_t = 0u;
      Run seen_run(Sl), rej_run(Rl), det_run(Dl), conf_run(Cl);
#pragma unroll
      for (int j = 0; j < kPerItem; ++j) {
        ob[j] = (uint32_t)unknown_id;
        sb[j] = 0u;
        if (j < n) {
          if (score) sb[j] = (uint32_t)cdf_lut[cd[j]];
          if (lab[j] >= (uint32_t)nc) {
            ++nbad_l;
          } else {
            const bool rej = (int)cd[j] >= thr;
            seen_run.add((int)lab[j]);
            if (rej)
              rej_run.add((int)lab[j]);
            else
              ob[j] = Il[lab[j]];
            if (target) {
              const uint32_t g = Gl[tg[j]];
              if (g < 2u) det_run.add((int)(g * 2u + (rej ? 1u : 0u)));
              if (g == 0u) {
                if (tg[j] >= (uint32_t)nc)
                  ++nbad_t;
                else if (!rej)
                  conf_run.add((int)(tg[j] * (uint32_t)nc + lab[j]));
              }
            }
          }
        }
      }
      seen_run.done();
      rej_run.done();
      det_run.done();
      conf_run.done();
      if (nbad_l) atomicAdd(&bad_l, nbad_l);
      if (nbad_t) atomicAdd(&bad_t, nbad_t);
      if (out) store_bytes(out, o, n, ob);
      if (score) store_bytes(score, o, n, sb);
    }

    const bool last = base + (long long)gridDim.x * kMapWG >= nitems;
    if (last || ++trips == kFlushEvery) {                          // uniform over the work-group
      trips = 0;
      __syncthreads();
      flush_counters<kMapWG>(Sl, nc, seen);
      flush_counters<kMapWG>(Rl, nc, rejected);
      flush_counters<kMapWG>(Dl, 4, detect);
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

}  // namespace

API int mdil_openset_version(void) { return 100; }
API const char* mdil_openset_last_error(void) { return g_err; }

API int mdil_openset_head(const float* x, const float* w, const float* bias, int N, int H, int W, int nc,
                          const unsigned char* target, const unsigned char* group_lut, int const_group, int kinds,
                          int map_kind, unsigned char* label, unsigned short* code, long long* hist,
                          long long* nonfinite, void* stream) {
  if (!x || !w || !bias || N <= 0 || H <= 0 || W <= 0) {
    set_error("openset_head: bad argument (x %p w %p bias %p N %d H %d W %d)", (const void*)x, (const void*)w,
              (const void*)bias, N, H, W);
    return MDIL_OPENSET_ERR_INVALID;
  }
  if (!label && !code && !hist && !nonfinite) {
    set_error("openset_head: nothing to write (label, code, hist and nonfinite are all NULL)");
    return MDIL_OPENSET_ERR_INVALID;
  }
  if (!classes_ok(kFnHead, nc, MDIL_OPENSET_MIN_CLASSES, MDIL_OPENSET_MAX_CLASSES)) return MDIL_OPENSET_ERR_INVALID;
  if (kinds < 1 || kinds > 15) {
    set_error("openset_head: kinds=%d outside [1, 15] (a bit mask: 1 msp, 2 maxlogit, 4 energy, 8 entropy)", kinds);
    return MDIL_OPENSET_ERR_INVALID;
  }
  if (map_kind < -1 || map_kind >= MDIL_OPENSET_KINDS || (code != nullptr) != (map_kind >= 0)) {
    set_error("openset_head: map_kind=%d with code %p (a code map needs a map_kind in [0, 3]; without one map_kind "
              "is -1)", map_kind, (void*)code);
    return MDIL_OPENSET_ERR_INVALID;
  }
  if (const_group < 0 || const_group > 2) {
    set_error("openset_head: const_group=%d outside [0, 2]", const_group);
    return MDIL_OPENSET_ERR_INVALID;
  }
  if (target && !group_lut) {
    set_error("openset_head: a target needs its group_lut (u8 [256])");
    return MDIL_OPENSET_ERR_INVALID;
  }
  if (((uintptr_t)x & 15) || ((uintptr_t)w & 3) || ((uintptr_t)bias & 3) || ((uintptr_t)target & 1) ||
      ((uintptr_t)label & 1) || ((uintptr_t)code & 3) || ((uintptr_t)hist & 7) || ((uintptr_t)nonfinite & 7)) {
    set_error("openset_head: alignment (x 16 B; w and bias 4 B; target and label 2 B; code 4 B; hist and nonfinite "
              "8 B)");
    return MDIL_OPENSET_ERR_INVALID;
  }
  if (2LL * W > 0x7fffffffLL || (long long)N * H > MDIL_OPENSET_MAX_PIXELS / 4 / W) {
    set_error("openset_head: too large (N %d, features %d x %d: at most 2^40 output pixels)", N, H, W);
    return MDIL_OPENSET_ERR_INVALID;
  }
  const long long npix = (long long)N * H * W;
  const int grid = bounded_grid(npix, kHeadWG, kHeadMaxBlocks);
  hipLaunchKernelGGL(openset_head_kernel, dim3(grid), dim3(kHeadWG), 0, (hipStream_t)stream, x, w, bias, npix, W, nc,
                     target, group_lut, const_group, kinds, map_kind, label, code, reinterpret_cast<u64*>(hist),
                     reinterpret_cast<u64*>(nonfinite));
  return launched(kFnHead) ? MDIL_OPENSET_OK : MDIL_OPENSET_ERR_LAUNCH;
}

API int mdil_openset_apply(const unsigned char* label, const unsigned short* code, long long npix, int nc, int thr,
                           const unsigned char* id_map, int unknown_id, const unsigned char* cdf_lut,
                           const unsigned char* target, const unsigned char* group_lut, unsigned char* out,
                           unsigned char* score, long long* seen, long long* rejected, long long* detect,
                           long long* confusion, long long* bad_targets, long long* bad_labels, void* stream) {
  if (!label || !code || npix <= 0) {
    set_error("openset_apply: bad argument (label %p code %p npix %lld)", (const void*)label, (const void*)code, npix);
    return MDIL_OPENSET_ERR_INVALID;
  }
  if (npix > MDIL_OPENSET_MAX_PIXELS) {
    set_error("openset_apply: too large (npix %lld: at most 2^40 pixels)", npix);
    return MDIL_OPENSET_ERR_INVALID;
  }
  if (!classes_ok(kFnApply, nc, MDIL_OPENSET_MIN_CLASSES, MDIL_OPENSET_MAX_CLASSES)) return MDIL_OPENSET_ERR_INVALID;
  if (thr < 0 || thr > MDIL_OPENSET_CODES) {
    set_error("openset_apply: thr=%d outside [0, 65536]", thr);
    return MDIL_OPENSET_ERR_INVALID;
  }
  if (unknown_id < 0 || unknown_id > 255) {
    set_error("openset_apply: unknown_id=%d outside [0, 255]", unknown_id);
    return MDIL_OPENSET_ERR_INVALID;
  }
  if ((score != nullptr) != (cdf_lut != nullptr)) {
    set_error("openset_apply: a score map and a cdf_lut (u8 [65536]) go together (score %p cdf_lut %p)", (void*)score,
              (const void*)cdf_lut);
    return MDIL_OPENSET_ERR_INVALID;
  }
  if (target && (!group_lut || !detect || !confusion || !bad_targets)) {
    set_error("openset_apply: a target needs its group_lut, a detect table, a confusion matrix and a bad_targets "
              "counter");
    return MDIL_OPENSET_ERR_INVALID;
  }
  if (!out && !score && !seen && !rejected && !detect && !confusion && !bad_targets && !bad_labels) {
    set_error("openset_apply: nothing to write (out, score and every counter are NULL)");
    return MDIL_OPENSET_ERR_INVALID;
  }
  if (((uintptr_t)label & 7) || ((uintptr_t)code & 15) || ((uintptr_t)target & 7) || ((uintptr_t)out & 7) ||
      ((uintptr_t)score & 7) || ((uintptr_t)seen & 7) || ((uintptr_t)rejected & 7) || ((uintptr_t)detect & 7) ||
      ((uintptr_t)confusion & 7) || ((uintptr_t)bad_targets & 7) || ((uintptr_t)bad_labels & 7)) {
    set_error("openset_apply: alignment (code 16 B; label, target, out, score and the counters 8 B)");
    return MDIL_OPENSET_ERR_INVALID;
  }
  const long long nitems = (npix + kPerItem - 1) / kPerItem;
  const int grid = bounded_grid(nitems, kMapWG, kMapMaxBlocks);
  // without a target the counters that need one are not added to, whatever was given
  hipLaunchKernelGGL(openset_apply_kernel, dim3(grid), dim3(kMapWG), 0, (hipStream_t)stream, label, code, npix, nitems,
                     nc, thr, id_map, unknown_id, cdf_lut, target, group_lut, out, score, reinterpret_cast<u64*>(seen),
                     reinterpret_cast<u64*>(rejected), reinterpret_cast<u64*>(target ? detect : nullptr),
                     reinterpret_cast<u64*>(target ? confusion : nullptr),
                     reinterpret_cast<u64*>(target ? bad_targets : nullptr), reinterpret_cast<u64*>(bad_labels));
  return launched(kFnApply) ? MDIL_OPENSET_OK : MDIL_OPENSET_ERR_LAUNCH;
}
