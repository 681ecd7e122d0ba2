// What the map add-ons share beyond head_common.h, written once: pseudo, openset, audit and acquire (a head
// kernel that counts into integer tables, then kernels over the stored 8- and 16-bit maps), route, whose head
// kernel walks the same per-parity chain, and ripu, whose kernels read stored maps alone.  Private to
// mdil_ss_amd/ext like head_common.h and compiled INTO each of the six libraries, which stay self-contained binaries.  It is a header of its own because
// head_common.h's device code is also compiled into predict / fullres / ensemble / drift / calib, whose
// bytes are not to move.  The arithmetic contracts (order of operations, roundings) are documented in the
// kernels' header comments; the helpers here are the single spelling of the steps they name.  Who uses what:
//   pseudo     u64, Run, flush_counters
//   openset    u64, kLog2e, is_finite, stage_parity, parity_logits, quad_bytes, cached_add, flush_cache, Run,
//              load_bytes, store_bytes, flush_counters
//   audit      u64, kLog2e, is_finite, wave_sum_u32, quad_bytes, Run, load_bytes, store_bytes, flush_counters
//   acquire    u64, kLog2e, is_finite, wave_sum_u32, quad_bytes, cached_add, flush_cache, Run, load_bytes,
//              store_bytes, flush_counters, kApplyFlushEvery, annotate_pixel, zero_annotator, flush_annotator
//              (audit_head and acquire_head keep stage_parity and parity_logits spelled out: as calls they cost
//              0.5 to 1.5 % of those kernels' time, past the measured margin; see the comments at the call sites)
//   route      kLog2e, is_finite, stage_parity, parity_logits
//   ripu       u64, Run, load_bytes, store_bytes, flush_counters, kApplyFlushEvery, annotate_pixel, zero_annotator,
//              flush_annotator (no head code)
//   spx        u64, cached_add, flush_cache, Run, load_bytes, store_bytes, flush_counters, kApplyFlushEvery, annotate_pixel,
//              zero_annotator, flush_annotator (no head code)
//   density    u64, is_finite, order_key16, wave_sum_u32, stage_parity, parity_logits, quad_bytes, cached_add_probed,
//              flush_cache (and of head_common.h: vote, shape_ok, classes_ok, bounded_grid, launched)
// What differs on purpose stays in its file, where a comment says why: the three quantise rules and code16, each
// file's wave_merged_add(s), route's fold_rows, pseudo_head's logits4 chain and its load_item.
#pragma once
#include "head_common.h"

#include <math.h>

namespace {

typedef unsigned long long u64;

constexpr float kLog2e = 1.4426950408889634f;
constexpr int kPerItem = 8;                          // pixels a lane of a map kernel owns
constexpr uint32_t kEmptySlot = 0xffffffffu;         // cached_add: no key; keys are below 2^31

__device__ __forceinline__ bool is_finite(float v) { return fabsf(v) < INFINITY; }   // false for a NaN

// The 16-bit code of a score (include/mdil_openset.h): the high half of the radix-sort key of its bits, order-preserving
// over all floats (NaNs aside).  openset_head.hip keeps its own spelling, code16; density_head.hip uses this one.
__device__ __forceinline__ uint32_t order_key16(float u) {
  const uint32_t bits = __float_as_uint(u);
  const uint32_t key = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  return key >> 16;
}

// Sum over the 64 lanes of a wave, every lane active.  Values below 2^26: the sum fits.
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
  return v;
}

// ------------------------------------------------------------------------- the per-parity head chain
// Stages the head's tables into LDS the way the per-parity chain reads them, by a work-group of WG lanes (the
// caller's barrier follows):  Wp[a*2+b][c][ci] = W[ci][c][a][b];  Bl[c] = bias[c].
template <int WG, int MAXC>
__device__ __forceinline__ void stage_parity(const float* __restrict__ w, const float* __restrict__ bias, int nc,
                                             float (&Wp)[4][MAXC][16], float (&Bl)[MAXC]) {
  for (int i = threadIdx.x; i < nc * 64; i += WG) {
    const int k = i & 3, ci = (i >> 2) & 15, c = i >> 6;
    Wp[k][c][ci] = w[(ci * nc + c) * 4 + k];
  }
  for (int i = threadIdx.x; i < nc; i += WG) Bl[i] = bias[i];
}

// The logits d[c], c < nc, of parity `par` (= a*2+b) for one feature pixel: bias first, then ci ascending, every
// step an explicit FMA (predict_head.hip's chain, so a vote over d gives predict's label bit for bit).
template <int MAXC>
__device__ __forceinline__ void parity_logits(const f32x4 (&xv)[4], const float (&Wp)[4][MAXC][16],
                                              const float (&Bl)[MAXC], int par, int nc, float (&d)[MAXC]) {
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    if (c < nc) {
      float a = Bl[c];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(&Wp[par][c][k * 4]);
#pragma unroll
        for (int e = 0; e < 4; ++e) a = __builtin_fmaf(xv[k][e], wv[e], a);
      }
      d[c] = a;
    }
  }
}

// The four bytes (byte a*2+b) that a u8 map of row length 2 W holds for the feature pixel whose output pixel
// (2h, 2w) lies at o0: one 2-byte load per row.
__device__ __forceinline__ uint32_t quad_bytes(const unsigned char* __restrict__ map, long long o0, int W) {
  return (uint32_t) * reinterpret_cast<const uint16_t*>(map + o0) |
         (uint32_t) * reinterpret_cast<const uint16_t*>(map + o0 + 2LL * W) << 16;
}

// ------------------------------------------------------------------------- a work-group's table of adds
// table[slot] += n by way of the work-group's direct-mapped LDS table of SLOTS (key, 32-bit count) pairs: the
// slot's entry is claimed for its key by a compare-and-swap or found to hold it already; an entry that holds
// another key sends the add to global memory instead (a 64-bit atomic, relaxed, agent scope).
template <int SLOTS>
__device__ __forceinline__ void cached_add(u64* __restrict__ table, uint32_t* tags, uint32_t* counts, uint32_t slot,
                                           uint32_t n) {
  static_assert(SLOTS > 1 && (SLOTS & (SLOTS - 1)) == 0, "the hash keeps log2(SLOTS) bits");
  const uint32_t h = (slot * 2654435761u) >> (32 - __builtin_ctz(SLOTS));   // below SLOTS
  const uint32_t old = atomicCAS(&tags[h], kEmptySlot, slot);
  if (old == kEmptySlot || old == slot)
    atomicAdd(&counts[h], n);
  else
    __hip_atomic_fetch_add(table + slot, (u64)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// cached_add that tries PROBES slots (h, h ^ 1, ...) before the add goes to global memory; flush_cache serves both.
template <int SLOTS, int PROBES>
__device__ __forceinline__ void cached_add_probed(u64* __restrict__ table, uint32_t* tags, uint32_t* counts,
                                                  uint32_t slot, uint32_t n) {
  static_assert(SLOTS > 1 && (SLOTS & (SLOTS - 1)) == 0 && PROBES >= 1 && PROBES <= SLOTS, "the hash keeps log2(SLOTS) bits");
  const uint32_t h = (slot * 2654435761u) >> (32 - __builtin_ctz(SLOTS));
#pragma unroll
  for (uint32_t probe = 0; probe < (uint32_t)PROBES; ++probe) {
    const uint32_t hh = h ^ probe;
    const uint32_t old = atomicCAS(&tags[hh], kEmptySlot, slot);
    if (old == kEmptySlot || old == slot) {
      atomicAdd(&counts[hh], n);
      return;
    }
  }
  __hip_atomic_fetch_add(table + slot, (u64)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The occupied entries -> the global table, by the whole work-group of WG lanes, and the table is empty again;
// the caller's barriers surround it.
template <int WG, int SLOTS>
__device__ __forceinline__ void flush_cache(u64* __restrict__ table, uint32_t* tags, uint32_t* counts) {
  for (int i = threadIdx.x; i < SLOTS; i += WG) {
    const uint32_t slot = tags[i];
    if (slot != kEmptySlot) {
      const uint32_t v = counts[i];
      if (v) __hip_atomic_fetch_add(table + slot, (u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      tags[i] = kEmptySlot;
      counts[i] = 0u;
    }
  }
}

// ------------------------------------------------------------------------- the map kernels
// counters[i] (32-bit, LDS) -> global[i] (64-bit), the non-zero ones, by the whole work-group of WG lanes; a
// NULL destination only clears them.  The caller's barriers surround it.
template <int WG>
__device__ __forceinline__ void flush_counters(uint32_t* counters, int n, u64* global) {
  for (int i = threadIdx.x; i < n; i += WG) {
    const uint32_t v = counters[i];
    if (v) {
      if (global) __hip_atomic_fetch_add(global + i, (u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      counters[i] = 0u;
    }
  }
}

// A run of equal keys: `add(key)` extends it or, on another key, sends it to counters[key] as one
// LDS atomic; `done()` sends the last run.  key < 0: nothing to count.
struct Run {
  uint32_t* counters;
  int key;
  uint32_t n;
  __device__ __forceinline__ explicit Run(uint32_t* c) : counters(c), key(-1), n(0u) {}
  __device__ __forceinline__ void done() {
    if (key >= 0) atomicAdd(&counters[key], n);
    key = -1;
    n = 0u;
  }
  __device__ __forceinline__ void add(int k) {
    if (k != key) {
      done();
      key = k;
    }
    ++n;
  }
};

// Eight bytes of a u8 map at item offset o: one packed load where the item is whole, bytes otherwise.
__device__ __forceinline__ void load_bytes(const unsigned char* __restrict__ map, long long o, int n,
                                           uint32_t (&v)[kPerItem]) {
  if (n == kPerItem) {
    const uint2 t = *reinterpret_cast<const uint2*>(map + o);
    const uint32_t tw[2] = {t.x, t.y};
#pragma unroll
    for (int j = 0; j < kPerItem; ++j) v[j] = (tw[j >> 2] >> (8 * (j & 3))) & 0xffu;
  } else {
#pragma unroll
    for (int j = 0; j < kPerItem; ++j) v[j] = j < n ? (uint32_t)map[o + j] : 0u;
  }
}

__device__ __forceinline__ void store_bytes(unsigned char* __restrict__ map, long long o, int n,
                                            const uint32_t (&v)[kPerItem]) {
  if (n == kPerItem) {
    uint2 t;
    t.x = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
    t.y = v[4] | v[5] << 8 | v[6] << 16 | v[7] << 24;
    *reinterpret_cast<uint2*>(map + o) = t;
  } else {
#pragma unroll
    for (int j = 0; j < kPerItem; ++j)
      if (j < n) map[o + j] = (unsigned char)v[j];
  }
}

// ------------------------------------------------------------------------- the annotator's rule
// What acquire_apply and ripu_apply do with one pixel, and how their work-groups count.  They differ in where `sel`
// comes from (a tile look-up that steps along the row; a byte that equals 255) and in ripu's two wrong counts, which
// stay in their files.
constexpr int kApplyFlushEvery = 1 << 19;            // trips; a trip adds at most 2048 counts per work-group

// One pixel, whose ob and mb come in as drop_id and 0: selected -> the target (where there is one), 255 in the mask;
// else `previous` where that is not drop_id -> kept, 128; else `fill` where that is not drop_id -> filled, 64.  A
// NULL map is absent and its byte (tg, pv, fl) is not read.  The three runs count the classes below nc; nshown counts the selected
// pixels, nbad the selected targets that are neither a class nor ignore_index.
__device__ __forceinline__ void annotate_pixel(bool sel, const unsigned char* target, const uint32_t& tg,
                                               const unsigned char* previous, const uint32_t& pv,
                                               const unsigned char* fill, const uint32_t& fl, int nc, int ignore_index,
                                               int drop_id, Run& ann_run, Run& kept_run, Run& fill_run, uint32_t& ob,
                                               uint32_t& mb, uint32_t& nshown, uint32_t& nbad) {
  if (sel) {
    ++nshown;
    mb = 255u;
    if (target) {
      ob = tg;
      if ((int)tg != ignore_index) {
        if (tg < (uint32_t)nc)
          ann_run.add((int)tg);
        else
          ++nbad;
      }
    }
  } else if (previous && pv != (uint32_t)drop_id) {
    ob = pv;
    mb = 128u;
    if (pv < (uint32_t)nc) kept_run.add((int)pv);
  } else if (fill && fl != (uint32_t)drop_id) {
    ob = fl;
    mb = 64u;
    if (fl < (uint32_t)nc) fill_run.add((int)fl);
  }
}

// The work-group's LDS counters before its first item: Al / Kl / Fl (annotated, kept, filled per class) and the K
// scalar ones.  The barrier is inside.
template <int WG, int K>
__device__ __forceinline__ void zero_annotator(uint32_t* Al, uint32_t* Kl, uint32_t* Fl, int nc, uint32_t (&misc)[K]) {
  for (int c = threadIdx.x; c < nc; c += WG) Al[c] = Kl[c] = Fl[c] = 0u;
  if (threadIdx.x < K) misc[threadIdx.x] = 0u;
  __syncthreads();
}

// Those counters -> global memory (NULL destinations only clear), and they are zero again; called where the whole
// work-group arrives: after its last trip and every kApplyFlushEvery trips.  The barriers are inside.
template <int WG, int K>
__device__ __forceinline__ void flush_annotator(uint32_t* Al, uint32_t* Kl, uint32_t* Fl, int nc, u64* annotated,
                                                u64* kept, u64* filled, uint32_t (&misc)[K], u64* const (&dst)[K]) {
  __syncthreads();
  flush_counters<WG>(Al, nc, annotated);
  flush_counters<WG>(Kl, nc, kept);
  flush_counters<WG>(Fl, nc, filled);
  if (threadIdx.x < K) {
    const uint32_t v = misc[threadIdx.x];
    if (v && dst[threadIdx.x])
      __hip_atomic_fetch_add(dst[threadIdx.x], (u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    misc[threadIdx.x] = 0u;
  }
  __syncthreads();
}

}  // namespace
