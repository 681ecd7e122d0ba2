// libmdil_acquire.so: which regions of a new domain to label first (gfx950).  Two kernels:
//
//   acquire_head    Decoder.output_conv + argmax + one uncertainty per pixel (1 - p_top, normalised entropy or
//                   1 - top-2 margin) as a LINEAR 16-bit q, and per tile of the label grid the integer table
//                   [pixels, sum q, wrong, with a valid target, nc label counts].  route_head.hip's chain with
//                   other outputs; the logits are never stored.
//   acquire_apply   stored maps + the chosen tiles -> the label map an annotator hands back, the mask of where
//                   each label came from, their counters
//
// The chain is route_head.hip's, spelled the same way (Wp[a*2+b][c][ci] in LDS, the logits of one parity in
// registers, vote, then c ascending: d_c, one hardware exp2, s, A, e2), so `label` is predict_head's bits and
// ent / margin route_head's.  logf(s) is formed for kind 1 alone (kind is uniform over the grid).
//
// Layout of acquire_head.  A lane owns one feature pixel (16 channels in registers) and walks its four
// parities.  Tile sizes are even, so the four outputs of a lane lie in ONE tile: a lane first sums its own
// four pixels in registers (pixels, wrong and valid packed into one word, q in another) and keeps its four
// labels as bytes.  The grid is bounded and the loop over feature pixels strides; its trip count is the same
// for every lane of a work-group (a lane past the end computes a clamped pixel, writes nothing and counts
// nothing), because the steps below talk to the whole wave and the whole work-group.
//
// The adds, once per feature pixel (not per parity).
//   1. In the wave, by tile: the lowest lane that still has something to add broadcasts its tile (readlane),
//      a ballot finds every lane of that tile, two xor-shuffle trees sum their packed counts and their q, and
//      the leader carries them as ONE add per field.  Inside that round the labels of the matched lanes are
//      merged the same way: the first lane with a label left broadcasts it, four ballots count every matched
//      (lane, parity) that holds it, one add.  After kLabelRounds label rounds what is left goes on as adds of
//      1, after kTileRounds tile rounds the lanes that are left add for themselves: a 2 x 2 tile (every lane
//      a tile of its own) pays the rounds and then what it would have paid anyway.
//   2. In the work-group, an add goes to a direct-mapped table of kCacheSlots (cell, 32-bit count) pairs in
//      LDS, openset_head.hip's (map_common.h's cached_add and flush_cache): the slot is claimed by a
//      compare-and-swap on its cell index; a slot that another cell holds sends the add to global memory
//      instead.  The table is flushed to the global table by 64-bit atomics (relaxed, agent scope) after the
//      work-group's loop and every kFlushEvery trips.
// A slot cannot wrap: between two flushes a work-group sees kFlushEvery * 1024 output pixels, and the largest
// field, the sum of q, grows by at most 65,535 per pixel: 31 * 1024 * 65,535 < 2^32 (static_assert below).
// Integer sums: the result does not depend on the order of arrival, nor on the grid.
//
// acquire_apply.  audit_apply's layout: a lane owns 8 consecutive pixels of the flat maps (8-byte loads and
// stores; the last item of an odd-sized map goes byte by byte).  Row ends and tile borders fall inside an item:
// the lane divides once, for its first pixel, and then steps (x, y, n) and the tile coordinates along; the
// `selected` byte is read again only where the tile changes.  The counters live in LDS as 32-bit integers,
// runs of equal keys inside a lane's 8 pixels are one LDS atomic, and a work-group flushes its non-zero
// counters every kApplyFlushEvery trips and at its end by 64-bit global atomics.
#include "../../include/mdil_acquire.h"
#include "map_common.h"

#include <float.h>

namespace {

constexpr int kMaxC = MDIL_ACQUIRE_MAX_CLASSES;
constexpr int kFields = MDIL_ACQUIRE_TILE_FIELDS;
constexpr int kHeadWG = 256;                         // 4 wavefronts of 64 lanes
constexpr int kHeadMaxBlocks = 768;                  // three per CU; beyond 196,608 feature pixels the loop strides
constexpr int kCacheSlots = 4096;                    // LDS table of (cell, count): 32 KB
constexpr int kTileRounds = 8;                       // ballot rounds over tiles per feature pixel
constexpr int kLabelRounds = 4;                      // ballot rounds over labels per tile round
constexpr int kFlushEvery = 31;                      // trips between two flushes of the LDS table
constexpr int kMapWG = 256;
constexpr int kMapMaxBlocks = 512;                   // beyond 131,072 items (of 8 pixels) the loop strides
constexpr char kFnHead[] = "acquire_head";
constexpr char kFnApply[] = "acquire_apply";

static_assert((long long)kFlushEvery * kHeadWG * 4 * 65535 < (1LL << 32), "a 32-bit LDS slot could wrap");

// q = min(65535, (uint32)(max(u, 0) * 65536)): the scaling is exact, the cast truncates.  The comparisons keep a
// NaN and the negatives out of the cast (a NaN is not >= anything: it is sent to 0).
__device__ __forceinline__ uint32_t quantise(float u) {
  const float v = u * 65536.0f;
  return v >= 65535.0f ? 65535u : (v >= 0.0f ? (uint32_t)v : 0u);
}

// What one lane holds after its four parities.  packed: pixels | wrong << 10 | valid << 20 (each at most 4, a
// wave's sum at most 256); qs: the sum of its q; labels: byte a*2+b; left: bit a*2+b set where that pixel counts.
struct Lane {
  uint32_t cell0, packed, qs, labels, left;
};

__device__ __forceinline__ uint32_t label_of(uint32_t labels, int j) { return (labels >> (8 * j)) & 0xffu; }

// The adds of one feature pixel per lane: every lane of the wave calls it (the caller's loop is wave-uniform).
__device__ __forceinline__ void wave_merged_adds(u64* __restrict__ tiles, uint32_t* tags, uint32_t* counts, Lane L,
                                                 bool with_target) {
  const int lane = threadIdx.x & 63;
  bool active = L.left != 0u;
  u64 todo = __ballot(active);
  for (int round = 0; round < kTileRounds && todo; ++round) {
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
    const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)L.cell0, leader);
    const bool match = active && L.cell0 == c0;
    const u64 same = __ballot(match);
    const uint32_t pk = wave_sum_u32(match ? L.packed : 0u);
    const uint32_t qs = wave_sum_u32(match ? L.qs : 0u);
    if (lane == leader) {
      cached_add<kCacheSlots>(tiles, tags, counts, c0, pk & 1023u);
      if (qs) cached_add<kCacheSlots>(tiles, tags, counts, c0 + 1u, qs);
      if (with_target) {
        if ((pk >> 10) & 1023u) cached_add<kCacheSlots>(tiles, tags, counts, c0 + 2u, (pk >> 10) & 1023u);
        if (pk >> 20) cached_add<kCacheSlots>(tiles, tags, counts, c0 + 3u, pk >> 20);
      }
    }
    // the labels of the matched lanes
    uint32_t left = match ? L.left : 0u;
    u64 open = __ballot(left != 0u);
    for (int lr = 0; lr < kLabelRounds && open; ++lr) {
      const int first = __builtin_amdgcn_readfirstlane(__ffsll((long long)open) - 1);
      const uint32_t mine = left ? label_of(L.labels, __ffs((int)left) - 1) : 0u;
      const uint32_t l0 = (uint32_t)__builtin_amdgcn_readlane((int)mine, first);
      uint32_t n = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool hit = (left >> j & 1u) && label_of(L.labels, j) == l0;
        n += (uint32_t)__popcll(__ballot(hit));
        left = hit ? left & ~(1u << j) : left;
      }
      if (lane == first) cached_add<kCacheSlots>(tiles, tags, counts, c0 + (uint32_t)kFields + l0, n);
      open = __ballot(left != 0u);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (left >> j & 1u)
        cached_add<kCacheSlots>(tiles, tags, counts, c0 + (uint32_t)kFields + label_of(L.labels, j), 1u);
    active = active && !match;
    todo &= ~same;
  }
  if (active) {                                                    // a lane of a tile no round reached
    cached_add<kCacheSlots>(tiles, tags, counts, L.cell0, L.packed & 1023u);
    if (L.qs) cached_add<kCacheSlots>(tiles, tags, counts, L.cell0 + 1u, L.qs);
    if (with_target) {
      if ((L.packed >> 10) & 1023u) cached_add<kCacheSlots>(tiles, tags, counts, L.cell0 + 2u, (L.packed >> 10) & 1023u);
      if (L.packed >> 20) cached_add<kCacheSlots>(tiles, tags, counts, L.cell0 + 3u, L.packed >> 20);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (L.left >> j & 1u)
        cached_add<kCacheSlots>(tiles, tags, counts, L.cell0 + (uint32_t)kFields + label_of(L.labels, j), 1u);
  }
}

// Occupancy: __launch_bounds__(256, 2) as openset_head and audit_head, the 32 logits of a parity and the 16
// features in registers, 41 KB of LDS: three work-groups per CU, three waves per SIMD (Acquire).
__global__ __launch_bounds__(kHeadWG, 2) void acquire_head_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, long long npix, int H, int W,
    int nc, int th, int tw, int Ty, int Tx, int kind, float inv_log_nc, const unsigned char* __restrict__ target,
    int ignore_index, unsigned char* __restrict__ label, unsigned short* __restrict__ qmap, u64* __restrict__ tiles,
    u64* __restrict__ nonfinite, u64* __restrict__ bad_targets) {
  __shared__ __attribute__((aligned(16))) float Wp[4][kMaxC][16];   // [a*2+b][c][ci]
  __shared__ float Bl[kMaxC];
  __shared__ uint32_t tags[kCacheSlots];
  __shared__ uint32_t counts[kCacheSlots];
  __shared__ uint32_t nf, bt;
  static_assert((MDIL_ACQUIRE_MAX_PIXELS / 4 + (long long)kHeadMaxBlocks * kHeadWG - 1) / ((long long)kHeadMaxBlocks * kHeadWG) *
                        kHeadWG * 4 < 0x80000000LL,
                "a lane's 32-bit counter could wrap");
  for (int i = threadIdx.x; i < nc * 64; i += kHeadWG) {
    const int k = i & 3, ci = (i >> 2) & 15, c = i >> 6;
    Wp[k][c][ci] = w[(ci * nc + c) * 4 + k];
  }
  for (int i = threadIdx.x; i < nc; i += kHeadWG) Bl[i] = bias[i];
  for (int i = threadIdx.x; i < kCacheSlots; i += kHeadWG) {
    tags[i] = kEmptySlot;
    counts[i] = 0u;
  }
  if (threadIdx.x == 0) nf = bt = 0u;
  __syncthreads();

  const long long HW = (long long)H * W;
  const uint32_t row = (uint32_t)(kFields + nc);                   // cells of one tile
  uint32_t bad = 0u, badt = 0u;
  int trips = 0;
  // the trip count is the same for every lane of the work-group
  for (long long base = (long long)blockIdx.x * kHeadWG; base < npix; base += (long long)gridDim.x * kHeadWG) {
    const bool valid = base + threadIdx.x < npix;
    const long long p = valid ? base + threadIdx.x : npix - 1;     // a lane past the end: a clamped pixel, no writes
    f32x4 xv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xv[k] = *reinterpret_cast<const f32x4*>(x + p * 16 + k * 4);
    const long long r = p / W;                                     // n * H + h
    const long long n = p / HW;
    const int h = (int)(r - n * H), col = (int)(p - r * W);
    const long long o0 = (2 * r * 2 * W) + 2 * col;                // pixel (2h, 2w); row below: + 2W
    uint32_t given = 0u;                                           // byte a*2+b
    if (target) given = quad_bytes(target, o0, W);
    Lane L;
    L.cell0 = (uint32_t)((n * Ty + (2 * h) / th) * Tx + (2 * col) / tw) * row;   // below 2^31 (checked by the host)
    L.packed = L.qs = L.labels = L.left = 0u;
    uint32_t q_top = 0u, q_bottom = 0u;                            // the two pixels of a row

#pragma unroll 1
    for (int par = 0; par < 4; ++par) {
      float d[kMaxC];
      // The logits of this parity: bias first, then ci ascending.  map_common.h's stage_parity and parity_logits,
      // spelled out here and above: through the helpers the compiler schedules this kernel differently (same
      // registers, same length) and the variants with tiles ran 1 to 1.5 % slower than before, past the
      // run-to-run margin (profiles/map_common_ab.json); spelled out, the kernel's code is what it was.
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) {
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
      float m = 0.f;
      int bi = 0;
#pragma unroll
      for (int c = 0; c < kMaxC; ++c)
        if (c < nc) vote(c, d[c], m, bi);
      float s = 0.f, A = 0.f, e2 = 0.f;
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) {
        if (c < nc) {
          float v = d[c] - m;
          v = v == -INFINITY ? -FLT_MAX : v;                       // 0 * d_c stays 0; a NaN stays a NaN
          const float e = __builtin_amdgcn_exp2f(__fmul_rn(v, kLog2e));
          s += e;
          A = __builtin_fmaf(e, v, A);
          e2 = c != bi ? fmaxf(e2, e) : e2;
        }
      }
      const float conf = 1.0f / s;
      float u;
      if (kind == MDIL_ACQUIRE_ENTROPY) {                          // uniform over the grid
        const float ent = __fsub_rn(logf(s), __fmul_rn(A, conf));
        u = __fmul_rn(ent, inv_log_nc);
      } else if (kind == MDIL_ACQUIRE_MARGIN) {
        u = __fsub_rn(1.0f, __fmul_rn(conf, __fsub_rn(1.0f, e2)));
      } else {
        u = __fmul_rn(__fsub_rn(s, 1.0f), conf);
      }
      const bool finite = is_finite(s) && is_finite(m);
      const uint32_t q = finite ? quantise(u) : 0u;

      const uint32_t tb = (given >> (8 * par)) & 0xffu;
      const bool labelled = target && (int)tb != ignore_index;
      const bool usable = labelled && tb < (uint32_t)nc;           // a VALID pixel
      badt += valid && labelled && !usable ? 1u : 0u;
      bad += valid && !finite ? 1u : 0u;

      L.labels |= (uint32_t)bi << (8 * par);
      if (par < 2)
        q_top |= q << (16 * (par & 1));
      else
        q_bottom |= q << (16 * (par & 1));
      if (valid && finite) {
        L.left |= 1u << par;
        L.packed += 1u + (usable && tb != (uint32_t)bi ? 1u << 10 : 0u) + (usable ? 1u << 20 : 0u);
        L.qs += q;
      }
    }

    if (valid && label) {
      *reinterpret_cast<uint16_t*>(label + o0) = (uint16_t)(L.labels & 0xffffu);
      *reinterpret_cast<uint16_t*>(label + o0 + 2LL * W) = (uint16_t)(L.labels >> 16);
    }
    if (valid && qmap) {
      *reinterpret_cast<uint32_t*>(qmap + o0) = q_top;
      *reinterpret_cast<uint32_t*>(qmap + o0 + 2LL * W) = q_bottom;
    }
    if (tiles) {
      wave_merged_adds(tiles, tags, counts, L, target != nullptr);
      if (++trips == kFlushEvery) {                                // uniform over the work-group
        trips = 0;
        __syncthreads();
        flush_cache<kHeadWG, kCacheSlots>(tiles, tags, counts);
        __syncthreads();
      }
    }
  }

  if (bad) atomicAdd(&nf, bad);
  if (badt) atomicAdd(&bt, badt);
  __syncthreads();                                                 // every lane of the work-group is here
  if (threadIdx.x == 0) {
    if (nonfinite && nf) __hip_atomic_fetch_add(nonfinite, (u64)nf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (bad_targets && bt) __hip_atomic_fetch_add(bad_targets, (u64)bt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tiles) flush_cache<kHeadWG, kCacheSlots>(tiles, tags, counts);
}

__global__ __launch_bounds__(kMapWG) void acquire_apply_kernel(
    const unsigned char* __restrict__ selected, const unsigned char* __restrict__ target,
    const unsigned char* __restrict__ previous, const unsigned char* __restrict__ fill, long long npix, long long nitems,
    int Hl, int Wl, int th, int tw, int Ty, int Tx, int nc, int ignore_index, int drop_id, unsigned char* __restrict__ out,
    unsigned char* __restrict__ mask, u64* __restrict__ shown, u64* __restrict__ annotated, u64* __restrict__ kept,
    u64* __restrict__ filled, u64* __restrict__ bad_targets) {
  __shared__ uint32_t Al[kMaxC], Kl[kMaxC], Fl[kMaxC];               // annotated, kept, filled
  __shared__ uint32_t misc[2];                                       // shown, bad targets
  zero_annotator<kMapWG>(Al, Kl, Fl, nc, misc);

  const long long HWl = (long long)Hl * Wl;
  int trips = 0;
  for (long long base = (long long)blockIdx.x * kMapWG; base < nitems; base += (long long)gridDim.x * kMapWG) {
    const long long item = base + threadIdx.x;
    if (item < nitems) {
      const long long o = item * kPerItem;
      const int n = o + kPerItem <= npix ? kPerItem : (int)(npix - o);
      uint32_t tg[kPerItem], pv[kPerItem], fl[kPerItem];
      if (target) load_bytes(target, o, n, tg);
      if (previous) load_bytes(previous, o, n, pv);
      if (fill) load_bytes(fill, o, n, fl);

      // the first pixel's place, by division; the others step along
      long long img = o / HWl;
      const long long rem = o - img * HWl;
      int y = (int)(rem / Wl), xx = (int)(rem - (long long)y * Wl);
      int ty = y / th, yin = y - ty * th, tx = xx / tw, xin = xx - tx * tw;
      bool sel = selected[(img * Ty + ty) * Tx + tx] != 0;

      uint32_t ob[kPerItem], mb[kPerItem], nshown = 0u, nbad = 0u;
      Run ann_run(Al), kept_run(Kl), fill_run(Fl);
#pragma unroll
      for (int j = 0; j < kPerItem; ++j) {
        ob[j] = (uint32_t)drop_id;
        mb[j] = 0u;
        if (j < n) {
          annotate_pixel(sel, target, tg[j], previous, pv[j], fill, fl[j], nc, ignore_index, drop_id, ann_run, kept_run,
                         fill_run, ob[j], mb[j], nshown, nbad);
          // the next pixel of the flat map
          if (j + 1 < n) {
            bool moved = false;
            ++xx;
            if (++xin == tw) {
              xin = 0;
              ++tx;
              moved = true;
            }
            if (xx == Wl) {
              xx = tx = xin = 0;
              moved = true;
              ++y;
              if (++yin == th) {
                yin = 0;
                ++ty;
              }
              if (y == Hl) {
                y = ty = yin = 0;
                ++img;
              }
            }
            if (moved) sel = selected[(img * Ty + ty) * Tx + tx] != 0;
          }
        }
      }
      ann_run.done();
      kept_run.done();
      fill_run.done();
      if (nshown) atomicAdd(&misc[0], nshown);
      if (nbad) atomicAdd(&misc[1], nbad);
      if (out) store_bytes(out, o, n, ob);
      if (mask) store_bytes(mask, o, n, mb);
    }

    const bool last = base + (long long)gridDim.x * kMapWG >= nitems;
    if (last || ++trips == kApplyFlushEvery) {                     // uniform over the work-group
      trips = 0;
      u64* const dst[2] = {shown, bad_targets};
      flush_annotator<kMapWG>(Al, Kl, Fl, nc, annotated, kept, filled, misc, dst);
    }
  }
}

inline bool tile_ok(const char* fn, int th, int tw) {
  if (th >= MDIL_ACQUIRE_MIN_TILE && th <= MDIL_ACQUIRE_MAX_TILE && tw >= MDIL_ACQUIRE_MIN_TILE &&
      tw <= MDIL_ACQUIRE_MAX_TILE && !(th & 1) && !(tw & 1))
    return true;
  set_error("%s: tile %d x %d (each side even and in [%d, %d])", fn, th, tw, MDIL_ACQUIRE_MIN_TILE, MDIL_ACQUIRE_MAX_TILE);
  return false;
}

}  // namespace

API int mdil_acquire_version(void) { return 100; }
API const char* mdil_acquire_last_error(void) { return g_err; }

API int mdil_acquire_head(const float* x, const float* w, const float* bias, int N, int H, int W, int nc, int th, int tw,
                          int kind, float inv_log_nc, const unsigned char* target, int ignore_index,
                          unsigned char* label, unsigned short* qmap, long long* tiles, long long* nonfinite,
                          long long* bad_targets, void* stream) {
  if (!x || !w || !bias || N <= 0 || H <= 0 || W <= 0) {
    set_error("acquire_head: bad argument (x %p w %p bias %p N %d H %d W %d)", (const void*)x, (const void*)w,
              (const void*)bias, N, H, W);
    return MDIL_ACQUIRE_ERR_INVALID;
  }
  if (!label && !qmap && !tiles && !nonfinite && !bad_targets) {
    set_error("acquire_head: nothing to write (label, qmap, tiles, nonfinite and bad_targets are all NULL)");
    return MDIL_ACQUIRE_ERR_INVALID;
  }
  if (!classes_ok(kFnHead, nc, MDIL_ACQUIRE_MIN_CLASSES, MDIL_ACQUIRE_MAX_CLASSES)) return MDIL_ACQUIRE_ERR_INVALID;
  if (!tile_ok(kFnHead, th, tw)) return MDIL_ACQUIRE_ERR_INVALID;
  if (kind < 0 || kind >= MDIL_ACQUIRE_KINDS) {
    set_error("acquire_head: kind=%d (0 msp, 1 entropy, 2 margin)", kind);
    return MDIL_ACQUIRE_ERR_INVALID;
  }
  if (kind == MDIL_ACQUIRE_ENTROPY && !(inv_log_nc >= 0.0f && inv_log_nc < INFINITY)) {
    set_error("acquire_head: inv_log_nc=%g (finite and >= 0; meant to be 1 / ln nc)", (double)inv_log_nc);
    return MDIL_ACQUIRE_ERR_INVALID;
  }
  if (!ignore_ok(kFnHead, ignore_index)) return MDIL_ACQUIRE_ERR_INVALID;
  if (!target && bad_targets) {
    set_error("acquire_head: bad_targets needs a target");
    return MDIL_ACQUIRE_ERR_INVALID;
  }
  if (((uintptr_t)x & 15) || ((uintptr_t)w & 3) || ((uintptr_t)bias & 3) || ((uintptr_t)target & 1) ||
      ((uintptr_t)label & 1) || ((uintptr_t)qmap & 3) || ((uintptr_t)tiles & 7) || ((uintptr_t)nonfinite & 7) ||
      ((uintptr_t)bad_targets & 7)) {
    set_error("acquire_head: alignment (x 16 B; w and bias 4 B; target and label 2 B; qmap 4 B; the counters 8 B)");
    return MDIL_ACQUIRE_ERR_INVALID;
  }
  if (!shape_ok(N, H, W, MDIL_ACQUIRE_MAX_PIXELS / 4)) {
    set_error("acquire_head: too large (N %d, features %d x %d: at most 2^40 output pixels)", N, H, W);
    return MDIL_ACQUIRE_ERR_INVALID;
  }
  const int Ty = (2 * H + th - 1) / th, Tx = (int)((2LL * W + tw - 1) / tw);
  if (tiles && (long long)N * Ty * Tx > MDIL_ACQUIRE_MAX_CELLS / (MDIL_ACQUIRE_TILE_FIELDS + nc)) {
    set_error("acquire_head: too large (N %d, %d x %d tiles of %d cells: at most 2^31 cells in a tile table)", N, Ty, Tx,
              MDIL_ACQUIRE_TILE_FIELDS + nc);
    return MDIL_ACQUIRE_ERR_INVALID;
  }
  const long long npix = (long long)N * H * W;
  const int grid = bounded_grid(npix, kHeadWG, kHeadMaxBlocks);
  hipLaunchKernelGGL(acquire_head_kernel, dim3(grid), dim3(kHeadWG), 0, (hipStream_t)stream, x, w, bias, npix, H, W, nc, th,
                     tw, Ty, Tx, kind, inv_log_nc, target, ignore_index, label, qmap, reinterpret_cast<u64*>(tiles),
                     reinterpret_cast<u64*>(nonfinite), reinterpret_cast<u64*>(bad_targets));
  return launched(kFnHead) ? MDIL_ACQUIRE_OK : MDIL_ACQUIRE_ERR_LAUNCH;
}

API int mdil_acquire_apply(const unsigned char* selected, const unsigned char* target, const unsigned char* previous,
                           const unsigned char* fill, int N, int Hl, int Wl, int th, int tw, int nc, int ignore_index,
                           int drop_id, unsigned char* out, unsigned char* mask, long long* shown, long long* annotated,
                           long long* kept, long long* filled, long long* bad_targets, void* stream) {
  if (!selected || N <= 0 || Hl <= 0 || Wl <= 0) {
    set_error("acquire_apply: bad argument (selected %p N %d Hl %d Wl %d)", (const void*)selected, N, Hl, Wl);
    return MDIL_ACQUIRE_ERR_INVALID;
  }
  if ((long long)N * Hl > MDIL_ACQUIRE_MAX_PIXELS / Wl) {
    set_error("acquire_apply: too large (N %d, maps %d x %d: at most 2^40 pixels)", N, Hl, Wl);
    return MDIL_ACQUIRE_ERR_INVALID;
  }
  if (!classes_ok(kFnApply, nc, MDIL_ACQUIRE_MIN_CLASSES, MDIL_ACQUIRE_MAX_CLASSES)) return MDIL_ACQUIRE_ERR_INVALID;
  if (!tile_ok(kFnApply, th, tw)) return MDIL_ACQUIRE_ERR_INVALID;
  if (!ignore_ok(kFnApply, ignore_index)) return MDIL_ACQUIRE_ERR_INVALID;
  if (!byte_id_ok(kFnApply, "drop_id", drop_id)) return MDIL_ACQUIRE_ERR_INVALID;
  if (!apply_outputs_ok(kFnApply, {out, mask, shown, annotated, kept, filled, bad_targets})) return MDIL_ACQUIRE_ERR_INVALID;
  if (!apply_target_ok(kFnApply, target, annotated, bad_targets)) return MDIL_ACQUIRE_ERR_INVALID;
  if (!aligned8_ok(kFnApply, "target, previous, fill, out, mask and the counters",
                   {target, previous, fill, out, mask, shown, annotated, kept, filled, bad_targets}))
    return MDIL_ACQUIRE_ERR_INVALID;
  const long long npix = (long long)N * Hl * Wl;
  const long long nitems = (npix + kPerItem - 1) / kPerItem;
  const int Ty = (Hl + th - 1) / th, Tx = (Wl + tw - 1) / tw;
  const int grid = bounded_grid(nitems, kMapWG, kMapMaxBlocks);
  hipLaunchKernelGGL(acquire_apply_kernel, dim3(grid), dim3(kMapWG), 0, (hipStream_t)stream, selected, target, previous,
                     fill, npix, nitems, Hl, Wl, th, tw, Ty, Tx, nc, ignore_index, drop_id, out, mask,
                     reinterpret_cast<u64*>(shown), reinterpret_cast<u64*>(annotated), reinterpret_cast<u64*>(kept),
                     reinterpret_cast<u64*>(filled), reinterpret_cast<u64*>(bad_targets));
  return launched(kFnApply) ? MDIL_ACQUIRE_OK : MDIL_ACQUIRE_ERR_LAUNCH;
}
