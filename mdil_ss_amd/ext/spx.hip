// libmdil_spx.so: an integer SLIC, the per-superpixel table and the one-click annotator (gfx950).  Integers only
// after the colour quantisation; include/mdil_spx.h spells the rule out.
//
//   spx_codes    image -> r | g << 8 | b << 16 per pixel, kept in the `id` map while the call runs: an assign reads 4
//                bytes per pixel instead of 12
//   spx_init     the first centres; zeroes `sums`
//   spx_assign   the assign fused with the accumulation of the next update's sums
//   spx_update   sums -> centres; zeroes `sums`
//   spx_table    per superpixel [pixels, sum q, wrong, valid, label counts] and the valid-target counts
//   spx_apply    ripu_apply's rule with the region read through the id map and one answer per region
//
// spx_assign.  A work-group of 256 lanes owns a job: a block of kBlockCells(S) x kBlockCells(S) WHOLE cells of one
// image, at most kBlockPx x kBlockPx pixels (16 x 16 cells at S = 4, 4 x 4 at 16, one at S > 32).  It stages the
// centres of those cells plus one ring of cells in LDS (at most 18 x 18 x 5 ints, 6.3 KB; a cell outside the grid is
// marked), so every candidate of every pixel of the block is there.  A wave walks rows of the block, the column on the
// lane: one coalesced load of the codes, nine distances from LDS in ascending k with a strict <, so a tie keeps the
// lowest k.  The six sums of the staged centres live in LDS as 32-bit counts (a job adds at most 4096 pixels with
// coordinates below 4096: every sum stays below 2^24).  Before the LDS atomics the wave merges: lanes of one run of
// equal centres (a row crosses few superpixels) are summed by a segmented shuffle scan over three packed words
// (r | g << 16, b | n << 16, x; sum y is n * y), and the last lane of the run adds.  After the rows the non-zero entries go to
// `sums` with 64-bit atomics, which commute: the bytes do not depend on the grid.  LDS: 6.3 + 7.6 KB.  A larger image
// takes more rounds of the loop over jobs, not a larger grid (bounded_grid).
//
// spx_table.  A lane owns 8 consecutive pixels and merges them into runs of one superpixel; the adds go through
// map_common.h's cached_add, a direct-mapped LDS table of (cell, count): where ids are local (SLIC's) nearly every add
// meets in LDS, and for any other id map a collision falls through to a global atomic, so the result is the same.
//
// spx_apply.  ripu_apply's layout: a lane owns 8 consecutive pixels; `selected` and `answer` are looked up per run of
// equal ids; the counters live in LDS as 32-bit integers and are flushed by 64-bit atomics.
#include "../../include/mdil_spx.h"
#include "map_common.h"

namespace {

constexpr int kMaxC = MDIL_SPX_MAX_CLASSES;
constexpr int kFields = MDIL_SPX_FIELDS;
constexpr int kBlockPx = 64;                          // a job of spx_assign is at most 64 x 64 pixels
constexpr int kMinStep = MDIL_SPX_MIN_STEP;
constexpr int kMaxRing = kBlockPx / kMinStep + 2;     // 18 cells a side with the ring
constexpr int kMaxLocal = kMaxRing * kMaxRing;
constexpr int kAssignWG = 256;
constexpr int kAssignWaves = kAssignWG / 64;
constexpr int kAssignMaxBlocks = 1024;                // beyond that the loop over jobs strides
constexpr int kFlatWG = 256;
constexpr int kFlatMaxBlocks = 1024;
constexpr int kMapWG = 256;
constexpr int kMapMaxBlocks = 512;                    // beyond 131,072 items (of 8 pixels) the loop strides
constexpr int kTableSlots = 2048;                     // of each of the two LDS tables of adds
constexpr int kTableFlushEvery = 16;                  // trips: a trip adds at most 2048 x 65,535 to a sum of q
constexpr int kNoCentre = INT32_MIN;                  // Y of a staged cell outside the grid
constexpr char kFnSlic[] = "spx_slic";
constexpr char kFnTable[] = "spx_table";
constexpr char kFnApply[] = "spx_apply";

static_assert(kBlockPx == 64, "a row of a block is one wave");
static_assert((long long)kTableFlushEvery * kMapWG * kPerItem * 65535 < (1LL << 32), "a 32-bit sum of q could wrap");
static_assert((long long)kBlockPx * kBlockPx * (MDIL_SPX_MAX_SIDE - 1) < (1LL << 32), "a job's 32-bit sum of y could wrap");
static_assert(64 * 255 < 65536 && 64 * MDIL_SPX_MAX_SIDE < (1 << 30), "the packed words of the wave merge could carry");

__host__ __device__ __forceinline__ int block_cells(int S) { return kBlockPx / S > 1 ? kBlockPx / S : 1; }

// The colour code of the header: NaN -> 0, clamp, one fused multiply-add, truncation.
__device__ __forceinline__ uint32_t code8(float v) {
  v = v == v ? v : 0.0f;
  v = fminf(fmaxf(v, 0.0f), 1.0f);
  return (uint32_t)__builtin_fmaf(v, 255.0f, 0.5f);
}

__global__ __launch_bounds__(kFlatWG) void spx_codes_kernel(const float* __restrict__ image, long long npix, long long HW,
                                                            int* __restrict__ id) {
  for (long long p = (long long)blockIdx.x * kFlatWG + threadIdx.x; p < npix; p += (long long)gridDim.x * kFlatWG) {
    const long long n = p / HW;
    const float* px = image + n * 3 * HW + (p - n * HW);
    id[p] = (int)(code8(px[0]) | code8(px[HW]) << 8 | code8(px[2 * HW]) << 16);
  }
}

__global__ __launch_bounds__(kFlatWG) void spx_init_kernel(const int* __restrict__ id, long long cells, int H, int W, int S,
                                                           int Gx, int K, int* __restrict__ centres,
                                                           long long* __restrict__ sums) {
  for (long long i = (long long)blockIdx.x * kFlatWG + threadIdx.x; i < cells; i += (long long)gridDim.x * kFlatWG) {
    const long long n = i / K;
    const int k = (int)(i - n * K), gy = k / Gx, gx = k - gy * Gx;
    const int y = min(H - 1, gy * S + S / 2), x = min(W - 1, gx * S + S / 2);
    const uint32_t c = (uint32_t)id[(n * H + y) * W + x];
    int* o = centres + i * 5;
    o[0] = 16 * y;
    o[1] = 16 * x;
    o[2] = 16 * (int)(c & 255u);
    o[3] = 16 * (int)(c >> 8 & 255u);
    o[4] = 16 * (int)(c >> 16 & 255u);
#pragma unroll
    for (int j = 0; j < 6; ++j) sums[i * 6 + j] = 0;
  }
}

__global__ __launch_bounds__(kFlatWG) void spx_update_kernel(long long cells, int* __restrict__ centres,
                                                             long long* __restrict__ sums) {
  for (long long i = (long long)blockIdx.x * kFlatWG + threadIdx.x; i < cells; i += (long long)gridDim.x * kFlatWG) {
    const long long n = sums[i * 6];
    if (n > 0) {
#pragma unroll
      for (int j = 0; j < 5; ++j) centres[i * 5 + j] = (int)((16 * sums[i * 6 + 1 + j] + n / 2) / n);
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) sums[i * 6 + j] = 0;
  }
}

__global__ __launch_bounds__(kAssignWG) void spx_assign_kernel(int* __restrict__ id, const int* __restrict__ centres,
                                                               u64* __restrict__ sums, long long jobs, int By, int Bx,
                                                               int BC, int H, int W, int S, int Gy, int Gx, u64 S2, u64 m2,
                                                               int write_id) {
  __shared__ int C[kMaxLocal][5];
  __shared__ uint32_t A[kMaxLocal][6];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int LW = BC + 2, local = LW * LW, K = Gy * Gx;
  const int hx = lane / S;                                           // the home cell's column within the block

  for (long long job = blockIdx.x; job < jobs; job += gridDim.x) {   // uniform over the work-group
    const long long n = job / ((long long)By * Bx);
    const int rem = (int)(job - n * By * Bx);
    const int jy = rem / Bx, jx = rem - jy * Bx;
    const int cy0 = jy * BC - 1, cx0 = jx * BC - 1;                  // the ring's first cell
    for (int i = tid; i < local; i += kAssignWG) {
      const int ly = i / LW, gy = cy0 + ly, gx = cx0 + i - ly * LW;
      if (gy >= 0 && gy < Gy && gx >= 0 && gx < Gx) {
        const int* c = centres + (n * K + (long long)gy * Gx + gx) * 5;
#pragma unroll
        for (int j = 0; j < 5; ++j) C[i][j] = c[j];
      } else {
        C[i][0] = kNoCentre;
      }
#pragma unroll
      for (int j = 0; j < 6; ++j) A[i][j] = 0u;
    }
    __syncthreads();

    const int py0 = jy * BC * S, px0 = jx * BC * S;
    const int ph = min(H, py0 + BC * S) - py0, pw = min(W, px0 + BC * S) - px0;
    const int x = px0 + lane;
    const bool incol = lane < pw;
    for (int row = wave; row < ph; row += kAssignWaves) {            // uniform over the wave
      const int y = py0 + row, hy = row / S;
      int lk = -1;
      uint32_t code = 0u;
      if (incol) {
        const long long o = (n * H + y) * W + x;
        code = (uint32_t)id[o];
        const int r16 = 16 * (int)(code & 255u), g16 = 16 * (int)(code >> 8 & 255u), b16 = 16 * (int)(code >> 16 & 255u);
        u64 best = ~0ull;
        for (int dy = 0; dy < 3; ++dy) {
          for (int dx = 0; dx < 3; ++dx) {                           // ascending k: a tie keeps the lowest
            const int i = (hy + dy) * LW + hx + dx;
            const int Y = C[i][0];
            if (Y == kNoCentre) continue;
            const int ey = 16 * y - Y, ex = 16 * x - C[i][1];
            const int er = r16 - C[i][2], eg = g16 - C[i][3], eb = b16 - C[i][4];
            const u64 D = S2 * (u64)(uint32_t)(er * er + eg * eg + eb * eb) + m2 * (u64)(uint32_t)(ey * ey + ex * ex);
            if (D < best) {
              best = D;
              lk = i;
            }
          }
        }
        if (write_id) {
          const int ly = lk / LW;
          id[o] = (cy0 + ly) * Gx + cx0 + lk - ly * LW;
        }
      }
      // the wave's merge: runs of equal lk along the row, a segmented inclusive scan, the run's last lane adds
      const int prev = __shfl_up(lk, 1, 64);
      const u64 heads = __ballot(lane == 0 || prev != lk);
      const int head = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane)));
      uint32_t v0 = incol ? (code & 255u) | (code >> 8 & 255u) << 16 : 0u;   // r | g << 16
      uint32_t v1 = incol ? (code >> 16 & 255u) | 1u << 16 : 0u;             // b | n << 16
      uint32_t v2 = incol ? (uint32_t)x : 0u;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t0 = (uint32_t)__shfl_up((int)v0, d, 64), t1 = (uint32_t)__shfl_up((int)v1, d, 64),
                       t2 = (uint32_t)__shfl_up((int)v2, d, 64);
        if (lane - d >= head) {
          v0 += t0;
          v1 += t1;
          v2 += t2;
        }
      }
      const bool last = lane == 63 || (heads >> (lane + 1) & 1ull);
      if (last && lk >= 0) {
        const uint32_t cnt = v1 >> 16;
        atomicAdd(&A[lk][0], cnt);
        atomicAdd(&A[lk][1], cnt * (uint32_t)y);
        atomicAdd(&A[lk][2], v2);
        atomicAdd(&A[lk][3], v0 & 0xffffu);
        atomicAdd(&A[lk][4], v0 >> 16);
        atomicAdd(&A[lk][5], v1 & 0xffffu);
      }
    }
    __syncthreads();

    for (int i = tid; i < local; i += kAssignWG) {
      if (A[i][0]) {                                                 // a centre with pixels lies inside the grid
        const int ly = i / LW;
        u64* s = sums + (n * K + (long long)(cy0 + ly) * Gx + cx0 + i - ly * LW) * 6;
#pragma unroll
        for (int j = 0; j < 6; ++j)
          if (A[i][j]) __hip_atomic_fetch_add(s + j, (u64)A[i][j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    __syncthreads();                                                 // before the next job stages
  }
}

// A run of equal slots of one of the two LDS tables: `add` extends it or sends it on.
template <int SLOTS>
struct SlotRun {
  u64* table;
  uint32_t *tags, *counts, slot, n;
  __device__ __forceinline__ SlotRun(u64* t, uint32_t* tg, uint32_t* ct) : table(t), tags(tg), counts(ct), slot(kEmptySlot), n(0u) {}
  __device__ __forceinline__ void done() {
    if (n) cached_add<SLOTS>(table, tags, counts, slot, n);
    n = 0u;
  }
  __device__ __forceinline__ void add(uint32_t s, uint32_t v) {
    if (s != slot) {
      done();
      slot = s;
    }
    n += v;
  }
};

__global__ __launch_bounds__(kMapWG) void spx_table_kernel(
    const unsigned char* __restrict__ label, const unsigned short* __restrict__ qmap,
    const unsigned char* __restrict__ target, int ignore_index, const int* __restrict__ id, long long npix, long long nitems,
    long long HW, int K, int nc, u64* __restrict__ table, u64* __restrict__ tcount, u64* __restrict__ bad_targets,
    u64* __restrict__ bad_ids) {
  __shared__ uint32_t tagT[kTableSlots], cntT[kTableSlots], tagC[kTableSlots], cntC[kTableSlots];
  __shared__ uint32_t misc[2];                                       // bad targets, bad ids
  for (int i = threadIdx.x; i < kTableSlots; i += kMapWG) {
    tagT[i] = tagC[i] = kEmptySlot;
    cntT[i] = cntC[i] = 0u;
  }
  if (threadIdx.x < 2) misc[threadIdx.x] = 0u;
  __syncthreads();

  const uint32_t F = (uint32_t)(kFields + nc);
  int trips = 0;
  for (long long base = (long long)blockIdx.x * kMapWG; base < nitems; base += (long long)gridDim.x * kMapWG) {
    const long long item = base + threadIdx.x;
    if (item < nitems) {
      const long long o = item * kPerItem;
      const int cnt = o + kPerItem <= npix ? kPerItem : (int)(npix - o);
      long long n = o / HW, rem = o - n * HW;
      uint32_t lb[kPerItem], tg[kPerItem];
      load_bytes(label, o, cnt, lb);
      if (target) load_bytes(target, o, cnt, tg);
      SlotRun<kTableSlots> px(table, tagT, cntT), sq(table, tagT, cntT), wr(table, tagT, cntT), vd(table, tagT, cntT),
          lc(table, tagT, cntT), tc(tcount, tagC, cntC);
      uint32_t nbadt = 0u, nbadid = 0u;
#pragma unroll
      for (int j = 0; j < kPerItem; ++j) {
        if (j < cnt) {
          const int k = id[o + j];
          if ((uint32_t)k >= (uint32_t)K) {
            ++nbadid;
          } else {
            const uint32_t cell = (uint32_t)(n * K + k);
            if (table) {
              px.add(cell * F, 1u);
              sq.add(cell * F + 1u, (uint32_t)qmap[o + j]);
              if (lb[j] < (uint32_t)nc) lc.add(cell * F + kFields + lb[j], 1u);
            }
            if (target && (int)tg[j] != ignore_index) {
              if (tg[j] < (uint32_t)nc) {
                if (table) {
                  vd.add(cell * F + 3u, 1u);
                  if (lb[j] != tg[j]) wr.add(cell * F + 2u, 1u);
                }
                if (tcount) tc.add(cell * (uint32_t)nc + tg[j], 1u);
              } else {
                ++nbadt;
              }
            }
          }
          if (++rem == HW) {
            rem = 0;
            ++n;
          }
        }
      }
      px.done();
      sq.done();
      wr.done();
      vd.done();
      lc.done();
      tc.done();
      if (nbadt) atomicAdd(&misc[0], nbadt);
      if (nbadid) atomicAdd(&misc[1], nbadid);
    }

    const bool last = base + (long long)gridDim.x * kMapWG >= nitems;
    if (last || ++trips == kTableFlushEvery) {                       // uniform over the work-group
      trips = 0;
      __syncthreads();
      if (table) flush_cache<kMapWG, kTableSlots>(table, tagT, cntT);
      if (tcount) flush_cache<kMapWG, kTableSlots>(tcount, tagC, cntC);
      if (threadIdx.x < 2) {
        u64* const dst = threadIdx.x ? bad_ids : bad_targets;
        const uint32_t v = misc[threadIdx.x];
        if (v && dst) __hip_atomic_fetch_add(dst, (u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        misc[threadIdx.x] = 0u;
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(kMapWG) void spx_apply_kernel(
    const int* __restrict__ id, const unsigned char* __restrict__ selected, const unsigned char* __restrict__ answer,
    const unsigned char* __restrict__ target, const unsigned char* __restrict__ previous,
    const unsigned char* __restrict__ fill, const unsigned char* __restrict__ label, long long npix, long long nitems,
    long long HW, int K, int nc, int ignore_index, int drop_id, unsigned char* __restrict__ out,
    unsigned char* __restrict__ mask, u64* __restrict__ shown, u64* __restrict__ annotated, u64* __restrict__ kept,
    u64* __restrict__ filled, u64* __restrict__ bad_targets, u64* __restrict__ wrong_shown, u64* __restrict__ wrong_all,
    u64* __restrict__ noisy, u64* __restrict__ bad_ids) {
  __shared__ uint32_t Al[kMaxC], Kl[kMaxC], Fl[kMaxC];               // annotated, kept, filled
  __shared__ uint32_t misc[6];                                       // shown, bad targets, wrong shown, wrong all, noisy, bad ids
  zero_annotator<kMapWG>(Al, Kl, Fl, nc, misc);

  const bool judge = target && label;
  const unsigned char* const given = answer ? answer : target;       // what a chosen pixel receives, where there is one
  int trips = 0;
  for (long long base = (long long)blockIdx.x * kMapWG; base < nitems; base += (long long)gridDim.x * kMapWG) {
    const long long item = base + threadIdx.x;
    if (item < nitems) {
      const long long o = item * kPerItem;
      const int cnt = o + kPerItem <= npix ? kPerItem : (int)(npix - o);
      long long n = o / HW, rem = o - n * HW;
      uint32_t tg[kPerItem], pv[kPerItem], fl[kPerItem], lb[kPerItem];
      if (target) load_bytes(target, o, cnt, tg);
      if (previous) load_bytes(previous, o, cnt, pv);
      if (fill) load_bytes(fill, o, cnt, fl);
      if (judge) load_bytes(label, o, cnt, lb);

      uint32_t ob[kPerItem], mb[kPerItem], nshown = 0u, nbad = 0u, nws = 0u, nwa = 0u, nnoisy = 0u, nbadid = 0u;
      Run ann_run(Al), kept_run(Kl), fill_run(Fl);
      long long seen = -1;                                           // the run of equal superpixels: n * K + id
      bool sel = false;
      uint32_t av = 0u;
#pragma unroll
      for (int j = 0; j < kPerItem; ++j) {
        ob[j] = (uint32_t)drop_id;
        mb[j] = 0u;
        if (j < cnt) {
          const int k = id[o + j];
          if ((uint32_t)k >= (uint32_t)K) {
            ++nbadid;
            sel = false;
            seen = -1;
          } else if (n * K + k != seen) {
            seen = n * K + k;
            sel = selected[seen] == 255;
            av = answer && sel ? (uint32_t)answer[seen] : 0u;
          }
          const bool valid = target && tg[j] < (uint32_t)nc && (int)tg[j] != ignore_index;
          const bool wrong = judge && valid && lb[j] != tg[j];
          nwa += wrong ? 1u : 0u;
          if (sel && wrong) ++nws;
          if (sel && target && !valid && (int)tg[j] != ignore_index) ++nbad;
          uint32_t unused = 0u;                                      // annotate_pixel's bad count is of what it is GIVEN
          const uint32_t gv = answer ? av : (target ? tg[j] : 0u);
          annotate_pixel(sel, given, gv, previous, pv[j], fill, fl[j], nc, ignore_index, drop_id, ann_run, kept_run,
                         fill_run, ob[j], mb[j], nshown, unused);
          if (sel && valid && ob[j] != tg[j]) ++nnoisy;
          if (++rem == HW) {
            rem = 0;
            ++n;
            seen = -1;
          }
        }
      }
      ann_run.done();
      kept_run.done();
      fill_run.done();
      if (nshown) atomicAdd(&misc[0], nshown);
      if (nbad) atomicAdd(&misc[1], nbad);
      if (nws) atomicAdd(&misc[2], nws);
      if (nwa) atomicAdd(&misc[3], nwa);
      if (nnoisy) atomicAdd(&misc[4], nnoisy);
      if (nbadid) atomicAdd(&misc[5], nbadid);
      if (out) store_bytes(out, o, cnt, ob);
      if (mask) store_bytes(mask, o, cnt, mb);
    }

    const bool last = base + (long long)gridDim.x * kMapWG >= nitems;
    if (last || ++trips == kApplyFlushEvery) {                       // uniform over the work-group
      trips = 0;
      u64* const dst[6] = {shown, bad_targets, wrong_shown, wrong_all, noisy, bad_ids};
      flush_annotator<kMapWG>(Al, Kl, Fl, nc, annotated, kept, filled, misc, dst);
    }
  }
}

// N maps of H x W: positive sizes, sides of at most 4096 and 2^40 pixels in all.
inline bool maps_ok(const char* fn, int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) {
    set_error("%s: bad argument (N %d H %d W %d)", fn, N, H, W);
    return false;
  }
  if (H > MDIL_SPX_MAX_SIDE || W > MDIL_SPX_MAX_SIDE || (long long)N * H > MDIL_SPX_MAX_PIXELS / W) {
    set_error("%s: too large (N %d, maps %d x %d: sides of at most 4096 and 2^40 pixels in all)", fn, N, H, W);
    return false;
  }
  return true;
}

inline bool range_ok(const char* fn, const char* name, int v, int lo, int hi) {
  if (v >= lo && v <= hi) return true;
  set_error("%s: %s=%d outside [%d, %d]", fn, name, v, lo, hi);
  return false;
}

}  // namespace

API int mdil_spx_version(void) { return 100; }
API const char* mdil_spx_last_error(void) { return g_err; }

API int mdil_spx_slic(const float* image, int N, int H, int W, int step, int compactness, int iterations, int* id,
                      int* centres, long long* sums, void* stream) {
  if (!image) {
    set_error("spx_slic: bad argument (image %p)", (const void*)image);
    return MDIL_SPX_ERR_INVALID;
  }
  if (!id || !centres || !sums) {
    set_error("spx_slic: id, centres and sums are all required (id %p centres %p sums %p)", (void*)id, (void*)centres,
              (void*)sums);
    return MDIL_SPX_ERR_INVALID;
  }
  if (!maps_ok(kFnSlic, N, H, W)) return MDIL_SPX_ERR_INVALID;
  if (!range_ok(kFnSlic, "step", step, MDIL_SPX_MIN_STEP, MDIL_SPX_MAX_STEP)) return MDIL_SPX_ERR_INVALID;
  if (!range_ok(kFnSlic, "compactness", compactness, MDIL_SPX_MIN_COMPACTNESS, MDIL_SPX_MAX_COMPACTNESS))
    return MDIL_SPX_ERR_INVALID;
  if (!range_ok(kFnSlic, "iterations", iterations, 0, MDIL_SPX_MAX_ITERATIONS)) return MDIL_SPX_ERR_INVALID;
  if (!aligned8_ok(kFnSlic, "image, id, centres and sums", {image, id, centres, sums})) return MDIL_SPX_ERR_INVALID;

  const int S = step, Gy = (H + S - 1) / S, Gx = (W + S - 1) / S, K = Gy * Gx;
  const int BC = block_cells(S), By = (Gy + BC - 1) / BC, Bx = (Gx + BC - 1) / BC;
  const long long npix = (long long)N * H * W, cells = (long long)N * K, jobs = (long long)N * By * Bx;
  const hipStream_t st = (hipStream_t)stream;
  const int flat_pix = bounded_grid(npix, kFlatWG, kFlatMaxBlocks), flat_cells = bounded_grid(cells, kFlatWG, kFlatMaxBlocks);
  const int grid = bounded_grid(jobs, 1, kAssignMaxBlocks);
  hipLaunchKernelGGL(spx_codes_kernel, dim3(flat_pix), dim3(kFlatWG), 0, st, image, npix, (long long)H * W, id);
  if (!launched(kFnSlic)) return MDIL_SPX_ERR_LAUNCH;
  hipLaunchKernelGGL(spx_init_kernel, dim3(flat_cells), dim3(kFlatWG), 0, st, id, cells, H, W, S, Gx, K, centres, sums);
  if (!launched(kFnSlic)) return MDIL_SPX_ERR_LAUNCH;
  for (int t = 0; t <= iterations; ++t) {
    const int last = t == iterations;
    hipLaunchKernelGGL(spx_assign_kernel, dim3(grid), dim3(kAssignWG), 0, st, id, centres, reinterpret_cast<u64*>(sums),
                       jobs, By, Bx, BC, H, W, S, Gy, Gx, (u64)S * S, (u64)compactness * compactness, last);
    if (!launched(kFnSlic)) return MDIL_SPX_ERR_LAUNCH;
    if (!last) {
      hipLaunchKernelGGL(spx_update_kernel, dim3(flat_cells), dim3(kFlatWG), 0, st, cells, centres, sums);
      if (!launched(kFnSlic)) return MDIL_SPX_ERR_LAUNCH;
    }
  }
  return MDIL_SPX_OK;
}

API int mdil_spx_table(const unsigned char* label, const unsigned short* qmap, const unsigned char* target, int ignore_index,
                       const int* id, int N, int H, int W, int K, int nc, long long* table, long long* tcount,
                       long long* bad_targets, long long* bad_ids, void* stream) {
  if (!label || !qmap || !id) {
    set_error("spx_table: bad argument (label %p qmap %p id %p)", (const void*)label, (const void*)qmap, (const void*)id);
    return MDIL_SPX_ERR_INVALID;
  }
  if (!maps_ok(kFnTable, N, H, W)) return MDIL_SPX_ERR_INVALID;
  if (!classes_ok(kFnTable, nc, MDIL_SPX_MIN_CLASSES, MDIL_SPX_MAX_CLASSES)) return MDIL_SPX_ERR_INVALID;
  if (!ignore_ok(kFnTable, ignore_index)) return MDIL_SPX_ERR_INVALID;
  if (K < 1 || (long long)N * K > MDIL_SPX_MAX_CELLS / (kFields + nc)) {
    set_error("spx_table: K=%d (at least 1, and at most 2^31 cells: N %d x K x (4 + nc %d))", K, N, nc);
    return MDIL_SPX_ERR_INVALID;
  }
  if (!table && !tcount && !bad_targets && !bad_ids) {
    set_error("spx_table: nothing to write (table, tcount and both counters are NULL)");
    return MDIL_SPX_ERR_INVALID;
  }
  if (!target && (tcount || bad_targets)) {
    set_error("spx_table: tcount and bad_targets need a target");
    return MDIL_SPX_ERR_INVALID;
  }
  if (!aligned8_ok(kFnTable, "label, qmap, target, id, table, tcount and the counters",
                   {label, qmap, target, id, table, tcount, bad_targets, bad_ids}))
    return MDIL_SPX_ERR_INVALID;
  const long long npix = (long long)N * H * W;
  const long long nitems = (npix + kPerItem - 1) / kPerItem;
  const int grid = bounded_grid(nitems, kMapWG, kMapMaxBlocks);
  hipLaunchKernelGGL(spx_table_kernel, dim3(grid), dim3(kMapWG), 0, (hipStream_t)stream, label, qmap, target, ignore_index, id,
                     npix, nitems, (long long)H * W, K, nc, reinterpret_cast<u64*>(table), reinterpret_cast<u64*>(tcount),
                     reinterpret_cast<u64*>(bad_targets), reinterpret_cast<u64*>(bad_ids));
  return launched(kFnTable) ? MDIL_SPX_OK : MDIL_SPX_ERR_LAUNCH;
}

API int mdil_spx_apply(const int* id, const unsigned char* selected, const unsigned char* answer, const unsigned char* target,
                       const unsigned char* previous, const unsigned char* fill, const unsigned char* label, int N, int H,
                       int W, int K, int nc, int ignore_index, int drop_id, unsigned char* out, unsigned char* mask,
                       long long* shown, long long* annotated, long long* kept, long long* filled, long long* bad_targets,
                       long long* wrong_shown, long long* wrong_all, long long* noisy, long long* bad_ids, void* stream) {
  if (!id || !selected) {
    set_error("spx_apply: bad argument (id %p selected %p)", (const void*)id, (const void*)selected);
    return MDIL_SPX_ERR_INVALID;
  }
  if (!maps_ok(kFnApply, N, H, W)) return MDIL_SPX_ERR_INVALID;
  if (!classes_ok(kFnApply, nc, MDIL_SPX_MIN_CLASSES, MDIL_SPX_MAX_CLASSES)) return MDIL_SPX_ERR_INVALID;
  if (K < 1) {
    set_error("spx_apply: K=%d (at least 1)", K);
    return MDIL_SPX_ERR_INVALID;
  }
  if (!ignore_ok(kFnApply, ignore_index)) return MDIL_SPX_ERR_INVALID;
  if (!byte_id_ok(kFnApply, "drop_id", drop_id)) return MDIL_SPX_ERR_INVALID;
  if (!apply_outputs_ok(kFnApply, {out, mask, shown, annotated, kept, filled, bad_targets, wrong_shown, wrong_all, noisy, bad_ids}))
    return MDIL_SPX_ERR_INVALID;
  if (annotated && !answer && !target) {
    set_error("spx_apply: annotated needs an answer or a target");
    return MDIL_SPX_ERR_INVALID;
  }
  if (!target && (bad_targets || noisy)) {
    set_error("spx_apply: bad_targets and noisy need a target");
    return MDIL_SPX_ERR_INVALID;
  }
  if ((!target || !label) && (wrong_shown || wrong_all)) {
    set_error("spx_apply: wrong_shown and wrong_all need a target and a label map");
    return MDIL_SPX_ERR_INVALID;
  }
  if (!aligned8_ok(kFnApply, "id, selected, answer, target, previous, fill, label, out, mask and the counters",
                   {id, selected, answer, target, previous, fill, label, out, mask, shown, annotated, kept, filled, bad_targets,
                    wrong_shown, wrong_all, noisy, bad_ids}))
    return MDIL_SPX_ERR_INVALID;
  const long long npix = (long long)N * H * W;
  const long long nitems = (npix + kPerItem - 1) / kPerItem;
  const int grid = bounded_grid(nitems, kMapWG, kMapMaxBlocks);
  hipLaunchKernelGGL(spx_apply_kernel, dim3(grid), dim3(kMapWG), 0, (hipStream_t)stream, id, selected, answer, target, previous,
                     fill, label, npix, nitems, (long long)H * W, K, nc, ignore_index, drop_id, out, mask,
                     reinterpret_cast<u64*>(shown), reinterpret_cast<u64*>(annotated), reinterpret_cast<u64*>(kept),
                     reinterpret_cast<u64*>(filled), reinterpret_cast<u64*>(bad_targets), reinterpret_cast<u64*>(wrong_shown),
                     reinterpret_cast<u64*>(wrong_all), reinterpret_cast<u64*>(noisy), reinterpret_cast<u64*>(bad_ids));
  return launched(kFnApply) ? MDIL_SPX_OK : MDIL_SPX_ERR_LAUNCH;
}
