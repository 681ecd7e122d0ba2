// libmdil_ripu.so: RIPU's sliding (2k+1)^2 regions over stored label and q maps (gfx950).  Integers only.
//
//   ripu_score    one 32-bit key per pixel from the clipped (2k+1)^2 window centred on it: the window's sum of
//                 q, its per-class label counts h_c (through E = tlog[cnt] - sum_c tlog[h_c]) or its wrong pixels
//   ripu_random   the `random` criterion: a SplitMix64 hash per pixel, no window
//   ripu_select   the greedy pick, one work-group per image
//   ripu_apply    acquire_apply's rule with a per-pixel mask
//
// ripu_score.  A work-group of 256 lanes owns a job: kScoreRows output rows of a strip of S = 256 - 2k output
// columns of one image, and with the halo of k columns on either side exactly 256 columns, one per lane.  In
// LDS it keeps, per column, the histogram of the labels over the 2k+1 rows of the vertical window as 16-bit
// counts colh[c][column] (a column holds at most 65 pixels), and beside it the column's sum of q and its count
// of wrong pixels.  The column is on the lanes: [c][x] is conflict-free where [x][c] would put every lane of
// a wave into the same banks.  Going down one row costs a lane one increment (the row that enters) and one
// decrement (the row that leaves) of its own column, both read from the maps one row ahead of their use.  Per
// output row each class is then scanned along the strip by ONE wave (a lane sums its 4 columns, 8-byte LDS
// reads, then a shuffle scan), giving inclusive prefix sums P[c][column]; the window count of a pixel is
// P[c][x + k] - P[c][x - k - 1], and a lane walks the classes for its own pixel, looking tlog up in LDS.
// Columns outside the image are never counted into, rows outside it never enter: the window is clipped, as
// the header says, and cnt is the closed form.  Two barriers per output row.  LDS: 16 KB + 16 KB of counts and
// prefixes, 4 KB for q and wrong, 17 KB of tlog: 53 KB, three work-groups per CU.  The warm-up of a job (up to
// 2k rows counted in before its first output row) is what the row segments cost; kScoreRows = 32 keeps 576
// jobs on 6 x 512 x 1024 at k = 32.  The largest prefix is 256 x 65 = 16,640 (16 bits) and for q
// 256 x 65 x 65,535 < 2^31 (32 bits).
//
// ripu_select.  One work-group of 1024 lanes per image and no waits between work-groups.  The image's flat
// pixels are cut into at most kMaxChunks chunks of 2^s pixels (s >= 6, the smallest that fits); LDS holds per
// chunk the 64-bit word key << 32 | ~index of its best pixel that is not taken (0: none), so that a plain
// maximum orders by key and then by the LOWEST index.  A pick is: the maximum of the chunk words (4 per lane,
// a shuffle tree, 16 partial words), the count of the region's fresh pixels (each lane remembers which of its
// at most 5 pixels were fresh), the budget test, the marks, and a rescan of the chunks the region touched: row
// by row of the region, the chunks a row touches that no row above it touched, one wave per chunk.  The cost
// of a pick grows with the region and with the bounded number of chunks, not with the image; r = 0 rescans
// one chunk.  The marks are read back by the same work-group only, after a barrier (one CU, one L1).
//
// ripu_apply.  acquire_apply's layout: a lane owns 8 consecutive pixels of the flat maps; the counters live in
// LDS as 32-bit integers and are flushed by 64-bit atomics.
#include "../../include/mdil_ripu.h"
#include "map_common.h"

namespace {

constexpr int kMaxC = MDIL_RIPU_MAX_CLASSES;
constexpr int kMaxK = MDIL_RIPU_MAX_RADIUS;
constexpr int kScoreWG = 256;                         // lanes = columns of a strip with its halo
constexpr int kScoreWaves = kScoreWG / 64;
constexpr int kScoreRows = 32;                        // output rows of a job
constexpr int kScoreMaxBlocks = 3072;                 // beyond that the loop over jobs strides
constexpr int kTlogMax = (2 * kMaxK + 1) * (2 * kMaxK + 1) + 1;
constexpr int kFlatWG = 256;
constexpr int kFlatMaxBlocks = 1024;
constexpr int kSelWG = 1024;
constexpr int kSelWaves = kSelWG / 64;
constexpr int kMaxChunks = 4096;                      // 32 KB of 64-bit words
constexpr int kMinChunkShift = 6;
constexpr int kMapWG = 256;
constexpr int kMapMaxBlocks = 512;                    // beyond 131,072 items (of 8 pixels) the loop strides
constexpr char kFnScore[] = "ripu_score";
constexpr char kFnSelect[] = "ripu_select";
constexpr char kFnApply[] = "ripu_apply";

static_assert(kScoreWG * (2 * kMaxK + 1) < 65536, "a 16-bit prefix could wrap");
static_assert((long long)kScoreWG * (2 * kMaxK + 1) * 65535 < (1LL << 31), "the 32-bit prefix of q could wrap");
static_assert(((2 * kMaxK + 1) * (2 * kMaxK + 1) + kSelWG - 1) / kSelWG <= 5, "a lane's mask of fresh pixels holds 5 bits");
static_assert((MDIL_RIPU_MAX_IMAGE_PIXELS >> 12) <= kMaxChunks, "chunks of 2^12 pixels must cover the largest image");

__device__ __forceinline__ u64 mix(u64 seed, u64 j) {
  u64 z = seed + 0x9E3779B97F4A7C15ull * j;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ uint32_t saturate(u64 v) { return v > 0xffffffffull ? 0xffffffffu : (uint32_t)v; }

// Inclusive prefix sum over the 64 lanes of a wave, every lane active.
__device__ __forceinline__ uint32_t wave_scan(uint32_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)v, d, 64);
    v += lane >= d ? t : 0u;
  }
  return v;
}

__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const u64 t = (u64)__shfl_xor((long long)v, m, 64);
    v = t > v ? t : v;
  }
  return v;
}

// What one pixel adds to its column: the label (255: nothing to count), q, and 1 where it is wrong.
struct Px {
  uint32_t l, q, w;
};

__global__ __launch_bounds__(kScoreWG) void ripu_score_kernel(
    const unsigned char* __restrict__ label, const unsigned short* __restrict__ qmap,
    const unsigned char* __restrict__ target, int ignore_index, const unsigned char* __restrict__ taken,
    const int* __restrict__ tlog, long long jobs, int strips, int segs, int Hl, int Wl, int nc, int k, int by,
    uint32_t* __restrict__ key) {
  __shared__ __attribute__((aligned(8))) uint16_t colh[kMaxC][kScoreWG];
  __shared__ __attribute__((aligned(8))) uint16_t P[kMaxC][kScoreWG];
  __shared__ __attribute__((aligned(16))) uint32_t sqc[kScoreWG], Psq[kScoreWG], wrc[kScoreWG], Pwr[kScoreWG];
  __shared__ int tl[kTlogMax];

  const bool need_h = by == MDIL_RIPU_IMPURITY || by == MDIL_RIPU_RIPU;
  const bool need_q = by == MDIL_RIPU_UNCERTAINTY || by == MDIL_RIPU_RIPU;
  const bool need_w = by == MDIL_RIPU_ORACLE;
  const int j = threadIdx.x, lane = j & 63, wave = j >> 6;
  const int S = kScoreWG - 2 * k;
  if (need_h) {
    const int entries = (2 * k + 1) * (2 * k + 1) + 1;
    for (int i = j; i < entries; i += kScoreWG) tl[i] = tlog[i];
  }
  __syncthreads();

  for (long long job = blockIdx.x; job < jobs; job += gridDim.x) {   // uniform over the work-group
    const long long n = job / ((long long)strips * segs);
    const int rem = (int)(job - n * strips * segs);
    const int seg = rem / strips, strip = rem - seg * strips;
    const int x0 = strip * S, y0 = seg * kScoreRows, y1 = min(Hl, y0 + kScoreRows);
    const int gx = x0 - k + j;                                       // this lane's column of the image
    const bool incol = gx >= 0 && gx < Wl;
    const long long img = n * Hl * (long long)Wl;

    auto load = [&](int yy) -> Px {
      Px p = {255u, 0u, 0u};
      if (incol && yy >= 0 && yy < Hl) {
        const long long o = img + (long long)yy * Wl + gx;
        if (need_h) p.l = label[o];
        if (need_q) p.q = qmap[o];
        if (need_w) {
          const uint32_t t = target[o];
          p.w = t < (uint32_t)nc && (int)t != ignore_index && (uint32_t)label[o] != t ? 1u : 0u;
        }
      }
      return p;
    };
    auto count = [&](const Px& p, int sign) {                        // this lane's own column: no other lane writes it
      if (p.l < (uint32_t)nc) colh[p.l][j] = (uint16_t)(colh[p.l][j] + sign);
      if (need_q) sqc[j] += (uint32_t)sign * p.q;
      if (need_w) wrc[j] += (uint32_t)sign * p.w;
    };

    if (need_h)
      for (int c = 0; c < nc; ++c) colh[c][j] = 0;
    sqc[j] = wrc[j] = 0u;
    for (int yy = max(0, y0 - k); yy < min(Hl, y0 + k); ++yy) count(load(yy), 1);   // the rows above the first that enters
    Px enter = load(y0 + k);

    for (int y = y0; y < y1; ++y) {
      const Px leave = load(y - k);                                  // used after the output; in flight meanwhile
      count(enter, 1);
      enter = load(y + k + 1);
      __syncthreads();

      if (need_h) {
        for (int c = wave; c < nc; c += kScoreWaves) {               // one wave per class
          const uint2 v = *reinterpret_cast<const uint2*>(&colh[c][4 * lane]);
          const uint32_t a0 = v.x & 0xffffu, a1 = a0 + (v.x >> 16), a2 = a1 + (v.y & 0xffffu), a3 = a2 + (v.y >> 16);
          const uint32_t base = wave_scan(a3) - a3;
          uint2 o;
          o.x = (base + a0) | (base + a1) << 16;
          o.y = (base + a2) | (base + a3) << 16;
          *reinterpret_cast<uint2*>(&P[c][4 * lane]) = o;
        }
      }
      if ((need_q && wave == kScoreWaves - 1) || (need_w && wave == 0)) {
        const uint32_t* src = need_q ? sqc : wrc;
        uint32_t* dst = need_q ? Psq : Pwr;
        const uint4 v = *reinterpret_cast<const uint4*>(&src[4 * lane]);
        const uint32_t a0 = v.x, a1 = a0 + v.y, a2 = a1 + v.z, a3 = a2 + v.w;
        const uint32_t base = wave_scan(a3) - a3;
        *reinterpret_cast<uint4*>(&dst[4 * lane]) = make_uint4(base + a0, base + a1, base + a2, base + a3);
      }
      __syncthreads();

      if (j >= k && j < kScoreWG - k && gx < Wl) {
        const int lo = j - k - 1, hi = j + k;
        const u64 cnt = (u64)(min(y + k, Hl - 1) - max(y - k, 0) + 1) * (u64)(min(gx + k, Wl - 1) - max(gx - k, 0) + 1);
        u64 E = 0;
        if (need_h) {
          long long e = tl[cnt];
          for (int c = 0; c < nc; ++c) {
            const uint32_t h = (uint32_t)P[c][hi] - (lo >= 0 ? (uint32_t)P[c][lo] : 0u);
            e -= tl[h];
          }
          E = e > 0 ? (u64)e : 0;
        }
        u64 v;
        if (by == MDIL_RIPU_UNCERTAINTY) {
          v = ((u64)(Psq[hi] - (lo >= 0 ? Psq[lo] : 0u)) << 16) / cnt;
        } else if (by == MDIL_RIPU_IMPURITY) {
          v = (E << 16) / cnt;
        } else if (by == MDIL_RIPU_RIPU) {
          v = ((u64)(Psq[hi] - (lo >= 0 ? Psq[lo] : 0u)) * E) / (cnt * cnt);
        } else {
          v = ((u64)(Pwr[hi] - (lo >= 0 ? Pwr[lo] : 0u)) << 32) / (cnt + 1);
        }
        const long long o = img + (long long)y * Wl + gx;
        key[o] = taken && taken[o] ? 0u : saturate(v);
      }
      count(leave, -1);
    }
  }
}

__global__ __launch_bounds__(kFlatWG) void ripu_random_kernel(const unsigned char* __restrict__ taken, long long npix,
                                                              long long HW, u64 seed, u64 image0,
                                                              uint32_t* __restrict__ key) {
  for (long long p = (long long)blockIdx.x * kFlatWG + threadIdx.x; p < npix; p += (long long)gridDim.x * kFlatWG) {
    const long long n = p / HW;
    const u64 z = mix(mix(seed, image0 + (u64)n + 1ull), (u64)(p - n * HW) + 1ull) >> 32;
    key[p] = taken && taken[p] ? 0u : (z ? (uint32_t)z : 1u);
  }
}

// The word of chunk c: the best pixel that is not taken, by one wave.  `taken` is written by this work-group.
__device__ __forceinline__ void scan_chunk(const uint32_t* __restrict__ key, const unsigned char* taken, int HW, int shift,
                                           int c, u64* cmax) {
  const int lane = threadIdx.x & 63;
  const int end = min(HW, (c + 1) << shift);
  u64 best = 0;
  for (int i = (c << shift) + lane; i < end; i += 64) {
    const uint32_t kv = key[i];
    const u64 v = kv && !taken[i] ? (u64)kv << 32 | (u64)(0xffffffffu - (uint32_t)i) : 0ull;
    best = v > best ? v : best;
  }
  best = wave_max(best);
  if (lane == 0) cmax[c] = best;
}

__global__ __launch_bounds__(kSelWG) void ripu_select_kernel(const uint32_t* __restrict__ key_all, unsigned char* taken_all,
                                                             int Hl, int Wl, int r, long long budget, int max_picks,
                                                             int shift, int nchunks, long long* __restrict__ picks,
                                                             long long* __restrict__ count, long long* __restrict__ shown,
                                                             long long* __restrict__ stop) {
  __shared__ u64 cmax[kMaxChunks];
  __shared__ u64 part[kSelWaves];
  __shared__ uint32_t fresh_l;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int HW = Hl * Wl;                                            // at most 2^24 (checked by the host)
  const long long n = blockIdx.x;
  const uint32_t* key = key_all + n * HW;
  unsigned char* taken = taken_all + n * HW;

  for (int c = wave; c < nchunks; c += kSelWaves) scan_chunk(key, taken, HW, shift, c, cmax);
  __syncthreads();

  long long sh = 0;
  int done = 0, why = MDIL_RIPU_STOP_PICKS;
  while (done < max_picks) {                                         // every exit is uniform over the work-group
    u64 b = 0;
    for (int i = tid; i < nchunks; i += kSelWG) b = cmax[i] > b ? cmax[i] : b;
    b = wave_max(b);
    if (lane == 0) part[wave] = b;
    if (tid == 0) fresh_l = 0u;
    __syncthreads();
    b = part[lane & (kSelWaves - 1)];
#pragma unroll
    for (int m = kSelWaves / 2; m >= 1; m >>= 1) {
      const u64 t = (u64)__shfl_xor((long long)b, m, 64);
      b = t > b ? t : b;
    }
    if ((b >> 32) == 0) {
      why = MDIL_RIPU_STOP_EMPTY;
      break;
    }
    const int idx = (int)(0xffffffffu - (uint32_t)b);
    const int y = idx / Wl, x = idx - y * Wl;
    const int ya = max(0, y - r), yb = min(Hl - 1, y + r), xa = max(0, x - r), xb = min(Wl - 1, x + r);
    const int rw = xb - xa + 1, area = rw * (yb - ya + 1);
    uint32_t mine = 0u;                                              // bit s: this lane's s-th pixel of the region is fresh
    for (int t = tid, s = 0; t < area; t += kSelWG, ++s) {
      const int ry = t / rw;
      if (!taken[(ya + ry) * Wl + xa + (t - ry * rw)]) mine |= 1u << s;
    }
    const uint32_t nf = wave_sum_u32((uint32_t)__popc(mine));
    if (lane == 0 && nf) atomicAdd(&fresh_l, nf);
    __syncthreads();
    const uint32_t fresh = fresh_l;
    if (sh + (long long)fresh > budget) {
      why = MDIL_RIPU_STOP_BUDGET;
      break;
    }
    for (int t = tid, s = 0; t < area; t += kSelWG, ++s) {
      const int ry = t / rw;
      if (mine >> s & 1u) taken[(ya + ry) * Wl + xa + (t - ry * rw)] = 255;
    }
    __syncthreads();                                                 // the marks are stored before any lane reads them back
    for (int row = wave; row <= yb - ya; row += kSelWaves) {         // the chunks this row touches and no row above it did
      const int yy = ya + row;
      int a = (yy * Wl + xa) >> shift;
      const int e = (yy * Wl + xb) >> shift;
      if (row > 0) a = max(a, (((yy - 1) * Wl + xb) >> shift) + 1);
      for (int c = a; c <= e; ++c) scan_chunk(key, taken, HW, shift, c, cmax);
    }
    if (tid == 0 && picks) {
      long long* p = picks + (n * max_picks + done) * 4;
      p[0] = y;
      p[1] = x;
      p[2] = (long long)(b >> 32);
      p[3] = fresh;
    }
    sh += fresh;
    ++done;
    __syncthreads();
  }
  if (tid == 0) {
    if (count) count[n] = done;
    if (shown) shown[n] = sh;
    if (stop) stop[n] = why;
  }
}

__global__ __launch_bounds__(kMapWG) void ripu_apply_kernel(
    const unsigned char* __restrict__ selected, const unsigned char* __restrict__ target,
    const unsigned char* __restrict__ previous, const unsigned char* __restrict__ fill,
    const unsigned char* __restrict__ label, long long npix, long long nitems, int nc, int ignore_index, int drop_id,
    unsigned char* __restrict__ out, unsigned char* __restrict__ mask, u64* __restrict__ shown, u64* __restrict__ annotated,
    u64* __restrict__ kept, u64* __restrict__ filled, u64* __restrict__ bad_targets, u64* __restrict__ wrong_shown,
    u64* __restrict__ wrong_all) {
  __shared__ uint32_t Al[kMaxC], Kl[kMaxC], Fl[kMaxC];               // annotated, kept, filled
  __shared__ uint32_t misc[4];                                       // shown, bad targets, wrong shown, wrong all
  zero_annotator<kMapWG>(Al, Kl, Fl, nc, misc);

  const bool judge = target && label;
  int trips = 0;
  for (long long base = (long long)blockIdx.x * kMapWG; base < nitems; base += (long long)gridDim.x * kMapWG) {
    const long long item = base + threadIdx.x;
    if (item < nitems) {
      const long long o = item * kPerItem;
      const int n = o + kPerItem <= npix ? kPerItem : (int)(npix - o);
      uint32_t sl[kPerItem], tg[kPerItem], pv[kPerItem], fl[kPerItem], lb[kPerItem];
      load_bytes(selected, o, n, sl);
      if (target) load_bytes(target, o, n, tg);
      if (previous) load_bytes(previous, o, n, pv);
      if (fill) load_bytes(fill, o, n, fl);
      if (judge) load_bytes(label, o, n, lb);

      uint32_t ob[kPerItem], mb[kPerItem], nshown = 0u, nbad = 0u, nws = 0u, nwa = 0u;
      Run ann_run(Al), kept_run(Kl), fill_run(Fl);
#pragma unroll
      for (int j = 0; j < kPerItem; ++j) {
        ob[j] = (uint32_t)drop_id;
        mb[j] = 0u;
        if (j < n) {
          const bool sel = sl[j] == 255u;
          const bool wrong = judge && tg[j] < (uint32_t)nc && (int)tg[j] != ignore_index && lb[j] != tg[j];
          nwa += wrong ? 1u : 0u;
          if (sel && wrong) ++nws;
          annotate_pixel(sel, target, tg[j], previous, pv[j], fill, fl[j], nc, ignore_index, drop_id, ann_run, kept_run,
                         fill_run, ob[j], mb[j], nshown, nbad);
        }
      }
      ann_run.done();
      kept_run.done();
      fill_run.done();
      if (nshown) atomicAdd(&misc[0], nshown);
      if (nbad) atomicAdd(&misc[1], nbad);
      if (nws) atomicAdd(&misc[2], nws);
      if (nwa) atomicAdd(&misc[3], nwa);
      if (out) store_bytes(out, o, n, ob);
      if (mask) store_bytes(mask, o, n, mb);
    }

    const bool last = base + (long long)gridDim.x * kMapWG >= nitems;
    if (last || ++trips == kApplyFlushEvery) {                       // uniform over the work-group
      trips = 0;
      u64* const dst[4] = {shown, bad_targets, wrong_shown, wrong_all};
      flush_annotator<kMapWG>(Al, Kl, Fl, nc, annotated, kept, filled, misc, dst);
    }
  }
}

// N maps of Hl x Wl: positive sizes, at most 2^24 pixels per image and 2^40 in all.
inline bool maps_ok(const char* fn, int N, int Hl, int Wl) {
  if (N <= 0 || Hl <= 0 || Wl <= 0) {
    set_error("%s: bad argument (N %d Hl %d Wl %d)", fn, N, Hl, Wl);
    return false;
  }
  if ((long long)Hl * Wl > MDIL_RIPU_MAX_IMAGE_PIXELS || (long long)N * Hl > MDIL_RIPU_MAX_PIXELS / Wl) {
    set_error("%s: too large (N %d, maps %d x %d: at most 2^24 pixels per image and 2^40 in all)", fn, N, Hl, Wl);
    return false;
  }
  return true;
}

}  // namespace

API int mdil_ripu_version(void) { return 100; }
API const char* mdil_ripu_last_error(void) { return g_err; }

API int mdil_ripu_score(const unsigned char* label, const unsigned short* qmap, const unsigned char* target,
                        int ignore_index, const unsigned char* taken, const int* tlog, int N, int Hl, int Wl, int nc, int k,
                        int by, long long seed, long long image0, unsigned int* key, void* stream) {
  if (!label) {
    set_error("ripu_score: bad argument (label %p)", (const void*)label);
    return MDIL_RIPU_ERR_INVALID;
  }
  if (!key) {
    set_error("ripu_score: nothing to write (key is NULL)");
    return MDIL_RIPU_ERR_INVALID;
  }
  if (!maps_ok(kFnScore, N, Hl, Wl)) return MDIL_RIPU_ERR_INVALID;
  if (!classes_ok(kFnScore, nc, MDIL_RIPU_MIN_CLASSES, MDIL_RIPU_MAX_CLASSES)) return MDIL_RIPU_ERR_INVALID;
  if (k < MDIL_RIPU_MIN_RADIUS || k > MDIL_RIPU_MAX_RADIUS) {
    set_error("ripu_score: k=%d outside [%d, %d]", k, MDIL_RIPU_MIN_RADIUS, MDIL_RIPU_MAX_RADIUS);
    return MDIL_RIPU_ERR_INVALID;
  }
  if (by < 0 || by >= MDIL_RIPU_CRITERIA) {
    set_error("ripu_score: by=%d (0 uncertainty, 1 impurity, 2 ripu, 3 oracle, 4 random)", by);
    return MDIL_RIPU_ERR_INVALID;
  }
  if (!ignore_ok(kFnScore, ignore_index)) return MDIL_RIPU_ERR_INVALID;
  if (!qmap && (by == MDIL_RIPU_UNCERTAINTY || by == MDIL_RIPU_RIPU)) {
    set_error("ripu_score: by=%d needs a qmap", by);
    return MDIL_RIPU_ERR_INVALID;
  }
  if (!target && by == MDIL_RIPU_ORACLE) {
    set_error("ripu_score: by=%d needs a target", by);
    return MDIL_RIPU_ERR_INVALID;
  }
  if (!tlog && (by == MDIL_RIPU_IMPURITY || by == MDIL_RIPU_RIPU)) {
    set_error("ripu_score: by=%d needs the tlog table", by);
    return MDIL_RIPU_ERR_INVALID;
  }
  if (image0 < 0) {
    set_error("ripu_score: image0=%lld is negative", image0);
    return MDIL_RIPU_ERR_INVALID;
  }
  if (((uintptr_t)label & 7) || ((uintptr_t)qmap & 7) || ((uintptr_t)target & 7) || ((uintptr_t)taken & 7) ||
      ((uintptr_t)tlog & 7) || ((uintptr_t)key & 7)) {
    set_error("ripu_score: alignment (label, qmap, target, taken, tlog and key 8 B)");
    return MDIL_RIPU_ERR_INVALID;
  }
  const long long npix = (long long)N * Hl * Wl;
  if (by == MDIL_RIPU_RANDOM) {
    const int grid = bounded_grid(npix, kFlatWG, kFlatMaxBlocks);
    hipLaunchKernelGGL(ripu_random_kernel, dim3(grid), dim3(kFlatWG), 0, (hipStream_t)stream, taken, npix,
                       (long long)Hl * Wl, (u64)seed, (u64)image0, key);
    return launched(kFnScore) ? MDIL_RIPU_OK : MDIL_RIPU_ERR_LAUNCH;
  }
  const int S = kScoreWG - 2 * k;
  const int strips = (Wl + S - 1) / S, segs = (Hl + kScoreRows - 1) / kScoreRows;
  const long long jobs = (long long)N * strips * segs;
  const int grid = bounded_grid(jobs, 1, kScoreMaxBlocks);
  hipLaunchKernelGGL(ripu_score_kernel, dim3(grid), dim3(kScoreWG), 0, (hipStream_t)stream, label, qmap, target,
                     ignore_index, taken, tlog, jobs, strips, segs, Hl, Wl, nc, k, by, key);
  return launched(kFnScore) ? MDIL_RIPU_OK : MDIL_RIPU_ERR_LAUNCH;
}

API int mdil_ripu_select(const unsigned int* key, unsigned char* taken, int N, int Hl, int Wl, int r,
                         long long budget_pixels, int max_picks, long long* picks, long long* count, long long* shown,
                         long long* stop, void* stream) {
  if (!key || !taken) {
    set_error("ripu_select: bad argument (key %p taken %p)", (const void*)key, (const void*)taken);
    return MDIL_RIPU_ERR_INVALID;
  }
  if (!maps_ok(kFnSelect, N, Hl, Wl)) return MDIL_RIPU_ERR_INVALID;
  if (r < 0 || r > MDIL_RIPU_MAX_RADIUS) {
    set_error("ripu_select: r=%d outside [0, %d]", r, MDIL_RIPU_MAX_RADIUS);
    return MDIL_RIPU_ERR_INVALID;
  }
  if (budget_pixels < 0) {
    set_error("ripu_select: budget_pixels=%lld is negative", budget_pixels);
    return MDIL_RIPU_ERR_INVALID;
  }
  if (max_picks < 1 || max_picks > MDIL_RIPU_MAX_PICKS) {
    set_error("ripu_select: max_picks=%d outside [1, %d]", max_picks, MDIL_RIPU_MAX_PICKS);
    return MDIL_RIPU_ERR_INVALID;
  }
  if (((uintptr_t)key & 7) || ((uintptr_t)taken & 7) || ((uintptr_t)picks & 7) || ((uintptr_t)count & 7) ||
      ((uintptr_t)shown & 7) || ((uintptr_t)stop & 7)) {
    set_error("ripu_select: alignment (key, taken, picks, count, shown and stop 8 B)");
    return MDIL_RIPU_ERR_INVALID;
  }
  const int HW = Hl * Wl;
  int shift = kMinChunkShift;
  while (((HW - 1) >> shift) + 1 > kMaxChunks) ++shift;
  const int nchunks = ((HW - 1) >> shift) + 1;
  hipLaunchKernelGGL(ripu_select_kernel, dim3(N), dim3(kSelWG), 0, (hipStream_t)stream, key, taken, Hl, Wl, r,
                     budget_pixels, max_picks, shift, nchunks, picks, count, shown, stop);
  return launched(kFnSelect) ? MDIL_RIPU_OK : MDIL_RIPU_ERR_LAUNCH;
}

API int mdil_ripu_apply(const unsigned char* selected, const unsigned char* target, const unsigned char* previous,
                        const unsigned char* fill, const unsigned char* label, int N, int Hl, int Wl, int nc,
                        int ignore_index, int drop_id, unsigned char* out, unsigned char* mask, long long* shown,
                        long long* annotated, long long* kept, long long* filled, long long* bad_targets,
                        long long* wrong_shown, long long* wrong_all, void* stream) {
  if (!selected) {
    set_error("ripu_apply: bad argument (selected %p)", (const void*)selected);
    return MDIL_RIPU_ERR_INVALID;
  }
  if (!maps_ok(kFnApply, N, Hl, Wl)) return MDIL_RIPU_ERR_INVALID;
  if (!classes_ok(kFnApply, nc, MDIL_RIPU_MIN_CLASSES, MDIL_RIPU_MAX_CLASSES)) return MDIL_RIPU_ERR_INVALID;
  if (!ignore_ok(kFnApply, ignore_index)) return MDIL_RIPU_ERR_INVALID;
  if (!byte_id_ok(kFnApply, "drop_id", drop_id)) return MDIL_RIPU_ERR_INVALID;
  if (!apply_outputs_ok(kFnApply, {out, mask, shown, annotated, kept, filled, bad_targets, wrong_shown, wrong_all}))
    return MDIL_RIPU_ERR_INVALID;
  if (!apply_target_ok(kFnApply, target, annotated, bad_targets)) return MDIL_RIPU_ERR_INVALID;
  if ((!target || !label) && (wrong_shown || wrong_all)) {
    set_error("ripu_apply: wrong_shown and wrong_all need a target and a label map");
    return MDIL_RIPU_ERR_INVALID;
  }
  if (!aligned8_ok(kFnApply, "selected, target, previous, fill, label, out, mask and the counters",
                   {selected, target, previous, fill, label, out, mask, shown, annotated, kept, filled, bad_targets,
                    wrong_shown, wrong_all}))
    return MDIL_RIPU_ERR_INVALID;
  const long long npix = (long long)N * Hl * Wl;
  const long long nitems = (npix + kPerItem - 1) / kPerItem;
  const int grid = bounded_grid(nitems, kMapWG, kMapMaxBlocks);
  hipLaunchKernelGGL(ripu_apply_kernel, dim3(grid), dim3(kMapWG), 0, (hipStream_t)stream, selected, target, previous, fill,
                     label, npix, nitems, nc, ignore_index, drop_id, out, mask, reinterpret_cast<u64*>(shown),
                     reinterpret_cast<u64*>(annotated), reinterpret_cast<u64*>(kept), reinterpret_cast<u64*>(filled),
                     reinterpret_cast<u64*>(bad_targets), reinterpret_cast<u64*>(wrong_shown),
                     reinterpret_cast<u64*>(wrong_all));
  return launched(kFnApply) ? MDIL_RIPU_OK : MDIL_RIPU_ERR_LAUNCH;
}
