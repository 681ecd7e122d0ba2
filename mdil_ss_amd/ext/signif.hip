// libmdil_signif.so: per-image class counts of two u8 label maps, and replicates of their sum over
// resampled images scored by the iouEval rule (gfx950; include/mdil_signif.h has the definitions).
// The counts and the replicate sums are integers: nothing is rounded before the score, and every
// output is a function of the input, the seed and the replicate index alone.
//
// mdil_signif_count (signif_count_kernel).  A work-group takes units of kUnit consecutive pixels of
// ONE image, so its table in LDS ([3][nc] and the two stray counters, 32 bits: a unit has 8192
// pixels) belongs to one row of `counts`, and flushes it with one global 64-bit add per non-zero
// entry before the next unit.  A lane owns 16 consecutive pixels (one 16-byte load per map where the
// image size and the pointers allow it, dwords or bytes otherwise) and walks them as runs of equal
// (target, prediction) pairs: a run costs its adds once, whatever its length.  The lane's last run is
// then aggregated in the wave as segments.hip's wave_add does -- the first pending lane's pair is
// broadcast, every lane holding it hands its length to a shuffle tree, the leader adds once -- for at
// most kWaveKeys pairs; lanes still pending after that add for themselves.  An image of one label
// therefore costs one set of LDS adds per 1024 pixels, and noise costs what plain adds cost.
//
// mdil_signif_resample (signif_resample_kernel<mode, column chunks>).  One wavefront per replicate, four per
// work-group, striding over the replicates.  The 64 lanes hash 64 draws at once; each draw is then
// read back with v_readlane -- a scalar, so the row's address is one -- and the lanes add that
// row's columns from coalesced 8-byte loads: column lane + 64 k in accumulator k, at most three
// (2 * 3 * 32 = 192 columns), kBatch rows' loads in flight before the first add waits for one.
// Lanes past the last column read column 0 and their sums are never used.  The table (M x G*3*nc x 8 bytes: 480 KB at 500 images, 20 classes, two groups) is read
// from the L2.  SWAP walks the rows in order and picks, by the row's bit, between a lane's own
// column and the same column of the other group.  JACKKNIFE sums the whole table once per
// work-group (its four waves take every fourth row, the partial sums meet in LDS) and subtracts a
// row per replicate.  The epilogue stages the column sums in LDS; lane g*32 + c scores class c of
// group g in fp64 (adds and one correctly rounded divide: nothing here can be contracted), a
// ballot collects the empty classes, and lane g adds the k scores in class order.
//
// Where one group's slice of the table fits in LDS as 32-bit entries (M * 3 nc <= 32768: 546 images at
// 20 classes) the bootstrap runs from there instead (signif_bootstrap_lds_kernel, its comment below).
//
// Grids are capped and the loops stride past the cap; every loop that holds a barrier or a
// shuffle has a trip count uniform over the work-group or the wave.
#include "../../include/mdil_signif.h"
#include "head_common.h"

namespace {

constexpr int kWG = 256;                             // 4 wavefronts of 64 lanes
constexpr int kWaves = kWG / 64;
constexpr int kLanePixels = 16;
constexpr int kSteps = 2;
constexpr int kStepPixels = kWG * kLanePixels;       // 4096
constexpr int kUnit = kStepPixels * kSteps;          // pixels of one image a work-group counts per flush
constexpr int kWaveKeys = 4;                         // pairs aggregated over the wave per step
constexpr int kMaxCountBlocks = 8192;
constexpr int kMaxCols = MDIL_SIGNIF_MAX_GROUPS * 3 * MDIL_SIGNIF_MAX_CLASSES;       // 192
constexpr int kChunks = kMaxCols / 64;               // accumulators per lane
constexpr int kMaxResampleBlocks = 16384;
constexpr int kMaxJackknifeBlocks = 512;             // each sums the whole table once
constexpr int kBatch = 8;                            // rows whose loads are in flight together
constexpr int kLdsWG = 1024;                         // the bootstrap from LDS: 16 wavefronts share one slice
constexpr int kLdsWaves = kLdsWG / 64;
constexpr int kLdsEntries = 32768;                   // u32 entries of one group's slice: 128 KB of the 160 KB
constexpr int kGroupCols = 3 * MDIL_SIGNIF_MAX_CLASSES;
constexpr int kLdsBlocks = 256;                      // work-groups over all groups: one per CU

// ------------------------------------------------------------------------------------- count
// 16 pixels at byte offset o, one per byte of v[0..3]; `valid` of them exist (<= 0: none).
// mode 2: o is a multiple of 16 and valid == 16; mode 1: o is a multiple of 4 and so is valid.
template <int mode>
__device__ __forceinline__ void load16(const unsigned char* __restrict__ p, long long o, int valid, uint32_t (&v)[4]) {
  v[0] = v[1] = v[2] = v[3] = 0u;
  if (valid <= 0) return;
  if (mode == 2) {
    const uint4 q = *reinterpret_cast<const uint4*>(p + o);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else if (mode == 1) {
#pragma unroll
    for (int d = 0; d < 4; ++d)
      if (4 * d < valid) v[d] = *reinterpret_cast<const uint32_t*>(p + o + 4 * d);
  } else {
#pragma unroll
    for (int j = 0; j < kLanePixels; ++j)
      if (j < valid) v[j >> 2] |= (uint32_t)p[o + j] << (8 * (j & 3));
  }
}

// n pixels of the pair key = target << 8 | prediction into the table [tp nc][predicted nc][labelled nc]
// [bad_targets][unpredicted].
__device__ __forceinline__ void emit(uint32_t* cnt, int nc, int ignore_index, uint32_t key, uint32_t n) {
  const int t = (int)(key >> 8), p = (int)(key & 0xffu);
  if (t == ignore_index) return;
  if (t >= nc) {
    atomicAdd(&cnt[3 * nc], n);
    return;
  }
  atomicAdd(&cnt[2 * nc + t], n);
  atomicAdd(p < nc ? &cnt[nc + p] : &cnt[3 * nc + 1], n);
  if (p == t) atomicAdd(&cnt[t], n);
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// rows: the entry [first_image][g][0][0] of the table; row_stride = G * 3 * nc.
template <int mode>
__global__ __launch_bounds__(kWG) void signif_count_kernel(const unsigned char* __restrict__ pred,
                                                           const unsigned char* __restrict__ target,
                                                           long long units, long long per_image, int P, int nc,
                                                           int ignore_index, unsigned long long* rows,
                                                           int row_stride, unsigned long long* bad_targets,
                                                           unsigned long long* unpredicted) {
  __shared__ uint32_t cnt[3 * MDIL_SIGNIF_MAX_CLASSES + 2];
  const int n_all = 3 * nc + 2, lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < n_all; i += kWG) cnt[i] = 0u;

  // work-group-uniform loops: the barriers and the shuffles below run with every lane
  for (long long u = blockIdx.x; u < units; u += gridDim.x) {
    __syncthreads();                                 // the table is clear
    const long long n = u / per_image;
    const int chunk = (int)(u - n * per_image);
    const long long img = n * P;
    for (int s = 0; s < kSteps; ++s) {
      // chunk * kUnit < P <= 2^30, so base stays below 2^31
      const int base = chunk * kUnit + s * kStepPixels + (int)threadIdx.x * kLanePixels;
      const int valid = min(kLanePixels, P - base);
      uint32_t tv[4], pv[4];
      load16<mode>(target, img + base, valid, tv);
      load16<mode>(pred, img + base, valid, pv);
      uint32_t key = 0xffffffffu, len = 0u;
#pragma unroll
      for (int j = 0; j < kLanePixels; ++j) {
        if (j >= valid) continue;
        const uint32_t k = ((tv[j >> 2] >> (8 * (j & 3))) & 0xffu) << 8 | ((pv[j >> 2] >> (8 * (j & 3))) & 0xffu);
        if (k != key) {
          if (len) emit(cnt, nc, ignore_index, key, len);
          key = k;
          len = 0u;
        }
        ++len;
      }
      bool pend = len != 0u;
      for (int it = 0; it < kWaveKeys; ++it) {
        const unsigned long long have = __ballot(pend);
        if (!have) break;
        const int leader = __ffsll((long long)have) - 1;
        const uint32_t k = (uint32_t)__shfl((int)key, leader, 64);
        const bool take = pend && key == k;
        const uint32_t total = wave_sum_u32(take ? len : 0u);
        if (lane == leader) emit(cnt, nc, ignore_index, k, total);
        pend = pend && !take;
      }
      if (pend) emit(cnt, nc, ignore_index, key, len);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_all; i += kWG) {
      const uint32_t v = cnt[i];
      if (!v) continue;
      cnt[i] = 0u;
      atomicAdd(i < 3 * nc ? rows + n * row_stride + i : i == 3 * nc ? bad_targets : unpredicted,
                (unsigned long long)v);
    }
  }
}

// ---------------------------------------------------------------------------------- resample
struct ResampleArgs {
  const long long* counts;
  long long* sums;
  double* miou;
  double* iou;
  uint32_t* empty;
  unsigned long long seed, first;
  long long B;
  int M, G, nc, k;
};

__device__ __forceinline__ unsigned long long mix(unsigned long long seed, unsigned long long K) {
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * K;
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

// acc += the columns of the row picked by lane r of `pick` (BOOTSTRAP: the row's index; SWAP: row
// `at`, and the bit that exchanges its groups), for kBatch rows at once: the loads of a batch are
// issued before the first add waits for one.
template <int MODE, int NCH, int ROWS>
__device__ __forceinline__ void add_rows(const long long* __restrict__ counts, int C, int pick, int r, int at,
                                         const int (&col)[kChunks], const int (&other)[kChunks],
                                         long long (&acc)[kChunks]) {
  long long v[ROWS][NCH];
#pragma unroll
  for (int u = 0; u < ROWS; ++u) {
    const int p = __builtin_amdgcn_readlane(pick, r + u);          // wave-uniform: a row index or a bit
    const long long* rowp = counts + (long long)(MODE == MDIL_SIGNIF_BOOTSTRAP ? p : at + u) * C;
#pragma unroll
    for (int k = 0; k < NCH; ++k) v[u][k] = rowp[MODE == MDIL_SIGNIF_SWAP && p ? other[k] : col[k]];
  }
#pragma unroll
  for (int u = 0; u < ROWS; ++u)
#pragma unroll
    for (int k = 0; k < NCH; ++k) acc[k] += v[u][k];
}

template <int MODE, int NCH>
__global__ __launch_bounds__(kWG) void signif_resample_kernel(const ResampleArgs a) {
  __shared__ long long stage[kWaves][kMaxCols];
  __shared__ double scores[kWaves][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int M = a.M, G = a.G, nc = a.nc, C = G * 3 * nc, half = C >> 1;       // NCH = ceil(C / 64)
  const long long* __restrict__ counts = a.counts;
  int col[kChunks], other[kChunks];                  // a lane's columns (0 past the last), and the other group's
#pragma unroll
  for (int k = 0; k < kChunks; ++k) {
    col[k] = lane + 64 * k < C ? lane + 64 * k : 0;
    other[k] = col[k] < half ? col[k] + half : col[k] - half;
  }

  long long total[kChunks] = {0, 0, 0};
  if (MODE == MDIL_SIGNIF_JACKKNIFE) {
    for (int i = wave; i < M; i += kWaves) {
      const long long* rowp = counts + (long long)i * C;
#pragma unroll
      for (int k = 0; k < kChunks; ++k)
        if (k < NCH) total[k] += rowp[col[k]];
    }
#pragma unroll
    for (int k = 0; k < kChunks; ++k) stage[wave][lane + 64 * k] = total[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kChunks; ++k) {
      total[k] = 0;
      for (int w = 0; w < kWaves; ++w) total[k] += stage[w][lane + 64 * k];
    }
    __syncthreads();
  }

  // work-group-uniform loop (barriers inside); `active` is wave-uniform
  for (long long base = (long long)blockIdx.x * kWaves; base < a.B; base += (long long)gridDim.x * kWaves) {
    const long long bi = base + wave;
    const bool active = bi < a.B;
    long long acc[kChunks] = {0, 0, 0};
    if (active) {
      const unsigned long long b = a.first + (unsigned long long)bi;
      if (MODE == MDIL_SIGNIF_JACKKNIFE) {
        const long long* rowp = counts + (long long)b * C;         // b < M: checked by the host
#pragma unroll
        for (int k = 0; k < kChunks; ++k)
          if (k < NCH) acc[k] = total[k] - rowp[col[k]];
      } else {
        for (int j0 = 0; j0 < M; j0 += 64) {
          const unsigned long long z = mix(a.seed, (b << 32) + (unsigned long long)(j0 + lane) + 1ull);
          const int pick = MODE == MDIL_SIGNIF_BOOTSTRAP ? (int)(((z >> 32) * (unsigned long long)M) >> 32)
                                                         : (int)(z >> 63);
          const int draws = min(64, M - j0);
          int r = 0;
          for (; r + kBatch <= draws; r += kBatch)
            add_rows<MODE, NCH, kBatch>(counts, C, pick, r, j0 + r, col, other, acc);
          for (; r < draws; ++r) add_rows<MODE, NCH, 1>(counts, C, pick, r, j0 + r, col, other, acc);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kChunks; ++k) {
      stage[wave][lane + 64 * k] = acc[k];
      if (active && a.sums && lane + 64 * k < C) a.sums[bi * C + lane + 64 * k] = acc[k];
    }
    __syncthreads();
    const int g = lane >> 5, c = lane & 31;
    const bool scored = g < G && c < nc;
    double v = 0.0;
    bool none = false;
    if (scored) {
      const long long tp = stage[wave][(g * 3 + 0) * nc + c], pr = stage[wave][(g * 3 + 1) * nc + c],
                      lb = stage[wave][(g * 3 + 2) * nc + c];
      const double both = (double)tp, fp = (double)pr - both, fn = (double)lb - both;
      v = both / (both + fp + fn + 1e-15);
      none = pr + lb == 0;
    }
    const unsigned long long mask = __ballot(none);
    scores[wave][lane] = v;
    if (active && a.iou && scored && c < a.k) a.iou[(bi * G + g) * a.k + c] = v;
    __syncthreads();
    if (active && lane < G) {
      double s = 0.0;
      for (int i = 0; i < a.k; ++i) s += scores[wave][lane * 32 + i];
      a.miou[bi * G + lane] = s / (double)a.k;
      if (a.empty) a.empty[bi * G + lane] = (uint32_t)(mask >> (32 * lane));
    }
  }
}

// The bootstrap where one group's slice of the table fits in LDS as 32-bit entries ([M][3 nc], at
// most kLdsEntries of them; the entries are below 2^31 by contract).  A work-group of 16 wavefronts
// owns one group g (blockIdx.y) -- a group's score needs that group's columns only --, copies the
// slice once and strides over the replicates, one wavefront each: the same draws, read back with
// v_readlane, now index LDS rows, and the lanes add column lane and, with TWO (3 nc > 64), lane + 64.
template <bool TWO>
__global__ __launch_bounds__(kLdsWG) void signif_bootstrap_lds_kernel(const ResampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t slice[];     // [M][Cg]
  __shared__ long long stage[kLdsWaves][kGroupCols];
  __shared__ double scores[kLdsWaves][MDIL_SIGNIF_MAX_CLASSES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = blockIdx.y;
  const int M = a.M, G = a.G, nc = a.nc, Cg = 3 * nc, C = G * Cg;
  for (int i = threadIdx.x; i < M * Cg; i += kLdsWG) {
    const int row = i / Cg;
    slice[i] = (uint32_t)a.counts[(long long)row * C + g * Cg + (i - row * Cg)];
  }
  __syncthreads();
  const int c0 = lane < Cg ? lane : 0, c1 = lane + 64 < Cg ? lane + 64 : 0;     // 0 past the last column: never used

  // work-group-uniform loop (barriers inside); `active` is wave-uniform
  for (long long base = (long long)blockIdx.x * kLdsWaves; base < a.B; base += (long long)gridDim.x * kLdsWaves) {
    const long long bi = base + wave;
    const bool active = bi < a.B;
    long long acc0 = 0, acc1 = 0;
    if (active) {
      const unsigned long long b = a.first + (unsigned long long)bi;
      for (int j0 = 0; j0 < M; j0 += 64) {
        const unsigned long long z = mix(a.seed, (b << 32) + (unsigned long long)(j0 + lane) + 1ull);
        const int pick = (int)(((z >> 32) * (unsigned long long)M) >> 32) * Cg;       // the row's offset: < kLdsEntries
        const int draws = min(64, M - j0);
        int r = 0;
        for (; r + kBatch <= draws; r += kBatch) {
          uint32_t v0[kBatch], v1[kBatch];
#pragma unroll
          for (int u = 0; u < kBatch; ++u) {
            const int at = __builtin_amdgcn_readlane(pick, r + u);
            v0[u] = slice[at + c0];
            v1[u] = TWO ? slice[at + c1] : 0u;
          }
#pragma unroll
          for (int u = 0; u < kBatch; ++u) acc0 += v0[u], acc1 += v1[u];
        }
        for (; r < draws; ++r) {
          const int at = __builtin_amdgcn_readlane(pick, r);
          acc0 += slice[at + c0];
          if (TWO) acc1 += slice[at + c1];
        }
      }
    }
    stage[wave][lane] = acc0;
    if (lane + 64 < kGroupCols) stage[wave][lane + 64] = acc1;
    if (active && a.sums) {
      long long* out = a.sums + (bi * G + g) * Cg;
      if (lane < Cg) out[lane] = acc0;
      if (lane + 64 < Cg) out[lane + 64] = acc1;
    }
    __syncthreads();
    const bool scored = lane < nc;
    double v = 0.0;
    bool none = false;
    if (scored) {
      const long long tp = stage[wave][lane], pr = stage[wave][nc + lane], lb = stage[wave][2 * nc + lane];
      const double both = (double)tp, fp = (double)pr - both, fn = (double)lb - both;
      v = both / (both + fp + fn + 1e-15);
      none = pr + lb == 0;
      scores[wave][lane] = v;
    }
    const unsigned long long mask = __ballot(none);
    if (active && a.iou && scored && lane < a.k) a.iou[(bi * G + g) * a.k + lane] = v;
    __syncthreads();
    if (active && lane == 0) {
      double t = 0.0;
      for (int i = 0; i < a.k; ++i) t += scores[wave][i];
      a.miou[bi * G + g] = t / (double)a.k;
      if (a.empty) a.empty[bi * G + g] = (uint32_t)mask;
    }
  }
}

// -------------------------------------------------------------------------------------- host
inline bool misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

bool table_ok(const char* fn, long long M, int G) {
  if (M < 1 || M > MDIL_SIGNIF_MAX_IMAGES) {
    set_error("%s: M=%lld outside [1, %lld]", fn, M, MDIL_SIGNIF_MAX_IMAGES);
    return false;
  }
  if (G < 1 || G > MDIL_SIGNIF_MAX_GROUPS) {
    set_error("%s: G=%d outside [1, %d]", fn, G, MDIL_SIGNIF_MAX_GROUPS);
    return false;
  }
  return true;
}

}  // namespace

API int mdil_signif_version(void) { return 100; }
API const char* mdil_signif_last_error(void) { return g_err; }

API int mdil_signif_count(const unsigned char* pred, const unsigned char* target, int N, int H, int W, int nc,
                          int ignore_index, long long first_image, long long M, int G, int g, long long* counts,
                          long long* bad_targets, long long* unpredicted, void* stream) {
  constexpr char fn[] = "signif_count";
  if (!pred || !target || !counts || !bad_targets || !unpredicted || N <= 0 || H <= 0 || W <= 0) {
    set_error("signif_count: bad argument (pred %p target %p counts %p bad_targets %p unpredicted %p N %d H %d W %d)",
              (const void*)pred, (const void*)target, (void*)counts, (void*)bad_targets, (void*)unpredicted, N, H, W);
    return MDIL_SIGNIF_ERR_INVALID;
  }
  if (!classes_ok(fn, nc, MDIL_SIGNIF_MIN_CLASSES, MDIL_SIGNIF_MAX_CLASSES)) return MDIL_SIGNIF_ERR_INVALID;
  if (H > MDIL_SIGNIF_MAX_SIZE || W > MDIL_SIGNIF_MAX_SIZE) {
    set_error("signif_count: size %d x %d above %d", H, W, MDIL_SIGNIF_MAX_SIZE);
    return MDIL_SIGNIF_ERR_INVALID;
  }
  if ((long long)N * H > MDIL_SIGNIF_MAX_PIXELS / W) {
    set_error("signif_count: too large (N %d, maps %d x %d: at most 2^40 pixels)", N, H, W);
    return MDIL_SIGNIF_ERR_INVALID;
  }
  if (!ignore_ok(fn, ignore_index) || !table_ok(fn, M, G)) return MDIL_SIGNIF_ERR_INVALID;
  if (g < 0 || g >= G) {
    set_error("signif_count: group g=%d outside [0, %d)", g, G);
    return MDIL_SIGNIF_ERR_INVALID;
  }
  if (first_image < 0 || first_image > M - N) {
    set_error("signif_count: rows first_image=%lld .. +%d outside the table's %lld", first_image, N, M);
    return MDIL_SIGNIF_ERR_INVALID;
  }
  if (misaligned(pred, 3) || misaligned(target, 3) || misaligned(counts, 7) || misaligned(bad_targets, 7) ||
      misaligned(unpredicted, 7)) {
    set_error("signif_count: alignment (pred and target 4 B; counts, bad_targets and unpredicted 8 B)");
    return MDIL_SIGNIF_ERR_INVALID;
  }

  const int P = H * W;                               // <= 2^30
  const long long per_image = ((long long)P + kUnit - 1) / kUnit, units = per_image * N;
  const int mode = (P & 15) == 0 && !misaligned(pred, 15) && !misaligned(target, 15) ? 2 : (P & 3) == 0 ? 1 : 0;
  const int row_stride = G * 3 * nc;
  unsigned long long* rows = reinterpret_cast<unsigned long long*>(counts) + (first_image * G + g) * 3 * nc;
  const auto kernel = mode == 2 ? signif_count_kernel<2> : mode == 1 ? signif_count_kernel<1> : signif_count_kernel<0>;
  hipLaunchKernelGGL(kernel, dim3(bounded_grid(units, 1, kMaxCountBlocks)), dim3(kWG), 0, (hipStream_t)stream, pred,
                     target, units, per_image, P, nc, ignore_index, rows, row_stride,
                     reinterpret_cast<unsigned long long*>(bad_targets),
                     reinterpret_cast<unsigned long long*>(unpredicted));
  return launched(fn) ? MDIL_SIGNIF_OK : MDIL_SIGNIF_ERR_LAUNCH;
}

API int mdil_signif_resample(const long long* counts, long long M, int G, int nc, int ignore_index, int mode,
                             long long first_replicate, long long B, unsigned long long seed, long long* sums,
                             double* miou, double* iou, unsigned int* empty, void* stream) {
  constexpr char fn[] = "signif_resample";
  if (!counts || !miou) {
    set_error("signif_resample: bad argument (counts %p miou %p)", (const void*)counts, (void*)miou);
    return MDIL_SIGNIF_ERR_INVALID;
  }
  if (!classes_ok(fn, nc, MDIL_SIGNIF_MIN_CLASSES, MDIL_SIGNIF_MAX_CLASSES) || !table_ok(fn, M, G))
    return MDIL_SIGNIF_ERR_INVALID;
  if (!ignore_ok(fn, ignore_index)) return MDIL_SIGNIF_ERR_INVALID;
  if (ignore_index >= 0 && ignore_index < nc - 1) {
    set_error("signif_resample: ignore_index=%d: the ignore class must be the last one, %d, or outside [0, %d)",
              ignore_index, nc - 1, nc);
    return MDIL_SIGNIF_ERR_INVALID;
  }
  if (mode != MDIL_SIGNIF_BOOTSTRAP && mode != MDIL_SIGNIF_JACKKNIFE && mode != MDIL_SIGNIF_SWAP) {
    set_error("signif_resample: mode=%d is none of bootstrap (0), jackknife (1), swap (2)", mode);
    return MDIL_SIGNIF_ERR_INVALID;
  }
  if (mode == MDIL_SIGNIF_SWAP && G != 2) {
    set_error("signif_resample: the swap mode exchanges two predictors: it needs G=2 (got G=%d)", G);
    return MDIL_SIGNIF_ERR_INVALID;
  }
  if (first_replicate < 0 || B < 1 || B > MDIL_SIGNIF_MAX_REPLICATES ||
      first_replicate > MDIL_SIGNIF_MAX_REPLICATES - B) {
    set_error("signif_resample: replicates first_replicate=%lld, B=%lld outside 0 <= first, 1 <= B, first + B <= 2^32",
              first_replicate, B);
    return MDIL_SIGNIF_ERR_INVALID;
  }
  if (mode == MDIL_SIGNIF_JACKKNIFE && first_replicate + B > M) {
    set_error("signif_resample: the jackknife has M=%lld replicates (first_replicate=%lld, B=%lld)", M,
              first_replicate, B);
    return MDIL_SIGNIF_ERR_INVALID;
  }
  if (misaligned(counts, 7) || misaligned(sums, 7) || misaligned(miou, 7) || misaligned(iou, 7) ||
      misaligned(empty, 3)) {
    set_error("signif_resample: alignment (counts, sums, miou and iou 8 B; empty 4 B)");
    return MDIL_SIGNIF_ERR_INVALID;
  }

  ResampleArgs a;
  a.counts = counts, a.sums = sums, a.miou = miou, a.iou = iou, a.empty = empty;
  a.seed = seed, a.first = (unsigned long long)first_replicate, a.B = B;
  a.M = (int)M, a.G = G, a.nc = nc, a.k = ignore_index == nc - 1 ? nc - 1 : nc;
  hipStream_t s = (hipStream_t)stream;
  if (mode == MDIL_SIGNIF_BOOTSTRAP && M * 3 * nc <= kLdsEntries) {
    const size_t lds = (size_t)M * 3 * nc * sizeof(uint32_t);
    const auto kernel = 3 * nc > 64 ? signif_bootstrap_lds_kernel<true> : signif_bootstrap_lds_kernel<false>;
    if (lds > 48 * 1024) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) {
        set_error("signif_resample: %zu bytes of LDS refused: %s", lds, hipGetErrorString(e));
        return MDIL_SIGNIF_ERR_LAUNCH;
      }
    }
    hipLaunchKernelGGL(kernel, dim3(bounded_grid(B, kLdsWaves, kLdsBlocks / G), G), dim3(kLdsWG), lds, s, a);
    return launched(fn) ? MDIL_SIGNIF_OK : MDIL_SIGNIF_ERR_LAUNCH;
  }
  const int nch = (G * 3 * nc + 63) >> 6;
  void (*kernel)(const ResampleArgs);
  if (mode == MDIL_SIGNIF_BOOTSTRAP)
    kernel = nch == 1 ? signif_resample_kernel<MDIL_SIGNIF_BOOTSTRAP, 1>
                      : nch == 2 ? signif_resample_kernel<MDIL_SIGNIF_BOOTSTRAP, 2>
                                 : signif_resample_kernel<MDIL_SIGNIF_BOOTSTRAP, 3>;
  else if (mode == MDIL_SIGNIF_SWAP)
    kernel = nch == 1 ? signif_resample_kernel<MDIL_SIGNIF_SWAP, 1>
                      : nch == 2 ? signif_resample_kernel<MDIL_SIGNIF_SWAP, 2> : signif_resample_kernel<MDIL_SIGNIF_SWAP, 3>;
  else
    kernel = nch == 1 ? signif_resample_kernel<MDIL_SIGNIF_JACKKNIFE, 1>
                      : nch == 2 ? signif_resample_kernel<MDIL_SIGNIF_JACKKNIFE, 2>
                                 : signif_resample_kernel<MDIL_SIGNIF_JACKKNIFE, 3>;
  const int cap = mode == MDIL_SIGNIF_JACKKNIFE ? kMaxJackknifeBlocks : kMaxResampleBlocks;
  hipLaunchKernelGGL(kernel, dim3(bounded_grid(B, kWaves, cap)), dim3(kWG), 0, s, a);
  return launched(fn) ? MDIL_SIGNIF_OK : MDIL_SIGNIF_ERR_LAUNCH;
}
