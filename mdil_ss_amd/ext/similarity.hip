// libmdil_similarity.so: first and second moments of paired feature rows with labels (gfx950).
//
// A row contributes z^T z with z = [onehot(label) | x - pivot_x | y - pivot_y].  The columns of z
// are cut into groups of 16 (1-2 one-hot groups H, up to 8 of X, up to 8 of Y) and only these
// 16 x 16 tiles of z^T z are formed: H x X and H x Y (the class sums), the upper tiles of X x X and
// Y x Y, all of X x Y -- 168 tiles at 128 + 128 channels, 7 at 16 + 16.  The class counts are an
// integer histogram of the labels.
//
//   moments   a work-group takes one chunk of rows.  It stages RS rows of z at a time in LDS
//             (labels first, then the one-hot columns, then x and y with the pivot subtracted,
//             whole rows read as one contiguous span; rows past the end, rows with a label >= nc
//             and channels past cx / cy are zeros, which is all the padding the contraction needs)
//             and its four waves run v_mfma_f32_16x16x4_f32 down the rows: lane l reads
//             z[row 4 j + (l >> 4)][16 g + (l & 15)] as the A operand of group g or the B operand
//             alike, 4 rows x 64 B, conflict-free because the row stride is an odd multiple of 16
//             floats.  A tile's accumulator is one exact fp32 fma chain in row order.
//               many tiles (> 16): the tiles are dealt out to S work-groups x 4 waves x <= 16; the
//               wave's chain covers the chunk, <= 1024 rows.
//               few tiles (<= 16): every wave holds all tiles and takes every fourth 4-row step,
//               so a work-group's chunk is four chains of <= 1024 rows.
//             The accumulators go to the workspace as they lie in the registers.
//   reduce    per tile entry, the chains' partials are added in fp64 -- 32 interleaved
//             sequences, then those in order -- and added to their place (for an off-diagonal tile of
//             X x X / Y x Y, both places) in `state`; one more work-group sums the histograms.
//
// No float atomics anywhere; the LDS histogram uses integer atomics, whose result has no order.
#include "../../include/mdil_similarity.h"

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#define API extern "C" __attribute__((visibility("default")))

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

thread_local char g_err[512] = "";

__attribute__((format(printf, 1, 2))) void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

bool launched(const char* fn) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return true;
  set_error("%s: launch failed: %s", fn, hipGetErrorString(e));
  return false;
}

constexpr int kWG = 256;                       // 4 wavefronts of 64 lanes
constexpr int kWaveTiles = 16;                 // accumulator tiles a wave holds at most
constexpr int kMaxStageRows = 256;
constexpr int kStageBytes = 40960;             // LDS for the staged rows: three work-groups per CU
constexpr int kTargetGroups = 512;             // moments work-groups aimed at: 2 per CU
constexpr int kHist = MDIL_SIM_MAX_CLASSES + 1;   // the classes and `skipped`
constexpr int kNoClass = 255;
constexpr int kSeq = 32;                       // interleaved fp64 sequences of the reduction
constexpr int kRB = 32 * kSeq;                 // threads of a reduction work-group: 32 tile entries x kSeq

static_assert(MDIL_SIM_CHAIN <= 1024 && MDIL_SIM_CHAIN % 4 == 0, "chain length");

struct Plan {
  int gh, gx, gy;                              // 16-column groups of the one-hot part, of x, of y
  int tiles;                                   // 16 x 16 tiles formed
  int ksplit;                                  // 1: few tiles, the waves split the rows
  int S;                                       // work-groups a chunk's tiles are dealt out to
  int chunk, stage, stride;                    // rows per work-group, rows per LDS stage, floats per staged row
  int nchunks, nslots;                         // slots: partial tile sets in the workspace
  size_t part_off, bytes;                      // workspace: i32 [nchunks][kHist] | f32 [nslots][tiles][256]
};

inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

Plan make_plan(long long rows, int cx, int cy, int nc) {
  Plan P;
  P.gh = (nc + 15) / 16;
  P.gx = (cx + 15) / 16;
  P.gy = (cy + 15) / 16;
  P.tiles = P.gh * (P.gx + P.gy) + P.gx * (P.gx + 1) / 2 + P.gy * (P.gy + 1) / 2 + P.gx * P.gy;
  P.ksplit = P.tiles <= kWaveTiles;
  P.S = P.ksplit ? 1 : (P.tiles + 4 * kWaveTiles - 1) / (4 * kWaveTiles);
  const int waves = P.ksplit ? 4 : 1;          // chains per chunk
  long long c = ceil_div(rows * P.S, kTargetGroups);
  c = (c + 15) / 16 * 16;
  const long long lo = 64 * waves, hi = (long long)MDIL_SIM_CHAIN * waves;
  P.chunk = (int)(c < lo ? lo : c > hi ? hi : c);
  const int groups = P.gh + P.gx + P.gy;
  P.stride = 16 * (groups | 1);                // an odd multiple of 16 floats
  int rs = kStageBytes / (P.stride * 4) / 16 * 16;
  if (rs > kMaxStageRows) rs = kMaxStageRows;
  if (rs > P.chunk) rs = P.chunk;
  P.stage = rs;
  P.nchunks = (int)ceil_div(rows, P.chunk);
  P.nslots = P.nchunks * waves;
  P.part_off = ((size_t)P.nchunks * kHist * 4 + 15) & ~(size_t)15;
  P.bytes = P.part_off + (size_t)P.nslots * P.tiles * 256 * 4;
  return P;
}

// Tile t -> its two column groups (ga <= gb), in the order H x X, H x Y, X x X upper, Y x Y upper, X x Y.
__host__ __device__ inline void tile_groups(int t, int gh, int gx, int gy, int& ga, int& gb) {
  int n = gh * gx;
  if (t < n) { ga = t / gx; gb = gh + t % gx; return; }
  t -= n;
  n = gh * gy;
  if (t < n) { ga = t / gy; gb = gh + gx + t % gy; return; }
  t -= n;
  for (int a = 0; a < gx; ++a) {
    if (t < gx - a) { ga = gh + a; gb = gh + a + t; return; }
    t -= gx - a;
  }
  for (int a = 0; a < gy; ++a) {
    if (t < gy - a) { ga = gh + gx + a; gb = gh + gx + a + t; return; }
    t -= gy - a;
  }
  ga = gh + t / gy;                            // only reached with gy > 0
  gb = gh + gx + t % gy;
}

// rows [0, sp) x 16 g columns of the stage from `src` (f32 [..][c], this stage's first row) minus the
// pivot; zeros for rows without a class and for channels >= c.
template <bool VEC>
__device__ __forceinline__ void stage_features(float* __restrict__ dst, int stride, const float* __restrict__ src,
                                               int c, int g, const float* __restrict__ piv,
                                               const int* __restrict__ lab, int sp) {
  if (VEC) {
    const int q = g * 4;
    for (int e = threadIdx.x; e < sp * q; e += kWG) {
      const int r = e / q, ch = (e - r * q) * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (lab[r] != kNoClass && ch < c) {
        v = *reinterpret_cast<const f32x4*>(src + (size_t)r * c + ch);
        v -= *reinterpret_cast<const f32x4*>(piv + ch);
      }
      *reinterpret_cast<f32x4*>(dst + r * stride + ch) = v;
    }
  } else {
    const int q = g * 16;
    for (int e = threadIdx.x; e < sp * q; e += kWG) {
      const int r = e / q, ch = e - r * q;
      dst[r * stride + ch] = (lab[r] != kNoClass && ch < c) ? src[(size_t)r * c + ch] - piv[ch] : 0.f;
    }
  }
}

// VEC: cx and cy are multiples of 4, so every row of x and y is 16-byte aligned.  NT: the
// accumulator tiles of a wave, a compile-time count so that the LDS reads and the MFMAs of a step
// carry no branch between them; a wave with fewer tiles forms group 0 x group 0 in the slots left over
// and stores nothing from them.
template <bool VEC, int NT>
__global__ __launch_bounds__(kWG) void moments_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                      const unsigned char* __restrict__ labels, long long rows,
                                                      int cx, int cy, int nc, const float* __restrict__ pivot_x,
                                                      const float* __restrict__ pivot_y, Plan P,
                                                      int* __restrict__ counts, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float Zs[];             // [P.stage][P.stride]
  __shared__ __attribute__((aligned(16))) float piv[MDIL_SIM_MAX_CX + MDIL_SIM_MAX_CY];
  __shared__ int lab[kMaxStageRows];
  __shared__ int hist[kHist];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int chunk = blockIdx.x, split = blockIdx.y;
  const long long c0 = (long long)chunk * P.chunk;
  const int cn = (int)(rows - c0 < P.chunk ? rows - c0 : P.chunk);
  const int stride = P.stride;

  // the wave's tiles: LDS column offsets of the two operands
  int oa[NT], ob[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    const int id = P.ksplit ? k : (k * 4 + wave) * P.S + split;
    int ga = 0, gb = 0;
    if (id < P.tiles) tile_groups(id, P.gh, P.gx, P.gy, ga, gb);
    oa[k] = __builtin_amdgcn_readfirstlane(ga * 16);
    ob[k] = __builtin_amdgcn_readfirstlane(gb * 16);
  }
  f32x4 acc[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (t < kHist) hist[t] = 0;
  if (t < MDIL_SIM_MAX_CX) piv[t] = t < cx ? pivot_x[t] : 0.f;
  else if (t < MDIL_SIM_MAX_CX + MDIL_SIM_MAX_CY) piv[t] = t - MDIL_SIM_MAX_CX < cy ? pivot_y[t - MDIL_SIM_MAX_CX] : 0.f;

  const int hw = P.gh * 16, hshift = P.gh == 2 ? 5 : 4;
  const int j0 = P.ksplit ? wave : 0, jstep = P.ksplit ? 4 : 1;
  for (int s0 = 0; s0 < cn; s0 += P.stage) {               // uniform over the work-group
    const int sn = cn - s0 < P.stage ? cn - s0 : P.stage;  // rows of this stage
    const int sp = (sn + 3) & ~3;                          // ... rounded up to whole 4-row steps (<= P.stage)
    __syncthreads();
    for (int r = t; r < sp; r += kWG) {
      int l = kNoClass;
      if (r < sn) {
        l = labels ? (int)labels[c0 + s0 + r] : 0;
        if (l >= nc) l = kNoClass;
        if (split == 0) atomicAdd(&hist[l == kNoClass ? MDIL_SIM_MAX_CLASSES : l], 1);
      }
      lab[r] = l;
    }
    __syncthreads();
    for (int e = t; e < sp * hw; e += kWG) {
      const int r = e >> hshift, c = e & (hw - 1);
      Zs[r * stride + c] = lab[r] == c ? 1.f : 0.f;
    }
    stage_features<VEC>(Zs + hw, stride, x + (size_t)(c0 + s0) * cx, cx, P.gx, piv, lab, sp);
    if (cy > 0)
      stage_features<VEC>(Zs + hw + P.gx * 16, stride, y + (size_t)(c0 + s0) * cy, cy, P.gy, piv + MDIL_SIM_MAX_CX,
                          lab, sp);
    __syncthreads();
    const int steps = sp >> 2;
    for (int j = j0; j < steps; j += jstep) {
      const float* zr = Zs + (4 * j + (lane >> 4)) * stride + (lane & 15);
      float a[NT], b[NT];
#pragma unroll
      for (int k = 0; k < NT; ++k) {
        a[k] = zr[oa[k]];
        b[k] = zr[ob[k]];
      }
#pragma unroll
      for (int k = 0; k < NT; ++k) acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[k], b[k], acc[k], 0, 0, 0);
    }
  }

  const size_t slot = P.ksplit ? (size_t)chunk * 4 + wave : (size_t)chunk;
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    const int id = P.ksplit ? k : (k * 4 + wave) * P.S + split;
    if (id < P.tiles) {
      float* dst = part + (slot * P.tiles + id) * 256 + lane;
#pragma unroll
      for (int i = 0; i < 4; ++i) dst[i * 64] = acc[k][i];
    }
  }
  __syncthreads();
  if (split == 0 && t < kHist) counts[(size_t)chunk * kHist + t] = hist[t];
}

// Work-groups [0, 8 tiles): 32 entries of a tile each; the last work-group: the histograms.
__global__ __launch_bounds__(kRB) void reduce_kernel(const float* __restrict__ part, const int* __restrict__ counts,
                                                     Plan P, int cx, int cy, int nc, double* __restrict__ state) {
  __shared__ double buf[kSeq][32];
  __shared__ long long ibuf[kRB];
  const int t = threadIdx.x;
  double* n = state;
  double* sx = n + nc + 1;
  double* sy = sx + (size_t)nc * cx;
  double* gxx = sy + (size_t)nc * cy;
  double* gyy = gxx + (size_t)cx * cx;
  double* gxy = gyy + (size_t)cy * cy;
  if ((int)blockIdx.x == P.tiles * 8) {
    for (int c = 0; c < kHist; ++c) {
      long long a = 0;
      for (int k = t; k < P.nchunks; k += kRB) a += counts[(size_t)k * kHist + c];
      ibuf[t] = a;
      __syncthreads();
      for (int s = kRB / 2; s > 0; s >>= 1) {
        if (t < s) ibuf[t] += ibuf[t + s];
        __syncthreads();
      }
      if (t == 0) {
        if (c < nc) n[c] += (double)ibuf[0];
        else if (c == MDIL_SIM_MAX_CLASSES) n[nc] += (double)ibuf[0];
      }
      __syncthreads();
    }
    return;
  }
  const int tile = blockIdx.x >> 3, el = (blockIdx.x & 7) * 32 + (t & 31), q = t >> 5;
  double a = 0.0;
#pragma unroll 4
  for (int s = q; s < P.nslots; s += kSeq) a += (double)part[((size_t)s * P.tiles + tile) * 256 + el];
  buf[q][t & 31] = a;
  __syncthreads();
  if (q != 0) return;
  const int e = t & 31;
  double v = 0.0;
  for (int k = 0; k < kSeq; ++k) v += buf[k][e];          // sequence order
  // register i of lane l holds row 4 (l >> 4) + i, column l & 15 of the tile
  const int i = el >> 6, l = el & 63;
  int ga, gb;
  tile_groups(tile, P.gh, P.gx, P.gy, ga, gb);
  const int ra = ga * 16 + 4 * (l >> 4) + i, rb = gb * 16 + (l & 15);     // columns of z
  const int x0 = P.gh * 16, y0 = x0 + P.gx * 16;
  const bool b_is_y = rb >= y0;
  const int b = b_is_y ? rb - y0 : rb - x0;
  if (b >= (b_is_y ? cy : cx)) return;
  if (ra < x0) {                                           // class sums
    if (ra < nc) (b_is_y ? sy[(size_t)ra * cy + b] : sx[(size_t)ra * cx + b]) += v;
  } else if (ra < y0) {
    const int a_ = ra - x0;
    if (a_ >= cx) return;
    if (b_is_y) {
      gxy[(size_t)a_ * cy + b] += v;
    } else {
      gxx[(size_t)a_ * cx + b] += v;
      if (ga != gb) gxx[(size_t)b * cx + a_] += v;        // the mirror tile is not formed
    }
  } else {
    const int a_ = ra - y0;
    if (a_ >= cy) return;
    gyy[(size_t)a_ * cy + b] += v;
    if (ga != gb) gyy[(size_t)b * cy + a_] += v;
  }
}

bool sizes_ok(const char* fn, long long rows, int cx, int cy, int nc, bool say) {
  const char* what = nullptr;
  long long v = 0, lo = 0, hi = 0;
  if (cx < 1 || cx > MDIL_SIM_MAX_CX) { what = "cx"; v = cx; lo = 1; hi = MDIL_SIM_MAX_CX; }
  else if (cy < 0 || cy > MDIL_SIM_MAX_CY) { what = "cy"; v = cy; lo = 0; hi = MDIL_SIM_MAX_CY; }
  else if (nc < 1 || nc > MDIL_SIM_MAX_CLASSES) { what = "nc"; v = nc; lo = 1; hi = MDIL_SIM_MAX_CLASSES; }
  else if (rows < 1 || rows > MDIL_SIM_MAX_ROWS) { what = "rows"; v = rows; lo = 1; hi = MDIL_SIM_MAX_ROWS; }
  if (!what) return true;
  if (say) set_error("%s: %s=%lld outside [%lld, %lld]", fn, what, v, lo, hi);
  return false;
}

size_t state_doubles(int cx, int cy, int nc) {
  return (size_t)nc + 1 + (size_t)nc * (cx + cy) + (size_t)cx * cx + (size_t)cy * cy + (size_t)cx * cy;
}

bool overlap(const void* a, size_t an, const void* b, size_t bn) {
  return a && b && (uintptr_t)a < (uintptr_t)b + bn && (uintptr_t)b < (uintptr_t)a + an;
}

}  // namespace

API int mdil_sim_version(void) { return 100; }
API const char* mdil_sim_last_error(void) { return g_err; }

API long long mdil_sim_state_bytes(int cx, int cy, int nc) {
  if (!sizes_ok("sim_state_bytes", 1, cx, cy, nc, false)) return -1;
  return (long long)(state_doubles(cx, cy, nc) * 8);
}

API long long mdil_sim_workspace_bytes(long long rows, int cx, int cy, int nc) {
  if (!sizes_ok("sim_workspace_bytes", rows, cx, cy, nc, false)) return -1;
  return (long long)make_plan(rows, cx, cy, nc).bytes;
}

API int mdil_sim_accumulate(const float* x, const float* y, const unsigned char* labels, long long rows, int cx,
                            int cy, int nc, const float* pivot_x, const float* pivot_y, double* state,
                            void* workspace, void* stream) {
  const char* fn = "sim_accumulate";
  if (!sizes_ok(fn, rows, cx, cy, nc, true)) return MDIL_SIM_ERR_INVALID;
  if (!x || !pivot_x || !state || !workspace) {
    set_error("%s: bad argument (x %p pivot_x %p state %p workspace %p)", fn, (const void*)x, (const void*)pivot_x,
              (void*)state, workspace);
    return MDIL_SIM_ERR_INVALID;
  }
  if ((y != nullptr) != (cy > 0) || (pivot_y != nullptr) != (cy > 0)) {
    set_error("%s: y and pivot_y must be NULL exactly when cy == 0 (y %p pivot_y %p cy=%d)", fn, (const void*)y,
              (const void*)pivot_y, cy);
    return MDIL_SIM_ERR_INVALID;
  }
  if (!labels && nc != 1) {
    set_error("%s: labels NULL needs nc == 1 (nc=%d)", fn, nc);
    return MDIL_SIM_ERR_INVALID;
  }
  if (((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)state & 15) || ((uintptr_t)workspace & 15) ||
      ((uintptr_t)pivot_x & 3) || ((uintptr_t)pivot_y & 3)) {
    set_error("%s: alignment (x, y, state and workspace 16 B; pivot_x and pivot_y 4 B)", fn);
    return MDIL_SIM_ERR_INVALID;
  }
  const Plan P = make_plan(rows, cx, cy, nc);
  const size_t sb = state_doubles(cx, cy, nc) * 8;
  const struct { const void* p; size_t n; const char* name; } in[] = {
      {x, (size_t)rows * cx * 4, "x"}, {y, (size_t)rows * cy * 4, "y"}, {labels, (size_t)rows, "labels"},
      {pivot_x, (size_t)cx * 4, "pivot_x"}, {pivot_y, (size_t)cy * 4, "pivot_y"}};
  for (const auto& a : in) {
    if (overlap(state, sb, a.p, a.n) || overlap(workspace, P.bytes, a.p, a.n)) {
      set_error("%s: state or workspace overlap %s", fn, a.name);
      return MDIL_SIM_ERR_INVALID;
    }
  }
  if (overlap(state, sb, workspace, P.bytes)) {
    set_error("%s: state and workspace overlap", fn);
    return MDIL_SIM_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  int* counts = (int*)workspace;
  float* part = (float*)((char*)workspace + P.part_off);
  const dim3 grid(P.nchunks, P.S);
  const size_t lds = (size_t)P.stage * P.stride * 4;
  // tiles of the busiest wave, rounded up to the next instantiation
  const int per_wave = P.ksplit ? P.tiles : (P.tiles + 4 * P.S - 1) / (4 * P.S);
  const bool vec = cx % 4 == 0 && cy % 4 == 0;
#define MDIL_SIM_LAUNCH(V, NT)                                                                                  \
  hipLaunchKernelGGL((moments_kernel<V, NT>), grid, dim3(kWG), lds, st, x, y, labels, rows, cx, cy, nc, pivot_x, \
                     pivot_y, P, counts, part)
#define MDIL_SIM_CASE(NT)                                                 \
  if (per_wave <= NT) {                                                   \
    if (vec) MDIL_SIM_LAUNCH(true, NT); else MDIL_SIM_LAUNCH(false, NT);  \
  } else
  MDIL_SIM_CASE(2) MDIL_SIM_CASE(4) MDIL_SIM_CASE(6) MDIL_SIM_CASE(8) MDIL_SIM_CASE(10) MDIL_SIM_CASE(12)
  MDIL_SIM_CASE(14) MDIL_SIM_CASE(16) {
    set_error("%s: %d tiles per wave (at most %d)", fn, per_wave, kWaveTiles);
    return MDIL_SIM_ERR_INVALID;
  }
#undef MDIL_SIM_CASE
#undef MDIL_SIM_LAUNCH
  if (!launched(fn)) return MDIL_SIM_ERR_LAUNCH;
  hipLaunchKernelGGL(reduce_kernel, dim3(P.tiles * 8 + 1), dim3(kRB), 0, st, part, counts, P, cx, cy, nc, state);
  return launched(fn) ? MDIL_SIM_OK : MDIL_SIM_ERR_LAUNCH;
}
