// libmdil_boundary.so: the distance of every pixel of two label maps to its region's contour,
// binned by band widths, and the boundary-IoU / trimap counters, in two launches (gfx950).
//
//   d(L, p) = Chebyshev distance from p to the nearest pixel of another label or outside the image
//           = min over r of max(|r|, t(r)),   t(r) = 0 where row y + r is outside or L[y+r][x] != L[y][x],
//                                             t(r) = hx(y + r, x) otherwise
//   hx(y,x) = min(x - s + 1, e - x + 1),      [s, e] the horizontal run of equal labels around x
// (include/mdil_boundary.h has the counters).  Integers only: nothing is rounded, every output is
// exact and the same on every run.  Only min(d, cap + 1) is needed, cap = the largest width <= 128,
// so one byte holds a distance and every hx is stored capped at cap + 1.
//
// Row pass (boundary_rows_kernel).  One wavefront owns a row of one map and walks it in chunks of
// 256 pixels, four per lane as one dword.  Left to right, s is the running maximum of the positions
// where a run starts: a max-scan over the lanes (6 shuffle steps), carried from chunk to chunk;
// min(x - s + 1, cap + 1) goes to the workspace.  Right to left, e is the running minimum of the
// positions where a run ends, the same scan mirrored; each lane reads back the bytes it wrote itself
// and stores the minimum of both.  Pixels past W (the W % 4 tail, the last chunk) start no run and
// end none, and W - 1 always ends one, so they reach no pixel inside the row.
//
// Column pass (boundary_count_kernel).  A lane owns four horizontally adjacent pixels and, for each
// map, walks r = 1, 2, ... up and down while r is below the best distance of any of its four pixels
// (max(r, t) >= r cannot improve a best <= r).  Lanes run along x, so every step reads one dword of
// labels and one of hx per direction, coalesced over the wave, from rows that the neighbouring
// work-groups have just read: L2 traffic, at most 2 * cap steps.  A row outside the image gives t = 0
// and ends the walk, so the images of a batch never see each other.  Rows that are no multiple of
// four pixels wide are read and written by bytes.
//
// Counters.  Each work-group counts into 32-bit tables in LDS (dynamic: nb * nc * nc for the
// confusion, three nc * nb histograms, two bad counters, at most 40,200 bytes) with LDS atomics and
// adds its non-zero entries to the 64-bit counters with global atomic adds after its grid-stride
// loop.  The grid is bounded at 2048 work-groups and a call at 2^40 pixels, so a work-group counts
// at most 2^31 pixels and no 32-bit counter wraps.
#include "../../include/mdil_boundary.h"
#include "head_common.h"

namespace {

constexpr int kWG = 256;                             // 4 wavefronts of 64 lanes
constexpr int kWaves = kWG / 64;
constexpr int kChunk = 256;                          // pixels a wavefront covers per step of the row pass
constexpr int kMaxWidths = MDIL_BOUNDARY_MAX_WIDTHS;
constexpr int kMaxBlocks = 2048;                     // beyond that the loops stride
constexpr int kNone = 0x7fffffff;
constexpr char kFn[] = "boundary_count";

struct Widths {
  int w[kMaxWidths];
};

// Four pixels of a row starting at column x0 (a multiple of 4), one per byte; 0 past W.
__device__ __forceinline__ uint32_t load4(const unsigned char* row, int x0, int W, bool packed) {
  if (packed) return x0 < W ? *reinterpret_cast<const uint32_t*>(row + x0) : 0u;
  uint32_t v = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (x0 + j < W) v |= (uint32_t)row[x0 + j] << (8 * j);
  return v;
}

__device__ __forceinline__ void store4(unsigned char* row, int x0, int W, bool packed, uint32_t v) {
  if (packed) {
    if (x0 < W) *reinterpret_cast<uint32_t*>(row + x0) = v;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (x0 + j < W) row[x0 + j] = (unsigned char)(v >> (8 * j));
}

__device__ __forceinline__ int byte_of(uint32_t v, int j) { return (int)((v >> (8 * j)) & 0xffu); }

// ---------------------------------------------------------------------------------- row pass
// rows = N * H rows per map; job < rows: pred, else target.  ws: [2][N][H][W] bytes.
__global__ __launch_bounds__(kWG) void boundary_rows_kernel(const unsigned char* __restrict__ pred,
                                                            const unsigned char* __restrict__ target,
                                                            long long rows, int W, int lim,
                                                            unsigned char* ws) {
  const int lane = threadIdx.x & 63;
  const bool packed = (W & 3) == 0;
  const int nchunks = (W + kChunk - 1) / kChunk;
  // wave-uniform loop: every shuffle below runs with all 64 lanes
  for (long long job = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); job < 2 * rows;
       job += (long long)gridDim.x * kWaves) {
    const bool second = job >= rows;
    const long long row = second ? job - rows : job;
    const unsigned char* __restrict__ L = (second ? target : pred) + row * W;
    unsigned char* O = ws + job * W;

    int carry = -1;                                  // the last run start so far (x = 0 starts one)
    for (int c = 0; c < nchunks; ++c) {
      const int x0 = c * kChunk + lane * 4;
      const uint32_t v = load4(L, x0, W, packed);
      int before = (x0 > 0 && x0 <= W) ? (int)L[x0 - 1] : -1;
      bool brk[4];
      int m = -1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int b = byte_of(v, j);
        brk[j] = x0 + j < W && b != before;          // before = -1 at x = 0
        before = b;
        m = brk[j] ? x0 + j : m;
      }
      int inc = m;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off, 64);
        inc = lane >= off ? max(inc, t) : inc;
      }
      inc = max(inc, carry);
      const int up = __shfl_up(inc, 1, 64);
      int s = lane ? up : carry;
      carry = __shfl(inc, 63, 64);
      uint32_t out = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s = brk[j] ? x0 + j : s;
        out |= (uint32_t)min(x0 + j - s + 1, lim) << (8 * j);   // past W: never stored
      }
      store4(O, x0, W, packed, out);
    }

    carry = kNone;                                   // the first run end so far, from the right
    for (int c = nchunks - 1; c >= 0; --c) {
      const int x0 = c * kChunk + lane * 4;
      const uint32_t v = load4(L, x0, W, packed);
      const uint32_t left = load4(O, x0, W, packed);  // this lane's own bytes of the sweep above
      int after = x0 + 4 < W ? (int)L[x0 + 4] : -1;
      bool end[4];
      int m = kNone;
#pragma unroll
      for (int j = 3; j >= 0; --j) {
        const int b = byte_of(v, j);
        end[j] = x0 + j < W && (x0 + j == W - 1 || b != after);
        after = b;
        m = end[j] ? x0 + j : m;
      }
      int inc = m;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_down(inc, off, 64);
        inc = lane + off < 64 ? min(inc, t) : inc;
      }
      inc = min(inc, carry);
      const int down = __shfl_down(inc, 1, 64);
      int e = lane < 63 ? down : carry;
      carry = __shfl(inc, 0, 64);
      uint32_t out = 0;
#pragma unroll
      for (int j = 3; j >= 0; --j) {
        e = end[j] ? x0 + j : e;
        const int right = x0 + j < W ? min(e - (x0 + j) + 1, lim) : 0;
        out |= (uint32_t)min(right, byte_of(left, j)) << (8 * j);
      }
      store4(O, x0, W, packed, out);
    }
  }
}

// ------------------------------------------------------------------------------- column pass
// min(d, lim) of the lane's four pixels of row y of one image: L and Hx point at the image's first
// row (labels, capped hx), lab holds the four labels.  Bytes past W come out as 0.
__device__ __forceinline__ uint32_t walk(const unsigned char* __restrict__ L, const unsigned char* __restrict__ Hx,
                                         int y, int x0, int H, int W, bool packed, uint32_t lab) {
  const uint32_t own = load4(Hx + (long long)y * W, x0, W, packed);
  int best[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) best[j] = byte_of(own, j);
  int most = max(max(best[0], best[1]), max(best[2], best[3]));
  for (int r = 1; r < most; ++r) {
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
      const int yy = dir ? y + r : y - r;
      uint32_t l = 0, h = 0;
      const bool inside = yy >= 0 && yy < H;
      if (inside) {
        l = load4(L + (long long)yy * W, x0, W, packed);
        h = load4(Hx + (long long)yy * W, x0, W, packed);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int t = inside && byte_of(l, j) == byte_of(lab, j) ? byte_of(h, j) : 0;
        best[j] = min(best[j], max(r, t));
      }
    }
    most = max(max(best[0], best[1]), max(best[2], best[3]));
  }
  return (uint32_t)best[0] | (uint32_t)best[1] << 8 | (uint32_t)best[2] << 16 | (uint32_t)best[3] << 24;
}

struct CountArgs {
  const unsigned char* pred;
  const unsigned char* target;
  const unsigned char* hx_pred;
  const unsigned char* hx_target;
  unsigned char* dist_pred;
  unsigned char* dist_target;
  unsigned long long* target_hist;
  unsigned long long* pred_hist;
  unsigned long long* both_hist;
  unsigned long long* confusion;
  unsigned long long* bad_targets;
  unsigned long long* bad_preds;
  long long nitems;                                  // N * H * ceil(W / 4)
  int H, W, nc, nb, ignore_index;
  Widths widths;
};

__global__ __launch_bounds__(kWG) void boundary_count_kernel(const CountArgs p) {
  // [conf nb*nc*nc][target nc*nb][pred nc*nb][both nc*nb][bad_targets][bad_preds]
  extern __shared__ __attribute__((aligned(16))) uint32_t counts[];
  __shared__ unsigned char bin_of[MDIL_BOUNDARY_MAX_WIDTH + 2];       // d in [1, cap + 1] -> bin
  const int nc = p.nc, nb = p.nb, H = p.H, W = p.W;
  const int n_conf = nb * nc * nc, n_hist = nc * nb, n_all = n_conf + 3 * n_hist + 2;
  uint32_t* const conf = counts;
  uint32_t* const th = counts + n_conf;
  uint32_t* const ph = th + n_hist;
  uint32_t* const bh = ph + n_hist;
  uint32_t* const bad = bh + n_hist;
  for (int i = threadIdx.x; i < n_all; i += kWG) counts[i] = 0u;
  const int lim = p.widths.w[nb - 2] + 1;
  for (int d = threadIdx.x; d <= lim; d += kWG) {
    int k = 0;
#pragma unroll
    for (int i = 0; i < kMaxWidths; ++i) k += (i < nb - 1 && p.widths.w[i] < d) ? 1 : 0;
    bin_of[d] = (unsigned char)k;
  }
  __syncthreads();

  const long long G = ((long long)W + 3) >> 2;      // items per row
  const bool packed = (W & 3) == 0;
  for (long long item = (long long)blockIdx.x * kWG + threadIdx.x; item < p.nitems;
       item += (long long)gridDim.x * kWG) {
    const long long r = item / G;                    // n * H + y
    const int x0 = (int)(item - r * G) * 4;
    const long long n = r / H;
    const int y = (int)(r - n * H);
    const long long img = n * H * W, o = r * W;
    const uint32_t lp = load4(p.pred + o, x0, W, packed);
    const uint32_t lt = load4(p.target + o, x0, W, packed);
    const uint32_t dp = walk(p.pred + img, p.hx_pred + img, y, x0, H, W, packed, lp);
    const uint32_t dt = walk(p.target + img, p.hx_target + img, y, x0, H, W, packed, lt);
    if (p.dist_pred) store4(p.dist_pred + o, x0, W, packed, dp);
    if (p.dist_target) store4(p.dist_target + o, x0, W, packed, dt);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (x0 + j >= W) continue;
      const int g = byte_of(lt, j), q = byte_of(lp, j);
      if (g == p.ignore_index) continue;
      if (g >= nc) {
        atomicAdd(&bad[0], 1u);
      } else if (q >= nc) {
        atomicAdd(&bad[1], 1u);
      } else {
        const int a = byte_of(dt, j), b = byte_of(dp, j);
        const int kt = bin_of[a], kp = bin_of[b];
        atomicAdd(&th[g * nb + kt], 1u);
        atomicAdd(&ph[q * nb + kp], 1u);
        if (g == q) atomicAdd(&bh[g * nb + max(kt, kp)], 1u);       // bin() is monotone: bin(max) = max(bin)
        atomicAdd(&conf[(kt * nc + g) * nc + q], 1u);
      }
    }
  }

  __syncthreads();
  for (int i = threadIdx.x; i < n_all; i += kWG) {
    const uint32_t v = counts[i];
    if (!v) continue;
    unsigned long long* dst;
    if (i < n_conf)
      dst = p.confusion + i;
    else if (i < n_conf + n_hist)
      dst = p.target_hist + (i - n_conf);
    else if (i < n_conf + 2 * n_hist)
      dst = p.pred_hist + (i - n_conf - n_hist);
    else if (i < n_conf + 3 * n_hist)
      dst = p.both_hist + (i - n_conf - 2 * n_hist);
    else
      dst = i == n_all - 2 ? p.bad_targets : p.bad_preds;
    atomicAdd(dst, (unsigned long long)v);
  }
}

bool size_ok(int N, int H, int W) {
  return N > 0 && H > 0 && W > 0 && H <= MDIL_BOUNDARY_MAX_SIZE && W <= MDIL_BOUNDARY_MAX_SIZE &&
         (long long)N * H <= MDIL_BOUNDARY_MAX_PIXELS / W;
}

long long workspace_need(int N, int H, int W) { return (2LL * N * H * W + 15) & ~15LL; }

}  // namespace

API int mdil_boundary_version(void) { return 100; }
API const char* mdil_boundary_last_error(void) { return g_err; }

API long long mdil_boundary_workspace_bytes(int N, int H, int W) {
  return size_ok(N, H, W) ? workspace_need(N, H, W) : -1;
}

API int mdil_boundary_count(const unsigned char* pred, const unsigned char* target, int N, int H, int W, int nc,
                            const int* widths, int n_widths, int ignore_index, unsigned char* workspace,
                            long long workspace_bytes, unsigned char* dist_pred, unsigned char* dist_target,
                            long long* target_hist, long long* pred_hist, long long* both_hist,
                            long long* confusion, long long* bad_targets, long long* bad_preds, void* stream) {
  if (!pred || !target || !widths || !target_hist || !pred_hist || !both_hist || !confusion || !bad_targets ||
      !bad_preds || N <= 0 || H <= 0 || W <= 0) {
    set_error("boundary_count: bad argument (pred %p target %p widths %p target_hist %p pred_hist %p both_hist %p "
              "confusion %p bad_targets %p bad_preds %p N %d H %d W %d)",
              (const void*)pred, (const void*)target, (const void*)widths, (void*)target_hist, (void*)pred_hist,
              (void*)both_hist, (void*)confusion, (void*)bad_targets, (void*)bad_preds, N, H, W);
    return MDIL_BOUNDARY_ERR_INVALID;
  }
  if (!classes_ok(kFn, nc, MDIL_BOUNDARY_MIN_CLASSES, MDIL_BOUNDARY_MAX_CLASSES)) return MDIL_BOUNDARY_ERR_INVALID;
  if (H > MDIL_BOUNDARY_MAX_SIZE || W > MDIL_BOUNDARY_MAX_SIZE) {
    set_error("boundary_count: size %d x %d above %d", H, W, MDIL_BOUNDARY_MAX_SIZE);
    return MDIL_BOUNDARY_ERR_INVALID;
  }
  if (!size_ok(N, H, W)) {
    set_error("boundary_count: too large (N %d, maps %d x %d: at most 2^40 pixels)", N, H, W);
    return MDIL_BOUNDARY_ERR_INVALID;
  }
  if (!ignore_ok(kFn, ignore_index)) return MDIL_BOUNDARY_ERR_INVALID;
  if (n_widths < 1 || n_widths > kMaxWidths) {
    set_error("boundary_count: n_widths=%d outside [1, %d]", n_widths, kMaxWidths);
    return MDIL_BOUNDARY_ERR_INVALID;
  }
  Widths wd = {};
  for (int i = 0; i < n_widths; ++i) {
    wd.w[i] = widths[i];
    if (widths[i] < 1 || widths[i] > MDIL_BOUNDARY_MAX_WIDTH || (i && widths[i] <= widths[i - 1])) {
      set_error("boundary_count: widths must be strictly increasing within [1, %d] (widths[%d]=%d)",
                MDIL_BOUNDARY_MAX_WIDTH, i, widths[i]);
      return MDIL_BOUNDARY_ERR_INVALID;
    }
  }
  if (((uintptr_t)pred & 3) || ((uintptr_t)target & 3) || ((uintptr_t)workspace & 3) ||
      ((uintptr_t)dist_pred & 3) || ((uintptr_t)dist_target & 3) || ((uintptr_t)target_hist & 7) ||
      ((uintptr_t)pred_hist & 7) || ((uintptr_t)both_hist & 7) || ((uintptr_t)confusion & 7) ||
      ((uintptr_t)bad_targets & 7) || ((uintptr_t)bad_preds & 7)) {
    set_error("boundary_count: alignment (pred, target, workspace, dist_pred and dist_target 4 B; the counters 8 B)");
    return MDIL_BOUNDARY_ERR_INVALID;
  }
  const long long need = workspace_need(N, H, W);
  if (!workspace || workspace_bytes < need) {
    set_error("boundary_count: needs a workspace of %lld bytes (got %p, %lld bytes)", need, (void*)workspace,
              workspace_bytes);
    return MDIL_BOUNDARY_ERR_INVALID;
  }

  const long long rows = (long long)N * H, plane = rows * W;
  const int lim = wd.w[n_widths - 1] + 1;
  hipLaunchKernelGGL(boundary_rows_kernel, dim3(bounded_grid(2 * rows, kWaves, 4 * kMaxBlocks)), dim3(kWG), 0,
                     (hipStream_t)stream, pred, target, rows, W, lim, workspace);
  if (!launched(kFn)) return MDIL_BOUNDARY_ERR_LAUNCH;

  CountArgs p;
  p.pred = pred, p.target = target, p.hx_pred = workspace, p.hx_target = workspace + plane;
  p.dist_pred = dist_pred, p.dist_target = dist_target;
  p.target_hist = reinterpret_cast<unsigned long long*>(target_hist);
  p.pred_hist = reinterpret_cast<unsigned long long*>(pred_hist);
  p.both_hist = reinterpret_cast<unsigned long long*>(both_hist);
  p.confusion = reinterpret_cast<unsigned long long*>(confusion);
  p.bad_targets = reinterpret_cast<unsigned long long*>(bad_targets);
  p.bad_preds = reinterpret_cast<unsigned long long*>(bad_preds);
  p.nitems = rows * (((long long)W + 3) >> 2);
  p.H = H, p.W = W, p.nc = nc, p.nb = n_widths + 1, p.ignore_index = ignore_index;
  p.widths = wd;
  const int nb = n_widths + 1;
  const size_t lds = (size_t)(nb * nc * nc + 3 * nc * nb + 2) * sizeof(uint32_t);
  hipLaunchKernelGGL(boundary_count_kernel, dim3(bounded_grid(p.nitems, kWG, kMaxBlocks)), dim3(kWG), lds,
                     (hipStream_t)stream, p);
  return launched(kFn) ? MDIL_BOUNDARY_OK : MDIL_BOUNDARY_ERR_LAUNCH;
}
