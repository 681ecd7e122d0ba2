// libmdil_route.so: what a router needs of an image whose domain is not known (gfx950).  Two kernels,
// both with a PER-IMAGE reduction that no other add-on has:
//
//   route_stem   a[n, h, w, 0..12] = bias[c] + sum_{ci,ky,kx} image[n, ci, 2h-1+ky, 2w-1+kx] * w[c][ci][ky][kx]
//                a[n, h, w, 13+ci] = max of image[n, ci, 2h..2h+1, 2w..2w+1]
//                moments[n][c] = (sum a, sum a^2) over the image, fp64
//   route_head   l = output_conv(x), softmax, per pixel conf = p_top, ent = -sum p log p,
//                margin = p_top - p_second;  scores[n] = their sums over the image, fp64
//
// The stem reads the image once (planar fp32, 37.7 MB at 6 x 512 x 1024) and stores the activation only
// when asked; the head never stores the logits.
//
// Layout of both.  A lane owns one position (stem: one output position, 27 taps from the three
// planes, of which a neighbouring lane shares a column through the L1; head: one feature pixel, 16
// channels in registers, the four parities one after the other with calib_head's chain and forms at
// T = 1).  The work-groups are laid out PER IMAGE: image n owns the work-groups n * bpi .. n * bpi + bpi - 1
// with bpi = min(ceil(H W / 256), 256), and work-group j of an image takes the positions
// j * 256 + lane, + bpi * 256, ... of that image.  So which lane adds which value in which order is a
// function of H and W alone -- not of N, not of n.
//
// Sums.  No floating-point atomics.  A lane adds its own values in fp64 in the order it meets them;
// after the loop a fixed xor tree (head_common.h's wave_sum) sums the 64 lanes, the four waves'
// totals are added in wave order, and the work-group stores one row (stem: 32 doubles, head: 3) to
// the caller's workspace at row n * bpi + j.  A second launch, fold_rows below, gives every
// (image, column) one wavefront: lane l adds that image's rows l, l + 64, ... ascending, then the
// tree, and the total is STORED (the outputs are overwritten, not added to).  head_common.h's
// fold_kernel adds all rows of a call into one entry, so it cannot keep the images apart; hence a fold
// of this file's own.  Nothing in that chain sees N or n: image n's numbers are the same bits alone
// and in a batch.
//
// The stem's weights sit in LDS as Wl[tap][c] (tap = ci * 9 + ky * 3 + kx, 16 floats per row): every
// lane of a wave reads the same address (broadcast), four 16-byte reads per tap; the 13 chains advance
// together tap by tap, so each runs over ci, ky, kx ascending.  With padding 1 and even sizes only the
// row above the image (ky = 0 at h = 0) and the column left of it (kx = 0 at w = 0) fall outside; those
// taps are skipped, not multiplied by zero.  A position's 27 loads are issued together, from clamped
// addresses, before the first FMA: 162 VGPRs, three waves per SIMD, no scratch.
#include "../../include/mdil_route.h"
#include "map_common.h"

#include <float.h>

namespace {

constexpr int kWG = 256;                             // 4 wavefronts of 64 lanes
constexpr int kWaves = kWG / 64;
constexpr int kMaxC = MDIL_ROUTE_MAX_CLASSES;
constexpr int kMaxBlocksPerImage = 256;              // beyond 65,536 positions of an image the loop strides
constexpr long long kMaxPixels = 1LL << 38;          // positions of a call
constexpr int kStemOut = MDIL_ROUTE_STEM_CHANNELS, kStemConv = 13, kTaps = 27;
constexpr int kStemCols = 2 * kStemOut, kHeadCols = 3;
constexpr char kStemFn[] = "route_stem", kHeadFn[] = "route_head";

// The second launch of both entry points: out[n * cols + c] = the sum of column c over image n's
// `rows` rows of the workspace.  One wavefront per entry.
__global__ __launch_bounds__(64) void fold_rows(const double* __restrict__ workspace, int rows, int cols,
                                                double* __restrict__ out) {
  const long long n = blockIdx.x / cols;
  const int c = blockIdx.x - (int)n * cols;
  double v = 0.0;
  for (int b = threadIdx.x; b < rows; b += 64) v += workspace[(n * rows + b) * cols + c];
  v = wave_sum(v);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// The end of both main kernels: v[0..COLS) of every lane -> one row of the workspace.  Every lane of
// the work-group calls it.
template <int COLS>
__device__ __forceinline__ void store_row(const double (&v)[COLS], double (*part)[COLS], double* row) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < COLS; ++j) {
    const double t = wave_sum(v[j]);
    if (lane == 0) part[wave][j] = t;
  }
  __syncthreads();
  if ((int)threadIdx.x < COLS) {
    double t = part[0][threadIdx.x];
    for (int w = 1; w < kWaves; ++w) t += part[w][threadIdx.x];
    row[threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(kWG, 3) void route_stem_kernel(const float* __restrict__ image, const float* __restrict__ w,
                                                         const float* __restrict__ bias, int Hi, int Wi, int bpi,
                                                         double* __restrict__ workspace, float* __restrict__ act,
                                                         unsigned long long* __restrict__ nonfinite) {
  __shared__ __attribute__((aligned(16))) float Wl[kTaps][kStemOut];   // [ci*9 + ky*3 + kx][c], c < 13
  __shared__ __attribute__((aligned(16))) float Bl[kStemOut];
  __shared__ double part[kWaves][kStemCols];
  __shared__ uint32_t nf;
  for (int i = threadIdx.x; i < kTaps * kStemOut; i += kWG) {
    const int c = i & 15, tap = i >> 4;
    Wl[tap][c] = c < kStemConv ? w[c * kTaps + tap] : 0.f;
  }
  if (threadIdx.x < kStemOut) Bl[threadIdx.x] = threadIdx.x < kStemConv ? bias[threadIdx.x] : 0.f;
  if (threadIdx.x == 0) nf = 0u;
  __syncthreads();

  const int H = Hi >> 1, W = Wi >> 1;
  const long long HW = (long long)H * W;               // below 2^31 (checked by the host)
  const long long n = blockIdx.x / bpi;
  const int j = blockIdx.x - (int)n * bpi;
  const float* __restrict__ img = image + n * 3 * (long long)Hi * Wi;
  double sums[kStemCols];
#pragma unroll
  for (int c = 0; c < kStemCols; ++c) sums[c] = 0.0;
  uint32_t bad = 0u;

  for (long long p = (long long)j * kWG + threadIdx.x; p < HW; p += (long long)bpi * kWG) {
    const int h = (int)((uint32_t)p / (uint32_t)W), x = (int)p - h * W;
    // An offset of 0 the compiler cannot see through: without it the 351 weights are hoisted out of the
    // loop into registers (502 of them, one wave per SIMD) instead of being read from LDS in every trip.
    int z = 0;
    asm volatile("" : "+s"(z));
    const float(*Wt)[kStemOut] = Wl + z;
    // The 27 taps first, every address clamped into the image, and a use the compiler cannot move: left
    // alone it sinks each load into the branch that consumes it and waits for every one in turn, 27 round
    // trips to memory per position.  Now they are in flight together.
    float v[kTaps];
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) {
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int y = 2 * h - 1 + ky;                  // <= Hi - 1: only y = -1 falls outside
        const float* __restrict__ row = img + ((long long)ci * Hi + max(y, 0)) * Wi;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) v[ci * 9 + ky * 3 + kx] = row[max(2 * x - 1 + kx, 0)];   // <= Wi - 1 likewise
      }
    }
#pragma unroll
    for (int t = 0; t < kTaps; ++t) asm volatile("" : "+v"(v[t]));

    float a[kStemOut];
#pragma unroll
    for (int c = 0; c < kStemOut; ++c) a[c] = Bl[c];
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) {
      float pool = 0.f;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int tap = ci * 9 + ky * 3 + kx;
          if ((ky > 0 || h > 0) && (kx > 0 || x > 0)) {   // the tap is inside the image
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const f32x4 wv = *reinterpret_cast<const f32x4*>(&Wt[tap][q * 4]);
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (q * 4 + e < kStemConv) a[q * 4 + e] = __builtin_fmaf(v[tap], wv[e], a[q * 4 + e]);
            }
          }
          if (ky >= 1 && kx >= 1)                      // the 2x2 block, row-major; a NaN wins and stays
            pool = (ky == 1 && kx == 1) || v[tap] > pool || v[tap] != v[tap] ? v[tap] : pool;
        }
      }
      a[kStemConv + ci] = pool;
    }

    if (act) {
      float* o = act + (n * HW + p) * kStemOut;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 v = {a[q * 4], a[q * 4 + 1], a[q * 4 + 2], a[q * 4 + 3]};
        *reinterpret_cast<f32x4*>(o + q * 4) = v;
      }
    }
    bool ok = true;
#pragma unroll
    for (int c = 0; c < kStemOut; ++c) {
      const double v = (double)a[c];
      sums[2 * c] += v;
      sums[2 * c + 1] += v * v;                        // exact: 24 x 24 bits
      ok = ok && is_finite(a[c]);
    }
    bad += ok ? 0u : 1u;
  }

  if (nonfinite) {
    if (bad) atomicAdd(&nf, bad);
    __syncthreads();
    if (threadIdx.x == 0 && nf) atomicAdd(nonfinite + n, (unsigned long long)nf);
  }
  if (workspace) store_row<kStemCols>(sums, part, workspace + (long long)blockIdx.x * kStemCols);
}

// 2 waves per SIMD like calib_head: the 32 differences of a parity stay in registers
__global__ __launch_bounds__(kWG, 2) void route_head_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, int H, int W, int nc, int bpi,
                                                            unsigned char* __restrict__ label, float* __restrict__ conf_map,
                                                            float* __restrict__ ent_map, float* __restrict__ margin_map,
                                                            double* __restrict__ workspace,
                                                            unsigned long long* __restrict__ nonfinite) {
  __shared__ __attribute__((aligned(16))) float Wp[4][kMaxC][16];   // [a*2+b][c][ci]
  __shared__ float Bl[kMaxC];
  __shared__ double part[kWaves][kHeadCols];
  __shared__ uint32_t nf;
  stage_parity<kWG>(w, bias, nc, Wp, Bl);
  if (threadIdx.x == 0) nf = 0u;
  __syncthreads();

  const long long HW = (long long)H * W;               // below 2^31 (checked by the host)
  const long long n = blockIdx.x / bpi;
  const int j = blockIdx.x - (int)n * bpi;
  const bool summing = workspace || nonfinite;
  double sums[kHeadCols] = {0.0, 0.0, 0.0};            // ent, conf, margin
  uint32_t bad = 0u;

  for (long long p = (long long)j * kWG + threadIdx.x; p < HW; p += (long long)bpi * kWG) {
    const long long q = n * HW + p;
    f32x4 xv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xv[k] = *reinterpret_cast<const f32x4*>(x + q * 16 + k * 4);
    const int h = (int)((uint32_t)p / (uint32_t)W);
    const long long r = n * H + h;
    const long long o0 = (2 * r * 2 * W) + 2 * (p - (long long)h * W);   // pixel (2h, 2w); row below: + 2W
    uint32_t labels = 0u;                                                // byte a*2+b

#pragma unroll 1
    for (int par = 0; par < 4; ++par) {
      float d[kMaxC];
      parity_logits<kMaxC>(xv, Wp, Bl, par, nc, d);                  // predict_head.hip's chain, per parity
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
          v = v == -INFINITY ? -FLT_MAX : v;                             // 0 * d_c stays 0; a NaN stays a NaN
          const float e = __builtin_amdgcn_exp2f(__fmul_rn(v, kLog2e));
          s += e;
          A = __builtin_fmaf(e, v, A);
          e2 = c != bi ? fmaxf(e2, e) : e2;
        }
      }
      const float logs = logf(s);
      const float conf = 1.0f / s;
      const float ent = __fsub_rn(logs, __fmul_rn(A, conf));
      const float margin = __fmul_rn(conf, __fsub_rn(1.0f, e2));
      labels |= (uint32_t)bi << (8 * par);
      const long long o = o0 + (long long)(par >> 1) * 2 * W + (par & 1);
      if (conf_map) conf_map[o] = conf;
      if (ent_map) ent_map[o] = ent;
      if (margin_map) margin_map[o] = margin;
      if (summing) {
        if (is_finite(s)) {
          sums[0] += (double)ent;
          sums[1] += (double)conf;
          sums[2] += (double)margin;
        } else {
          ++bad;
        }
      }
    }

    if (label) {
      *reinterpret_cast<uint16_t*>(label + o0) = (uint16_t)(labels & 0xffffu);
      *reinterpret_cast<uint16_t*>(label + o0 + 2LL * W) = (uint16_t)(labels >> 16);
    }
  }

  if (nonfinite) {
    if (bad) atomicAdd(&nf, bad);
    __syncthreads();
    if (threadIdx.x == 0 && nf) atomicAdd(nonfinite + n, (unsigned long long)nf);
  }
  if (workspace) store_row<kHeadCols>(sums, part, workspace + (long long)blockIdx.x * kHeadCols);
}

// Work-groups of ONE image with H x W positions: a function of H and W alone.
inline int blocks_per_image(long long HW) { return bounded_grid(HW, kWG, kMaxBlocksPerImage); }

// N images of H x W positions that the per-image grids can index.  Sets no message.
inline bool route_shape_ok(int N, int H, int W) {
  if (!shape_ok(N, H, W, kMaxPixels)) return false;
  const long long HW = (long long)H * W;
  // a launch holds fewer than 2^32 work-items: the main kernel's N * bpi groups of 256, the fold's 32 N of 64
  return HW <= 0x7fffffffLL && (long long)N * blocks_per_image(HW) * kWG <= 0xffffffffLL &&
         (long long)N * kStemCols * 64 <= 0xffffffffLL;
}

inline bool fold(const char* fn, const double* workspace, int bpi, int N, int cols, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(fold_rows, dim3(N * cols), dim3(64), 0, stream, workspace, bpi, cols, out);
  return launched(fn);
}

}  // namespace

API int mdil_route_version(void) { return 100; }
API const char* mdil_route_last_error(void) { return g_err; }

API long long mdil_route_stem_workspace_bytes(int N, int Hi, int Wi) {
  if (N <= 0 || Hi <= 0 || Wi <= 0 || (Hi & 1) || (Wi & 1) || !route_shape_ok(N, Hi / 2, Wi / 2)) return -1;
  return (long long)N * blocks_per_image((long long)(Hi / 2) * (Wi / 2)) * kStemCols * (long long)sizeof(double);
}

API int mdil_route_stem(const float* image, const float* w, const float* bias, int N, int Hi, int Wi, double* moments,
                        float* act, long long* nonfinite, void* workspace, long long workspace_bytes, void* stream) {
  if (!image || !w || !bias || N <= 0 || Hi <= 0 || Wi <= 0) {
    set_error("route_stem: bad argument (image %p w %p bias %p N %d Hi %d Wi %d)", (const void*)image, (const void*)w,
              (const void*)bias, N, Hi, Wi);
    return MDIL_ROUTE_ERR_INVALID;
  }
  if ((Hi & 1) || (Wi & 1)) {
    set_error("route_stem: image size %d x %d: Hi and Wi must be even", Hi, Wi);
    return MDIL_ROUTE_ERR_INVALID;
  }
  const int H = Hi / 2, W = Wi / 2;
  if (!route_shape_ok(N, H, W)) {
    set_error("route_stem: too large (N %d, image %d x %d: at most 2^38 positions, 2^31 - 1 of one image, and fewer "
              "than 2^32 work-items in a launch)", N, Hi, Wi);
    return MDIL_ROUTE_ERR_INVALID;
  }
  if (!moments && !act && !nonfinite) {
    set_error("route_stem: nothing to write (moments, act and nonfinite are all NULL)");
    return MDIL_ROUTE_ERR_INVALID;
  }
  if (((uintptr_t)image & 3) || ((uintptr_t)w & 3) || ((uintptr_t)bias & 3) || ((uintptr_t)act & 15) ||
      ((uintptr_t)moments & 7) || ((uintptr_t)nonfinite & 7) || ((uintptr_t)workspace & 7)) {
    set_error("route_stem: alignment (image, w and bias 4 B; act 16 B; moments, nonfinite and workspace 8 B)");
    return MDIL_ROUTE_ERR_INVALID;
  }
  const int bpi = blocks_per_image((long long)H * W);
  const long long need = (long long)N * bpi * kStemCols * (long long)sizeof(double);
  if (!workspace_ok(kStemFn, moments, workspace, workspace_bytes, need)) return MDIL_ROUTE_ERR_INVALID;
  double* ws = moments ? static_cast<double*>(workspace) : nullptr;
  hipLaunchKernelGGL(route_stem_kernel, dim3(N * bpi), dim3(kWG), 0, (hipStream_t)stream, image, w, bias, Hi, Wi, bpi,
                     ws, act, reinterpret_cast<unsigned long long*>(nonfinite));
  if (!launched(kStemFn)) return MDIL_ROUTE_ERR_LAUNCH;
  if (moments && !fold(kStemFn, ws, bpi, N, kStemCols, moments, (hipStream_t)stream)) return MDIL_ROUTE_ERR_LAUNCH;
  return MDIL_ROUTE_OK;
}

API long long mdil_route_head_workspace_bytes(int N, int H, int W, int nc) {
  if (!route_shape_ok(N, H, W) || nc < MDIL_ROUTE_MIN_CLASSES || nc > MDIL_ROUTE_MAX_CLASSES) return -1;
  return (long long)N * blocks_per_image((long long)H * W) * kHeadCols * (long long)sizeof(double);
}

API int mdil_route_head(const float* x, const float* w, const float* bias, int N, int H, int W, int nc,
                        unsigned char* label, float* conf_map, float* ent_map, float* margin_map, double* scores,
                        long long* nonfinite, void* workspace, long long workspace_bytes, void* stream) {
  if (!x || !w || !bias || N <= 0 || H <= 0 || W <= 0) {
    set_error("route_head: bad argument (x %p w %p bias %p N %d H %d W %d)", (const void*)x, (const void*)w,
              (const void*)bias, N, H, W);
    return MDIL_ROUTE_ERR_INVALID;
  }
  if (!classes_ok(kHeadFn, nc, MDIL_ROUTE_MIN_CLASSES, MDIL_ROUTE_MAX_CLASSES)) return MDIL_ROUTE_ERR_INVALID;
  if (!route_shape_ok(N, H, W)) {
    set_error("route_head: too large (N %d, features %d x %d: at most 2^38 pixels, 2^31 - 1 of one image, 2 W below "
              "2^31, and fewer than 2^32 work-items in a launch)", N, H, W);
    return MDIL_ROUTE_ERR_INVALID;
  }
  if (!label && !conf_map && !ent_map && !margin_map && !scores && !nonfinite) {
    set_error("route_head: nothing to write (label, the three maps, scores and nonfinite are all NULL)");
    return MDIL_ROUTE_ERR_INVALID;
  }
  if (((uintptr_t)x & 15) || ((uintptr_t)w & 3) || ((uintptr_t)bias & 3) || ((uintptr_t)label & 1) ||
      ((uintptr_t)conf_map & 3) || ((uintptr_t)ent_map & 3) || ((uintptr_t)margin_map & 3) || ((uintptr_t)scores & 7) ||
      ((uintptr_t)nonfinite & 7) || ((uintptr_t)workspace & 7)) {
    set_error("route_head: alignment (x 16 B; w, bias and the float maps 4 B; label 2 B; scores, nonfinite and "
              "workspace 8 B)");
    return MDIL_ROUTE_ERR_INVALID;
  }
  const int bpi = blocks_per_image((long long)H * W);
  const long long need = (long long)N * bpi * kHeadCols * (long long)sizeof(double);
  if (!workspace_ok(kHeadFn, scores, workspace, workspace_bytes, need)) return MDIL_ROUTE_ERR_INVALID;
  double* ws = scores ? static_cast<double*>(workspace) : nullptr;
  hipLaunchKernelGGL(route_head_kernel, dim3(N * bpi), dim3(kWG), 0, (hipStream_t)stream, x, w, bias, H, W, nc, bpi,
                     label, conf_map, ent_map, margin_map, ws, reinterpret_cast<unsigned long long*>(nonfinite));
  if (!launched(kHeadFn)) return MDIL_ROUTE_ERR_LAUNCH;
  if (scores && !fold(kHeadFn, ws, bpi, N, kHeadCols, scores, (hipStream_t)stream)) return MDIL_ROUTE_ERR_LAUNCH;
  return MDIL_ROUTE_OK;
}
