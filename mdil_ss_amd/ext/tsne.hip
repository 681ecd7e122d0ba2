// libmdil_tsne.so: exact t-SNE on the device (gfx950) -- squared distances, sklearn's perplexity
// search and joint probabilities, and the gradient descent on the KL divergence.
//
// The hot path is mdil_tsne_run: one iteration over N points is one sweep over the N^2 entries of
// P (268 MB of fp32 at N = 8192) plus a few MB of partial sums, twice per iteration as launches:
//
//   sweep     P is symmetric, so the sums of point j are taken down COLUMN j: a lane owns four
//             adjacent columns (its four points' coordinates and 6 x 4 accumulators live in
//             registers), a wave walks rows, and every load is one coalesced 16-byte read per lane
//             (1 KB per wave) that is used once -- P is read exactly once per iteration.  The row
//             points y_i are wave-uniform and come from LDS (broadcast reads).  No sum crosses a
//             lane inside the loop.  A work-group is 4 waves on the same 256 columns and every
//             fourth row of a strip of rows; the waves merge through LDS in wave order and the
//             work-group stores [split][N] partial (a_x, a_y, r_x, r_y) and its own sums of s and l.
//             Grid: ceil(N / 256) column tiles x `nsplit` row strips, about 1024 work-groups.
//   finalize  Z from the work-groups' s sums (fp64, fixed order, the same bits in every
//             work-group), the partial rows merged in split order, the gradient and sklearn's
//             gains / momentum update, one lane per point.  At the switch out of the exaggeration
//             phase update and gains restart from 0 and 1 (sklearn starts a second _gradient_descent).
//   kl        (only on a KL iteration) one work-group: the divergence and the gradient norm.
//
// Every sum has a fixed order: sequential per lane, then trees over fixed lanes.  No atomics.
#include "../../include/mdil_tsne.h"

#include <hip/hip_runtime.h>
#include <math.h>
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
constexpr int kCols = 256;                     // columns of a sweep work-group: 64 lanes x 4
constexpr int kChunk = 1024;                   // row points staged in LDS at a time
constexpr int kMaxSplit = 64;
constexpr int kTargetGroups = 1024;            // sweep work-groups aimed at: 4 per CU
constexpr int kPlogpBlocks = 1024;
constexpr float kEpsF = 2.22e-16f;
constexpr double kEpsD = 2.22e-16;

// ---------------------------------------------------------------------------- workspace layout
struct Layout {
  int coltiles, nsplit, rps;                   // rps: rows per split
  size_t plogp, part4, zpart, lpart, gnpart, bytes;   // byte offsets
};

Layout layout(int N) {
  Layout L;
  L.coltiles = (N + kCols - 1) / kCols;
  int ns = kTargetGroups / L.coltiles;
  if (ns > kMaxSplit) ns = kMaxSplit;
  if (ns > (N + 31) / 32) ns = (N + 31) / 32;
  if (ns < 1) ns = 1;
  L.rps = (N + ns - 1) / ns;
  L.nsplit = (N + L.rps - 1) / L.rps;
  L.plogp = 0;                                                     // f64 [2] + f64 [kPlogpBlocks][2]
  L.part4 = (size_t)(2 + 2 * kPlogpBlocks) * 8;                    // f32 [nsplit][N][4]
  L.zpart = L.part4 + (size_t)L.nsplit * N * 16;                   // f32 [nsplit * coltiles]
  L.lpart = L.zpart + (size_t)L.nsplit * L.coltiles * 4;
  L.gnpart = L.lpart + (size_t)L.nsplit * L.coltiles * 4;          // f32 [coltiles]
  size_t run = L.gnpart + (size_t)L.coltiles * 4;
  const size_t aff = (size_t)(N + 1) * 8;                          // f64 [N] row sums + f64 total
  L.bytes = ((run > aff ? run : aff) + 15) & ~(size_t)15;
  return L;
}

// --------------------------------------------------------------------------- device reductions
// Sum over the work-group in a fixed tree; every lane gets the result.  `buf`: kWG entries.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* buf) {
  const int t = threadIdx.x;
  buf[t] = v;
  __syncthreads();
  for (int s = kWG / 2; s > 0; s >>= 1) {
    if (t < s) buf[t] += buf[t + s];
    __syncthreads();
  }
  const T r = buf[0];
  __syncthreads();
  return r;
}

// Sum of v[0 .. n) in fp64: lane t takes t, t + kWG, ... in order, then the tree.
__device__ __forceinline__ double block_sum_array(const float* v, int n, double* buf) {
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += kWG) a += (double)v[i];
  return block_sum(a, buf);
}

// ------------------------------------------------------------------------------------- sqdist
constexpr int kDT = 64;                        // output tile
constexpr int kDK = 32;                        // k chunk

__global__ __launch_bounds__(kWG) void sqdist_kernel(const float* __restrict__ X, int N, int d,
                                                     float* __restrict__ D) {
  __shared__ float A[kDT][kDK + 1], B[kDT][kDK + 1];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i0 = blockIdx.y * kDT, j0 = blockIdx.x * kDT;
  float acc[4][4] = {};
  for (int k0 = 0; k0 < d; k0 += kDK) {
    __syncthreads();
    for (int e = threadIdx.x; e < kDT * kDK; e += kWG) {
      const int r = e / kDK, k = e % kDK;
      const bool kin = k0 + k < d;
      A[r][k] = (kin && i0 + r < N) ? X[(size_t)(i0 + r) * d + k0 + k] : 0.f;
      B[r][k] = (kin && j0 + r < N) ? X[(size_t)(j0 + r) * d + k0 + k] : 0.f;
    }
    __syncthreads();
    const int kn = min(kDK, d - k0);
    for (int k = 0; k < kn; ++k) {
      float a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = A[ty + 16 * r][k];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = B[tx + 16 * c][k];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float df = a[r] - b[c];
          acc[r][c] = __builtin_fmaf(df, df, acc[r][c]);
        }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + ty + 16 * r, j = j0 + tx + 16 * c;
      if (i < N && j < N) D[(size_t)i * N + j] = acc[r][c];
    }
}

// --------------------------------------------------------------------------------- affinities
// One work-group per row, the row in (dynamic) LDS.
__global__ __launch_bounds__(kWG) void search_kernel(const float* __restrict__ D, int N, double log_perp,
                                                     double* __restrict__ beta_out, float* __restrict__ C,
                                                     double* __restrict__ rowsum) {
  extern __shared__ __attribute__((aligned(16))) float row[];
  __shared__ double buf[kWG];
  const int i = blockIdx.x, t = threadIdx.x;
  const float* src = D + (size_t)i * N;
  for (int j = t; j < N; j += kWG) row[j] = src[j];
  __syncthreads();
  double beta = 1.0, lo = -INFINITY, hi = INFINITY, beta_used = 1.0, sum_used = 1.0;
  for (int step = 0; step < MDIL_TSNE_MAX_SEARCH_STEPS; ++step) {     // uniform over the work-group
    double sp = 0.0, sdp = 0.0;
    for (int j = t; j < N; j += kWG) {
      if (j != i) {
        const double dj = (double)row[j];
        const double p = exp(-dj * beta);
        sp += p;
        sdp += dj * p;
      }
    }
    sp = block_sum(sp, buf);
    sdp = block_sum(sdp, buf);
    if (sp == 0.0) sp = 1e-8;
    const double diff = log(sp) + beta * sdp / sp - log_perp;
    beta_used = beta;
    sum_used = sp;
    if (fabs(diff) <= MDIL_TSNE_ENTROPY_TOL) break;
    if (diff > 0.0) {
      lo = beta;
      beta = (hi == INFINITY) ? beta * 2.0 : (beta + hi) * 0.5;
    } else {
      hi = beta;
      beta = (lo == -INFINITY) ? beta * 0.5 : (beta + lo) * 0.5;
    }
  }
  float* dst = C + (size_t)i * N;
  double rs = 0.0;
  for (int j = t; j < N; j += kWG) {
    const float c = (j == i) ? 0.f : (float)(exp(-(double)row[j] * beta_used) / sum_used);
    dst[j] = c;
    rs += (double)c;
  }
  rs = block_sum(rs, buf);
  if (t == 0) {
    rowsum[i] = rs;
    beta_out[i] = beta_used;
  }
}

// total = max(2 * sum_i rowsum[i], eps): the sum of C + C^T
__global__ __launch_bounds__(kWG) void total_kernel(const double* __restrict__ rowsum, int N,
                                                    double* __restrict__ total) {
  __shared__ double buf[kWG];
  double a = 0.0;
  for (int i = threadIdx.x; i < N; i += kWG) a += rowsum[i];
  a = block_sum(a, buf);
  if (threadIdx.x == 0) *total = fmax(2.0 * a, kEpsD);
}

// In place: the work-group of tile (bi, bj), bi <= bj, owns that tile and its mirror image.
__global__ __launch_bounds__(kWG) void symmetrize_kernel(float* __restrict__ P, int N,
                                                         const double* __restrict__ total) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bi > bj) return;
  __shared__ float sa[32][33], sb[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int ia = bi * 32 + r, ja = bj * 32 + tx;          // tile A: rows of bi, columns of bj
    const int ib = bj * 32 + r, jb = bi * 32 + tx;          // tile B: its mirror image
    sa[r][tx] = (ia < N && ja < N) ? P[(size_t)ia * N + ja] : 0.f;
    sb[r][tx] = (ib < N && jb < N) ? P[(size_t)ib * N + jb] : 0.f;
  }
  __syncthreads();
  const double tot = *total;
  for (int r = ty; r < 32; r += 8) {
    const int ia = bi * 32 + r, ja = bj * 32 + tx;
    if (ia < N && ja < N) {
      const float v = (float)(((double)sa[r][tx] + (double)sb[tx][r]) / tot);
      P[(size_t)ia * N + ja] = (ia == ja) ? 0.f : fmaxf(v, kEpsF);
    }
    const int ib = bj * 32 + r, jb = bi * 32 + tx;
    if (bi != bj && ib < N && jb < N) {
      const float v = (float)(((double)sa[tx][r] + (double)sb[r][tx]) / tot);
      P[(size_t)ib * N + jb] = fmaxf(v, kEpsF);
    }
  }
}

// ---------------------------------------------------------------------------------------- run
// sum p log p and sum p, once per call: block b takes rows b, b + grid, ...
template <bool VEC>
__global__ __launch_bounds__(kWG) void plogp_kernel(const float* __restrict__ P, int N,
                                                    double* __restrict__ part) {
  __shared__ double buf[kWG];
  double plp = 0.0, ps = 0.0;
  for (int i = blockIdx.x; i < N; i += gridDim.x) {
    const float* src = P + (size_t)i * N;
    if (VEC) {
      for (int j = threadIdx.x * 4; j < N; j += kWG * 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + j);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (v[k] > 0.f) {
            plp += (double)v[k] * log((double)v[k]);
            ps += (double)v[k];
          }
      }
    } else {
      for (int j = threadIdx.x; j < N; j += kWG) {
        const float v = src[j];
        if (v > 0.f) {
          plp += (double)v * log((double)v);
          ps += (double)v;
        }
      }
    }
  }
  plp = block_sum(plp, buf);
  ps = block_sum(ps, buf);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = plp;
    part[2 * blockIdx.x + 1] = ps;
  }
}

__global__ __launch_bounds__(kWG) void plogp_final_kernel(const double* __restrict__ part, int n,
                                                          double* __restrict__ out) {
  __shared__ double buf[kWG];
  double plp = 0.0, ps = 0.0;
  for (int i = threadIdx.x; i < n; i += kWG) {
    plp += part[2 * i];
    ps += part[2 * i + 1];
  }
  plp = block_sum(plp, buf);
  ps = block_sum(ps, buf);
  if (threadIdx.x == 0) {
    out[0] = plp;
    out[1] = ps;
  }
}

struct Acc {
  float s[4], ax[4], ay[4], rx[4], ry[4], l[4];
};

// One row of P against the lane's four columns.  (yjx, yjy): the lane's points; (yix, yiy): the
// row's point; p: P[row][col0 .. col0 + 3].
template <bool KL>
__device__ __forceinline__ void row_step(Acc& a, const f32x4 p, const float (&yjx)[4], const float (&yjy)[4],
                                         float yix, float yiy, int row, int col0) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float dx = yjx[k] - yix, dy = yjy[k] - yiy;
    const float d2 = __builtin_fmaf(dx, dx, dy * dy);
    const float n = __builtin_amdgcn_rcpf(1.f + d2);
    a.s[k] += (row == col0 + k) ? 0.f : n;
    const float pn = p[k] * n, n2 = n * n;
    a.ax[k] = __builtin_fmaf(pn, dx, a.ax[k]);
    a.ay[k] = __builtin_fmaf(pn, dy, a.ay[k]);
    a.rx[k] = __builtin_fmaf(n2, dx, a.rx[k]);
    a.ry[k] = __builtin_fmaf(n2, dy, a.ry[k]);
    if (KL) a.l[k] = __builtin_fmaf(p[k], -log1pf(d2), a.l[k]);
  }
}

template <bool VEC>
__device__ __forceinline__ f32x4 load_row(const float* __restrict__ P, int N, int row, int col0) {
  const float* src = P + (size_t)row * N + col0;
  if (VEC) return col0 < N ? *reinterpret_cast<const f32x4*>(src) : f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 v;
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = col0 + k < N ? src[k] : 0.f;
  return v;
}

// VEC: N is a multiple of 4 (every row 16-byte aligned, a lane's four columns all inside or all
// outside); otherwise the same walk with 4-byte loads.
template <bool VEC, bool KL>
__global__ __launch_bounds__(kWG, 4) void sweep_kernel(const float* __restrict__ P, const float* __restrict__ Y,
                                                       int N, int rps, f32x4* __restrict__ part4,
                                                       float* __restrict__ zpart, float* __restrict__ lpart) {
  __shared__ float Ysh[kChunk][2];
  __shared__ __attribute__((aligned(16))) float merge[4][6][kCols];
  __shared__ float red[kWG];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int ct = blockIdx.x, sp = blockIdx.y;
  const int col0 = ct * kCols + lane * 4;
  const int r0 = sp * rps, r1 = min(N, r0 + rps);
  float yjx[4], yjy[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool in = col0 + k < N;
    yjx[k] = in ? Y[2 * (col0 + k)] : 0.f;
    yjy[k] = in ? Y[2 * (col0 + k) + 1] : 0.f;
  }
  Acc a = {};
  for (int cb = r0; cb < r1; cb += kChunk) {               // uniform over the work-group
    const int cn = min(kChunk, r1 - cb);
    __syncthreads();
    for (int e = t; e < cn; e += kWG) {
      Ysh[e][0] = Y[2 * (cb + e)];
      Ysh[e][1] = Y[2 * (cb + e) + 1];
    }
    __syncthreads();
    int rr = wave;                                         // the wave's rows: wave, wave + 4, ...
    for (; rr + 12 < cn; rr += 16) {                       // four rows' loads in flight
      f32x4 p[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) p[u] = load_row<VEC>(P, N, cb + rr + 4 * u, col0);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        row_step<KL>(a, p[u], yjx, yjy, Ysh[rr + 4 * u][0], Ysh[rr + 4 * u][1], cb + rr + 4 * u, col0);
    }
    for (; rr < cn; rr += 4)
      row_step<KL>(a, load_row<VEC>(P, N, cb + rr, col0), yjx, yjy, Ysh[rr][0], Ysh[rr][1], cb + rr, col0);
  }
  // the four waves merge in wave order
  __syncthreads();
  *reinterpret_cast<f32x4*>(&merge[wave][0][lane * 4]) = f32x4{a.s[0], a.s[1], a.s[2], a.s[3]};
  *reinterpret_cast<f32x4*>(&merge[wave][1][lane * 4]) = f32x4{a.ax[0], a.ax[1], a.ax[2], a.ax[3]};
  *reinterpret_cast<f32x4*>(&merge[wave][2][lane * 4]) = f32x4{a.ay[0], a.ay[1], a.ay[2], a.ay[3]};
  *reinterpret_cast<f32x4*>(&merge[wave][3][lane * 4]) = f32x4{a.rx[0], a.rx[1], a.rx[2], a.rx[3]};
  *reinterpret_cast<f32x4*>(&merge[wave][4][lane * 4]) = f32x4{a.ry[0], a.ry[1], a.ry[2], a.ry[3]};
  *reinterpret_cast<f32x4*>(&merge[wave][5][lane * 4]) = f32x4{a.l[0], a.l[1], a.l[2], a.l[3]};
  __syncthreads();
  float m[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) m[q] = ((merge[0][q][t] + merge[1][q][t]) + merge[2][q][t]) + merge[3][q][t];
  const int col = ct * kCols + t;
  const bool in = col < N;
  if (in) part4[(size_t)sp * N + col] = f32x4{m[1], m[2], m[3], m[4]};
  const float zs = block_sum(in ? m[0] : 0.f, red);
  if (t == 0) zpart[sp * gridDim.x + ct] = zs;
  if (KL) {
    const float ls = block_sum(in ? m[5] : 0.f, red);
    if (t == 0) lpart[sp * gridDim.x + ct] = ls;
  }
}

__global__ __launch_bounds__(kWG) void finalize_kernel(const f32x4* __restrict__ part4,
                                                       const float* __restrict__ zpart, int nz, int nsplit,
                                                       int N, float e, float momentum, float lr, bool restart,
                                                       float* __restrict__ Y, float* __restrict__ update,
                                                       float* __restrict__ gains, float* __restrict__ gnpart) {
  __shared__ double dbuf[kWG];
  __shared__ float red[kWG];
  const float invZ = (float)(1.0 / block_sum_array(zpart, nz, dbuf));
  const int i = blockIdx.x * kWG + threadIdx.x;
  float gn = 0.f;
  if (i < N) {
    float ax = 0.f, ay = 0.f, rx = 0.f, ry = 0.f;
    for (int s = 0; s < nsplit; ++s) {
      const f32x4 v = part4[(size_t)s * N + i];
      ax += v[0];
      ay += v[1];
      rx += v[2];
      ry += v[3];
    }
    const float g[2] = {4.f * (e * ax - rx * invZ), 4.f * (e * ay - ry * invZ)};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float u = restart ? 0.f : update[2 * i + c];
      float gain = restart ? 1.f : gains[2 * i + c];
      gain = (u * g[c] < 0.f) ? gain + 0.2f : gain * 0.8f;
      gain = fmaxf(gain, 0.01f);
      const float un = momentum * u - lr * (gain * g[c]);
      gains[2 * i + c] = gain;
      update[2 * i + c] = un;
      Y[2 * i + c] += un;
    }
    gn = g[0] * g[0] + g[1] * g[1];
  }
  gn = block_sum(gn, red);
  if (threadIdx.x == 0) gnpart[blockIdx.x] = gn;
}

__global__ __launch_bounds__(kWG) void kl_kernel(const float* __restrict__ zpart, const float* __restrict__ lpart,
                                                 int nz, const float* __restrict__ gnpart, int ng,
                                                 const double* __restrict__ plogp, float e,
                                                 float* __restrict__ out) {
  __shared__ double dbuf[kWG];
  const double Z = block_sum_array(zpart, nz, dbuf);
  const double L = block_sum_array(lpart, nz, dbuf);
  const double G = block_sum_array(gnpart, ng, dbuf);
  if (threadIdx.x == 0) {
    const double S = plogp[1], ed = (double)e;
    out[0] = (float)(ed * (S * log(ed) + plogp[0] - L + S * log(Z)));
    out[1] = (float)sqrt(G);
  }
}

bool points_ok(const char* fn, int N) {
  if (N >= 2 && N <= MDIL_TSNE_MAX_POINTS) return true;
  set_error("%s: N=%d outside [2, %d]", fn, N, MDIL_TSNE_MAX_POINTS);
  return false;
}

}  // namespace

API int mdil_tsne_version(void) { return 100; }
API const char* mdil_tsne_last_error(void) { return g_err; }

API long long mdil_tsne_workspace_bytes(int N) {
  if (N < 2 || N > MDIL_TSNE_MAX_POINTS) return -1;
  return (long long)layout(N).bytes;
}

API int mdil_tsne_sqdist(const float* X, int N, int d, float* D, void* stream) {
  if (!X || !D) {
    set_error("tsne_sqdist: bad argument (X %p D %p)", (const void*)X, (void*)D);
    return MDIL_TSNE_ERR_INVALID;
  }
  if (!points_ok("tsne_sqdist", N)) return MDIL_TSNE_ERR_INVALID;
  if (d < 1 || d > MDIL_TSNE_MAX_DIM) {
    set_error("tsne_sqdist: d=%d outside [1, %d]", d, MDIL_TSNE_MAX_DIM);
    return MDIL_TSNE_ERR_INVALID;
  }
  const int tiles = (N + kDT - 1) / kDT;
  hipLaunchKernelGGL(sqdist_kernel, dim3(tiles, tiles), dim3(kWG), 0, (hipStream_t)stream, X, N, d, D);
  return launched("tsne_sqdist") ? MDIL_TSNE_OK : MDIL_TSNE_ERR_LAUNCH;
}

API int mdil_tsne_affinities(const float* D, int N, double perplexity, double* beta_out, float* P,
                             void* workspace, void* stream) {
  const char* fn = "tsne_affinities";
  if (!D || !beta_out || !P || !workspace) {
    set_error("%s: bad argument (D %p beta_out %p P %p workspace %p)", fn, (const void*)D, (void*)beta_out,
              (void*)P, workspace);
    return MDIL_TSNE_ERR_INVALID;
  }
  if (!points_ok(fn, N)) return MDIL_TSNE_ERR_INVALID;
  if (!(perplexity >= 1.0) || !(perplexity < (double)N)) {
    set_error("%s: perplexity=%g must be at least 1 and less than N=%d", fn, perplexity, N);
    return MDIL_TSNE_ERR_INVALID;
  }
  if (((uintptr_t)D & 15) || ((uintptr_t)P & 15) || ((uintptr_t)beta_out & 7) || ((uintptr_t)workspace & 15)) {
    set_error("%s: alignment (D, P and workspace 16 B; beta_out 8 B)", fn);
    return MDIL_TSNE_ERR_INVALID;
  }
  const size_t nn = (size_t)N * N * 4;
  if ((uintptr_t)D < (uintptr_t)P + nn && (uintptr_t)P < (uintptr_t)D + nn) {
    set_error("%s: D and P overlap", fn);
    return MDIL_TSNE_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  double* rowsum = (double*)workspace;
  double* total = rowsum + N;
  const size_t lds = (size_t)N * 4;
  // the row of the largest N (128 KB) is above the default limit for dynamic LDS
  const hipError_t ae = hipFuncSetAttribute(reinterpret_cast<const void*>(search_kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize,
                                            MDIL_TSNE_MAX_POINTS * 4);
  if (ae != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: cannot reserve %d bytes of LDS: %s", fn, MDIL_TSNE_MAX_POINTS * 4, hipGetErrorString(ae));
    return MDIL_TSNE_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(search_kernel, dim3(N), dim3(kWG), lds, st, D, N, log(perplexity), beta_out, P, rowsum);
  if (!launched(fn)) return MDIL_TSNE_ERR_LAUNCH;
  hipLaunchKernelGGL(total_kernel, dim3(1), dim3(kWG), 0, st, rowsum, N, total);
  if (!launched(fn)) return MDIL_TSNE_ERR_LAUNCH;
  const int tiles = (N + 31) / 32;
  hipLaunchKernelGGL(symmetrize_kernel, dim3(tiles, tiles), dim3(kWG), 0, st, P, N, total);
  return launched(fn) ? MDIL_TSNE_OK : MDIL_TSNE_ERR_LAUNCH;
}

API int mdil_tsne_run(const float* P, int N, float* Y, float* update, float* gains, int iters,
                      int first_iter, int exaggeration_iters, float exaggeration, float learning_rate,
                      int kl_every, float* kl_log, void* partials, void* stream) {
  const char* fn = "tsne_run";
  if (!P || !Y || !update || !gains || !partials || iters < 0 || first_iter < 0) {
    set_error("%s: bad argument (P %p Y %p update %p gains %p partials %p iters %d first_iter %d)", fn,
              (const void*)P, (void*)Y, (void*)update, (void*)gains, partials, iters, first_iter);
    return MDIL_TSNE_ERR_INVALID;
  }
  if (!points_ok(fn, N)) return MDIL_TSNE_ERR_INVALID;
  if (kl_every > 0 && iters >= kl_every && !kl_log) {
    set_error("%s: kl_every=%d needs a kl_log", fn, kl_every);
    return MDIL_TSNE_ERR_INVALID;
  }
  if (!(exaggeration > 0.f) || !(learning_rate > 0.f)) {
    set_error("%s: exaggeration=%g and learning_rate=%g must be positive", fn, (double)exaggeration,
              (double)learning_rate);
    return MDIL_TSNE_ERR_INVALID;
  }
  if (((uintptr_t)P & 15) || ((uintptr_t)partials & 15) || ((uintptr_t)Y & 7) || ((uintptr_t)update & 7) ||
      ((uintptr_t)gains & 7) || ((uintptr_t)kl_log & 3)) {
    set_error("%s: alignment (P and partials 16 B; Y, update and gains 8 B; kl_log 4 B)", fn);
    return MDIL_TSNE_ERR_INVALID;
  }
  if (iters == 0) return MDIL_TSNE_OK;
  hipStream_t st = (hipStream_t)stream;
  const Layout L = layout(N);
  char* base = (char*)partials;
  double* plogp = (double*)(base + L.plogp);
  f32x4* part4 = (f32x4*)(base + L.part4);
  float* zpart = (float*)(base + L.zpart);
  float* lpart = (float*)(base + L.lpart);
  float* gnpart = (float*)(base + L.gnpart);
  const bool vec = (N & 3) == 0;
  const int nz = L.nsplit * L.coltiles;
  const bool any_kl = kl_every > 0 && iters >= kl_every;
  if (any_kl) {
    const int pb = N < kPlogpBlocks ? N : kPlogpBlocks;
    if (vec)
      hipLaunchKernelGGL(plogp_kernel<true>, dim3(pb), dim3(kWG), 0, st, P, N, plogp + 2);
    else
      hipLaunchKernelGGL(plogp_kernel<false>, dim3(pb), dim3(kWG), 0, st, P, N, plogp + 2);
    if (!launched(fn)) return MDIL_TSNE_ERR_LAUNCH;
    hipLaunchKernelGGL(plogp_final_kernel, dim3(1), dim3(kWG), 0, st, plogp + 2, pb, plogp);
    if (!launched(fn)) return MDIL_TSNE_ERR_LAUNCH;
  }
  const dim3 sgrid(L.coltiles, L.nsplit);
  for (int it = 0; it < iters; ++it) {
    const bool early = (long long)first_iter + it < exaggeration_iters;
    const float e = early ? exaggeration : 1.f;
    const float momentum = early ? 0.5f : 0.8f;
    const bool kl = kl_every > 0 && it % kl_every == kl_every - 1;
#define MDIL_SWEEP(V, K) \
  hipLaunchKernelGGL((sweep_kernel<V, K>), sgrid, dim3(kWG), 0, st, P, Y, N, L.rps, part4, zpart, lpart)
    if (vec) {
      if (kl) MDIL_SWEEP(true, true); else MDIL_SWEEP(true, false);
    } else {
      if (kl) MDIL_SWEEP(false, true); else MDIL_SWEEP(false, false);
    }
#undef MDIL_SWEEP
    if (!launched(fn)) return MDIL_TSNE_ERR_LAUNCH;
    hipLaunchKernelGGL(finalize_kernel, dim3(L.coltiles), dim3(kWG), 0, st, part4, zpart, nz, L.nsplit, N, e,
                       momentum, learning_rate, (long long)first_iter + it == exaggeration_iters, Y, update, gains,
                       gnpart);
    if (!launched(fn)) return MDIL_TSNE_ERR_LAUNCH;
    if (kl) {
      hipLaunchKernelGGL(kl_kernel, dim3(1), dim3(kWG), 0, st, zpart, lpart, nz, gnpart, L.coltiles, plogp, e,
                         kl_log + 2 * (it / kl_every));
      if (!launched(fn)) return MDIL_TSNE_ERR_LAUNCH;
    }
  }
  return MDIL_TSNE_OK;
}
