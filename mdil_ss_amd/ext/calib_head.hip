// libmdil_calib.so: the calibration of a head, fused (gfx950).  Decoder.output_conv, the softmax at up
// to 16 temperatures, and per temperature the top-class confidence, the negative log-likelihood,
// the Brier score, the entropy and the reliability histogram in one pass over the 16-channel
// feature map.
//
//   l[n, 2h+a, 2w+b, c] = bias[c] + sum_ci x[n, h, w, ci] * W[ci][c][a][b]
//   label = argmax_c l,  m = max_c l,  d_c = l_c - m
//   per temperature T_k:  e_c = exp2(d_c beta2_k),  s = sum_c e_c,  conf = 1 / s,  nll = log s - d_y beta_k
//
// At batch 6 and 1024x512 the logit tensor is 252 MB that a temperature search reads once per
// candidate; here 50 MB of features come in once for 16 candidates.
//
// Layout.  A lane owns one feature pixel: 16 channels (four 16-byte loads) stay in registers.  It
// takes the four output pixels (parities a*2+b) one after the other: the nc logits of ONE parity
// are formed with predict_head's FMA chain (bias first, ci ascending: the same bits, so the label
// is that kernel's label) and kept in registers (at most 32), reduced to m and the label, turned
// into d_c, and the K temperatures loop over those registers: nc hardware exp2, 3 nc FMA-class
// operations, one log and one division per (pixel, temperature).  K x nc values are never live.
// Every loop over the classes is unrolled to 32 behind wave-uniform branches (per class where the
// logits are formed, per four classes in the temperature loop, where the classes nc .. 4 ceil(nc/4) - 1
// hold the largest negative float: e = 0 exactly, and s + 0, A + 0 * d, B + 0 change no bit), so the
// register file is indexed statically and nothing goes to scratch.  The head sits in LDS as
// Wp[a*2+b][c][ci]: one broadcast 16-byte read gives four input channels of a (parity, class) pair.
// All 64 lanes of a wave stay active through the whole loop body (a lane past the end re-reads the
// last pixel and neither counts nor stores), so ballots and DPP reductions see a full wave.
//
// Histogram.  One 64-bit cell in LDS holds the whole triple -- sum of q in bits 0..36, pixels in
// bits 37..49, correct pixels in bits 50..62 -- so a pixel costs ONE integer LDS atomic; K * bins
// cells for `hist`, nc * bins for `class_hist`, and two copies of all of them (even and odd lanes),
// which halves how many lanes of a wave meet at one address.  A trip adds at most 1024 pixels to a
// cell, so the fields hold four trips (4096 pixels, 2^36 in q): every four trips, and after the last,
// the work-group unpacks the non-zero cells and adds them to the 64-bit counters with global atomic
// adds.  Integer adds commute: exact in any order.  A trained model puts most pixels into one bin,
// and 64 lanes adding to one LDS address serialise.  So before a wave touches LDS, up to two rounds
// aggregate: the first lane still holding a value names its cell, a ballot finds the lanes that
// share it, and when they are at least 8 their values become two popcounts and one DPP reduction
// of q (64 * 2^24 fits 32 bits), added by lane 0 alone.  Whatever is left goes lane by lane.
//
// Sums.  No floating-point atomics.  Per (pixel, temperature) the three fp32 values go to fp64, are
// added over the four lanes of a quad by two DPP steps (a fixed tree) and added by the quad's first
// lane to its own fp64 slot in LDS, acc[wave][3k+j][quad].  After the loop lane 3k+j adds the 64
// slots of its entry in (wave, quad) order and stores the total to the caller's workspace, one row
// of 3 K doubles per work-group.  A second launch (head_common.h's fold_kernel, 3 K wavefronts) adds the rows -- lane l the rows
// l, l + 64, ... ascending, then a fixed xor tree -- and adds the total to sums.  The grid is a
// function of N * H * W, so the order is fixed by the shape and K.
#include "../../include/mdil_calib.h"
#include "head_common.h"

#include <float.h>
#include <math.h>

namespace {

constexpr int kWG = 256;                             // 4 wavefronts of 64 lanes
constexpr int kWaves = kWG / 64;
constexpr int kMaxC = MDIL_CALIB_MAX_CLASSES;
constexpr int kMaxK = MDIL_CALIB_MAX_TEMPS;
constexpr int kMaxBins = MDIL_CALIB_MAX_BINS;
constexpr int kMaxBlocks = 512;                      // two resident work-groups on each of 256 CUs;
                                                     // beyond 131,072 feature pixels the loop strides
constexpr int kFlushEvery = 4;                       // trips; a trip adds at most 1024 pixels to a cell
constexpr int kCountShift = 37, kCorrectShift = 50;  // fields of a cell: q 37 bits, pixels 13, correct 13
constexpr long long kMaxPixels = 1LL << 38;          // feature pixels: 4 * npix * K stays below 2^63
constexpr int kHistCells = kMaxK * kMaxBins;         // cells of `hist`; those of `class_hist` follow
constexpr int kCells = kHistCells + kMaxC * kMaxBins;
constexpr int kQuads = 16;                           // per wave
constexpr int kAggRounds = 2;                        // cells a wave aggregates before lane-wise atomics
constexpr int kAggMin = 8;                           // ... when at least this many lanes share the cell
constexpr double kLog2e = 1.4426950408889634;
constexpr char kFn[] = "calib_head";

struct CalibArgs {
  const float *x, *w, *bias;
  long long npix, plane;                             // feature pixels; output pixels of one temperature's map
  int W, nc, K, bins, class_temp, ignore_index;
  const unsigned char* target;
  unsigned char* label;
  float *conf_map, *nll_map;
  unsigned long long *hist, *class_hist, *nonfinite, *bad_targets;
  double* workspace;                                 // NULL without sums
  float beta[kMaxK + 1], beta2[kMaxK + 1];           // 1 / T and log2(e) / T; one more: the loop reads ahead
};

// v + the value `CTRL` brings from another lane; lanes of rows outside ROWS (and lanes without a
// source) add 0.  Every lane of the wave must be active.
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t dpp_add(uint32_t v) {
  return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xf, false);
}

// Sum over the 64 lanes of a wave, every lane active; the same value in every lane.
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
  v = dpp_add<0xb1, 0xf>(v);                         // quad_perm [1,0,3,2]
  v = dpp_add<0x4e, 0xf>(v);                         // quad_perm [2,3,0,1]
  v = dpp_add<0x124, 0xf>(v);                        // row_ror 4
  v = dpp_add<0x128, 0xf>(v);                        // row_ror 8: every lane holds its row's sum
  v = dpp_add<0x142, 0xa>(v);                        // row_bcast 15 into rows 1 and 3
  v = dpp_add<0x143, 0xc>(v);                        // row_bcast 31 into rows 2 and 3
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// Sum over the four lanes of a quad, every lane active: (v0 + v1) + (v2 + v3) in the quad's first lane.
__device__ __forceinline__ double quad_sum(double v) {
  v += dpp_f64<0xb1>(v);
  v += dpp_f64<0x4e>(v);
  return v;
}

// One value per lane with `valid` into the cells (count, correct, sum of q) at `key`.  Called by
// every lane of the wave.
__device__ __forceinline__ void hist_add(unsigned long long (*cells)[kCells], int key, bool valid, bool correct,
                                         uint32_t q, int lane) {
  unsigned long long rest = __ballot(valid);
#pragma unroll
  for (int r = 0; r < kAggRounds; ++r) {
    if (!rest) break;                                // uniform over the wave
    const int leader = __ffsll((unsigned long long)rest) - 1;
    const int cell = __builtin_amdgcn_readlane(key, leader);
    const bool mine = valid && key == cell;
    const unsigned long long mm = __ballot(mine);
    if (__popcll(mm) < kAggMin) break;               // uniform: too few to be worth a reduction
    const unsigned long long mc = __ballot(mine && correct);
    const uint32_t qs = wave_sum_u32(mine ? q : 0u);
    if (lane == 0)
      atomicAdd(&cells[0][cell], (unsigned long long)qs + ((unsigned long long)__popcll(mm) << kCountShift) +
                                     ((unsigned long long)__popcll(mc) << kCorrectShift));
    valid = valid && !mine;
    rest &= ~mm;
  }
  if (valid)
    atomicAdd(&cells[lane & 1][key], (unsigned long long)q + (1ull << kCountShift) +
                                         ((unsigned long long)correct << kCorrectShift));
}

__device__ __forceinline__ void flush(unsigned long long (*cells)[kCells], int first, unsigned long long* out,
                                      int n) {
  if (!out) return;
  for (int i = threadIdx.x; i < n; i += kWG) {
    const unsigned long long v = cells[0][first + i] + cells[1][first + i];   // at most 4096 pixels together
    if (v) {
      const unsigned long long cor = v >> kCorrectShift;
      atomicAdd(out + 3 * i, (v >> kCountShift) & ((1ull << (kCorrectShift - kCountShift)) - 1));
      if (cor) atomicAdd(out + 3 * i + 1, cor);
      atomicAdd(out + 3 * i + 2, v & ((1ull << kCountShift) - 1));
      cells[0][first + i] = cells[1][first + i] = 0ull;
    }
  }
}

// 2 work-groups per CU (2 waves per SIMD): 56 KB of LDS each
__global__ __launch_bounds__(kWG, 2) void calib_head_kernel(const CalibArgs p) {
  __shared__ __attribute__((aligned(16))) float Wp[4][kMaxC][16];   // [a*2+b][c][ci]
  __shared__ float Bl[kMaxC];
  __shared__ unsigned long long cells[2][kCells];     // [lane & 1][cell]: q | pixels << 37 | correct << 50
  __shared__ uint32_t nf[kMaxK];
  __shared__ uint32_t bad;
  __shared__ double acc[kWaves][kMaxK * 3][kQuads];   // a quad's own slot: only its first lane adds
  const int nc = p.nc, nc4 = (p.nc + 3) & ~3, K = p.K, bins = p.bins;
  for (int i = threadIdx.x; i < nc * 64; i += kWG) {
    const int k = i & 3, ci = (i >> 2) & 15, c = i >> 6;
    Wp[k][c][ci] = p.w[(ci * nc + c) * 4 + k];
  }
  for (int i = threadIdx.x; i < nc; i += kWG) Bl[i] = p.bias[i];
  for (int i = threadIdx.x; i < 2 * kCells; i += kWG) (&cells[0][0])[i] = 0ull;
  for (int i = threadIdx.x; i < kWaves * kMaxK * 3 * kQuads; i += kWG) (&acc[0][0][0])[i] = 0.0;
  if (threadIdx.x < kMaxK) nf[threadIdx.x] = 0u;
  if (threadIdx.x == 0) bad = 0u;
  __syncthreads();

  const unsigned char* __restrict__ target = p.target;
  const int W = p.W, ignore_index = p.ignore_index, class_temp = p.class_temp;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float fbins = (float)bins;
  const bool counting = p.hist || p.class_hist || p.nonfinite || p.bad_targets;
  int trips = 0;

  // every lane of the work-group makes every trip and stays active in it (ballots, DPP, barriers)
  for (long long base = (long long)blockIdx.x * kWG; base < p.npix; base += (long long)gridDim.x * kWG) {
    const bool inb = base + threadIdx.x < p.npix;
    const long long q = inb ? base + threadIdx.x : p.npix - 1;
    f32x4 xv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xv[j] = *reinterpret_cast<const f32x4*>(p.x + q * 16 + j * 4);
    const long long r = q / W;                                // n * H + h
    const long long o0 = (2 * r * 2 * W) + 2 * (q - r * W);   // pixel (2h, 2w); row below: + 2W
    const uint32_t tg = (uint32_t)*reinterpret_cast<const uint16_t*>(target + o0) |
                        (uint32_t)*reinterpret_cast<const uint16_t*>(target + o0 + 2LL * W) << 16;
    uint32_t labels = 0u;                                     // byte a*2+b

#pragma unroll 1
    for (int par = 0; par < 4; ++par) {
      float d[kMaxC];
      // the logits of this parity: bias first, then ci ascending (predict_head.hip's chain)
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) {
        if (c < nc) {
          float a = Bl[c];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(&Wp[par][c][j * 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e) a = __builtin_fmaf(xv[j][e], wv[e], a);
          }
          d[c] = a;
        }
      }
      const int t = (int)((tg >> (8 * par)) & 0xffu);
      const bool counted = inb && t < nc && t != ignore_index;
      float m = 0.f, ly = 0.f;
      int bi = 0;
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) {
        if (c < nc) {
          vote(c, d[c], m, bi);
          ly = c == t ? d[c] : ly;
        }
      }
      const float dy = ly - m;
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) {
        if (c < nc) {
          const float v = d[c] - m;
          d[c] = v == -INFINITY ? -FLT_MAX : v;               // 0 * d_c stays 0; a NaN stays a NaN
        } else if (c < nc4) {
          d[c] = -FLT_MAX;                                    // padding of the last four: e = 0
        }
      }
      const bool correct = bi == t;
      labels |= (uint32_t)bi << (8 * par);
      const long long o = o0 + (long long)(par >> 1) * 2 * W + (par & 1);
      if (p.bad_targets) {
        const unsigned long long bm = __ballot(inb && !counted && t != ignore_index);
        if (bm && lane == 0) atomicAdd(&bad, (uint32_t)__popcll(bm));
      }

      float beta = p.beta[0], beta2 = p.beta2[0];
#pragma unroll 1
      for (int k = 0; k < K; ++k) {
        const float beta_next = p.beta[k + 1], beta2_next = p.beta2[k + 1];   // a scalar load, in flight during k
        float s = 0.f, A = 0.f, B = 0.f;
#pragma unroll
        for (int c4 = 0; c4 < kMaxC; c4 += 4) {
          if (c4 < nc) {
            float e[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = __builtin_amdgcn_exp2f(d[c4 + j] * beta2);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              s += e[j];
              A = __builtin_fmaf(e[j], d[c4 + j], A);
              B = __builtin_fmaf(e[j], e[j], B);
            }
          }
        }
        const float ey = __builtin_amdgcn_exp2f(dy * beta2);
        const float logs = logf(s);
        const float conf = 1.0f / s;
        const float nll = logs - dy * beta;
        const float brier = __builtin_fmaf(B * conf, conf, __builtin_fmaf(-2.f, ey * conf, 1.f));
        const float ent = logs - beta * (A * conf);
        const bool finite = fabsf(s) < INFINITY && fabsf(nll) < INFINITY;   // false for a NaN
        const bool binned = counted && finite;

        if (inb) {
          if (p.conf_map) p.conf_map[(long long)k * p.plane + o] = conf;
          if (p.nll_map) p.nll_map[(long long)k * p.plane + o] = counted ? nll : 0.f;
        }
        if (counting) {
          int bin = (int)(conf * fbins);
          bin = max(0, min(bins - 1, bin));
          const uint32_t qv = binned ? (uint32_t)(conf * 16777216.0f) : 0u;
          if (p.hist) hist_add(cells, k * bins + bin, binned, correct, qv, lane);
          if (p.class_hist && k == class_temp)
            hist_add(cells, kHistCells + bi * bins + bin, binned, correct, qv, lane);
          if (p.nonfinite) {
            const unsigned long long nm = __ballot(counted && !finite);
            if (nm && lane == 0) atomicAdd(&nf[k], (uint32_t)__popcll(nm));
          }
        }
        if (p.workspace) {
          const double v0 = quad_sum(counted ? (double)nll : 0.0);
          const double v1 = quad_sum(counted ? (double)brier : 0.0);
          const double v2 = quad_sum(counted ? (double)ent : 0.0);
          if ((lane & 3) == 0) {
            acc[wave][3 * k][lane >> 2] += v0;
            acc[wave][3 * k + 1][lane >> 2] += v1;
            acc[wave][3 * k + 2][lane >> 2] += v2;
          }
        }
        beta = beta_next, beta2 = beta2_next;
      }
    }

    if (p.label && inb) {
      *reinterpret_cast<uint16_t*>(p.label + o0) = (uint16_t)(labels & 0xffffu);
      *reinterpret_cast<uint16_t*>(p.label + o0 + 2LL * W) = (uint16_t)(labels >> 16);
    }

    const bool last = base + (long long)gridDim.x * kWG >= p.npix;
    if (counting && (last || ++trips == kFlushEvery)) {  // uniform over the work-group
      trips = 0;
      __syncthreads();
      flush(cells, 0, p.hist, K * bins);
      flush(cells, kHistCells, p.class_hist, nc * bins);
      if (p.nonfinite && (int)threadIdx.x < K && nf[threadIdx.x]) {
        atomicAdd(p.nonfinite + threadIdx.x, (unsigned long long)nf[threadIdx.x]);
        nf[threadIdx.x] = 0u;
      }
      if (threadIdx.x == 0 && bad) {
        atomicAdd(p.bad_targets, (unsigned long long)bad);
        bad = 0u;
      }
      __syncthreads();
    }
  }

  if (p.workspace) {
    __syncthreads();
    if ((int)threadIdx.x < 3 * K) {
      double t = 0.0;
      for (int w = 0; w < kWaves; ++w)
        for (int g = 0; g < kQuads; ++g) t += acc[w][threadIdx.x][g];
      p.workspace[(long long)blockIdx.x * (3 * K) + threadIdx.x] = t;
    }
  }
}

}  // namespace

API int mdil_calib_version(void) { return 100; }
API const char* mdil_calib_last_error(void) { return g_err; }

API long long mdil_calib_workspace_bytes(int N, int H, int W, int nc, int K) {
  if (!shape_ok(N, H, W, kMaxPixels) || nc < MDIL_CALIB_MIN_CLASSES || nc > MDIL_CALIB_MAX_CLASSES || K < 1 ||
      K > MDIL_CALIB_MAX_TEMPS)
    return -1;
  return (long long)bounded_grid((long long)N * H * W, kWG, kMaxBlocks) * (3 * K) * (long long)sizeof(double);
}

API int mdil_calib_head(const float* x, const float* w, const float* bias, int N, int H, int W, int nc,
                        const unsigned char* target, int ignore_index, const float* temps, int K, int bins,
                        int class_temp, unsigned char* label, float* conf_map, float* nll_map, long long* hist,
                        long long* class_hist, double* sums, long long* nonfinite, long long* bad_targets,
                        void* workspace, long long workspace_bytes, void* stream) {
  if (!x || !w || !bias || N <= 0 || H <= 0 || W <= 0) {
    set_error("calib_head: bad argument (x %p w %p bias %p N %d H %d W %d)", (const void*)x, (const void*)w,
              (const void*)bias, N, H, W);
    return MDIL_CALIB_ERR_INVALID;
  }
  if (!classes_ok(kFn, nc, MDIL_CALIB_MIN_CLASSES, MDIL_CALIB_MAX_CLASSES)) return MDIL_CALIB_ERR_INVALID;
  if (!shape_ok(N, H, W, kMaxPixels)) {
    set_error("calib_head: too large (N %d, features %d x %d: at most 2^38 pixels, W below 2^30)", N, H, W);
    return MDIL_CALIB_ERR_INVALID;
  }
  if (!target) {
    set_error("calib_head: a target is required");
    return MDIL_CALIB_ERR_INVALID;
  }
  if (!ignore_ok(kFn, ignore_index)) return MDIL_CALIB_ERR_INVALID;
  if (K < 1 || K > MDIL_CALIB_MAX_TEMPS || !temps) {
    set_error("calib_head: K=%d outside [1, %d] or temps NULL (%p; a HOST pointer)", K, MDIL_CALIB_MAX_TEMPS,
              (const void*)temps);
    return MDIL_CALIB_ERR_INVALID;
  }
  for (int k = 0; k < K; ++k) {
    if (!(temps[k] > 0.f) || !(temps[k] < INFINITY)) {
      set_error("calib_head: temperature %d is %g: every temperature must be finite and > 0", k, (double)temps[k]);
      return MDIL_CALIB_ERR_INVALID;
    }
  }
  if (bins < 1 || bins > MDIL_CALIB_MAX_BINS) {
    set_error("calib_head: bins=%d outside [1, %d]", bins, MDIL_CALIB_MAX_BINS);
    return MDIL_CALIB_ERR_INVALID;
  }
  if (class_temp < -1 || class_temp >= K) {
    set_error("calib_head: class_temp=%d outside [-1, K=%d)", class_temp, K);
    return MDIL_CALIB_ERR_INVALID;
  }
  if (class_hist && class_temp < 0) {
    set_error("calib_head: class_hist needs class_temp >= 0");
    return MDIL_CALIB_ERR_INVALID;
  }
  if (((uintptr_t)x & 15) || ((uintptr_t)target & 1) || ((uintptr_t)label & 1) || ((uintptr_t)conf_map & 3) ||
      ((uintptr_t)nll_map & 3) || ((uintptr_t)hist & 7) || ((uintptr_t)class_hist & 7) || ((uintptr_t)sums & 7) ||
      ((uintptr_t)nonfinite & 7) || ((uintptr_t)bad_targets & 7) || ((uintptr_t)workspace & 7)) {
    set_error("calib_head: alignment (x 16 B; target and label 2 B; conf_map and nll_map 4 B; the counters, sums "
              "and workspace 8 B)");
    return MDIL_CALIB_ERR_INVALID;
  }
  const long long npix = (long long)N * H * W;
  const int grid = bounded_grid(npix, kWG, kMaxBlocks);
  const long long need = (long long)grid * (3 * K) * (long long)sizeof(double);
  if (!workspace_ok(kFn, sums, workspace, workspace_bytes, need)) return MDIL_CALIB_ERR_INVALID;
  CalibArgs p;
  p.x = x, p.w = w, p.bias = bias;
  p.npix = npix, p.plane = 4 * npix;
  p.W = W, p.nc = nc, p.K = K, p.bins = bins, p.class_temp = class_temp, p.ignore_index = ignore_index;
  p.target = target, p.label = label, p.conf_map = conf_map, p.nll_map = nll_map;
  p.hist = reinterpret_cast<unsigned long long*>(hist);
  p.class_hist = reinterpret_cast<unsigned long long*>(class_hist);
  p.nonfinite = reinterpret_cast<unsigned long long*>(nonfinite);
  p.bad_targets = reinterpret_cast<unsigned long long*>(bad_targets);
  p.workspace = sums ? static_cast<double*>(workspace) : nullptr;
  for (int k = 0; k <= kMaxK; ++k) {
    const float beta = k < K ? 1.0f / temps[k] : 1.0f;
    p.beta[k] = beta;
    p.beta2[k] = (float)((double)beta * kLog2e);
  }
  hipLaunchKernelGGL(calib_head_kernel, dim3(grid), dim3(kWG), 0, (hipStream_t)stream, p);
  if (!launched(kFn)) return MDIL_CALIB_ERR_LAUNCH;
  if (sums) {
    hipLaunchKernelGGL(fold_kernel<>, dim3(3 * K), dim3(64), 0, (hipStream_t)stream, p.workspace, grid, 3 * K,
                       sums);
    if (!launched(kFn)) return MDIL_CALIB_ERR_LAUNCH;
  }
  return MDIL_CALIB_OK;
}
