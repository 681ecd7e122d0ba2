// What the eleven head add-ons share, written once.  Private to mdil_ss_amd/ext (not under include/):
// it is compiled INTO each of the eleven libraries, which stay self-contained binaries -- the error
// buffer below is one per library -- and it shares nothing with csrc/, similarity.hip or tsne.hip.
// The arithmetic contracts (order of operations, roundings) are documented in the kernels' header
// comments; the helpers here are the single spelling of the steps they name.  Who uses what:
//   every head      set_error, bounded_grid, launched, classes_ok (boundary, segments, signif: these alone)
//   predict         vote, stage_head, logits4, colour_ok
//   fullres         axis, gather, stage_head, confusion_zero, out_size_ok, colour_ok, scoring_ok
//   ensemble        vote, axis, gather, confusion_zero, out_size_ok, colour_ok, scoring_ok
//   drift           vote, stage_head, logits4, confusion_zero, wave_sum, fold_kernel, shape_ok, ignore_ok, workspace_ok
//   calib           vote, fold_kernel (and through it wave_sum), shape_ok, ignore_ok, workspace_ok
//   route           vote, wave_sum, shape_ok, workspace_ok (its own per-image fold; calib_head's chain and forms at T = 1)
//   refine          vote, stage_head, scoring_ok (logits4's chain for the one parity a lane owns)
//   pseudo          vote, stage_head, logits4, ignore_ok
//   openset         vote
//   audit           vote, shape_ok, ignore_ok
//   acquire         vote, shape_ok, ignore_ok, byte_id_ok, apply_outputs_ok, apply_target_ok, aligned8_ok
//   ripu            ignore_ok, byte_id_ok, apply_outputs_ok, apply_target_ok, aligned8_ok (no device code of this header)
// pseudo, openset, audit, acquire and route share more through map_common.h, which includes this header: the
// per-parity Wp staging and chain, the LDS tables of integer adds and the helpers of the map kernels.
// calib_head.hip forms its logits per parity from its own Wp[a*2+b][c][ci] staging, not through
// logits4 (another LDS layout, the same chain), and keeps its DPP sums.
#pragma once
#include <hip/hip_runtime.h>
#include <initializer_list>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#define API extern "C" __attribute__((visibility("default")))

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {

thread_local char g_err[512] = "";

__attribute__((format(printf, 1, 2))) void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ------------------------------------------------------------------------------------ device
// One axis of the resize: output index o of O, source length L (even, >= 2).  -> first source
// index i0, its weight w0 and the weight w1 of i0 + 1 (0 where i0 + 1 would be clamped).
__device__ __forceinline__ void axis(int o, int L, int O, int& i0, float& w0, float& w1) {
  const long long num = (2LL * o + 1) * L - O;
  const int den = 2 * O;
  int rem = 0;
  i0 = 0;
  if (num > 0) {
    i0 = (int)(num / den);
    rem = (int)(num - (long long)i0 * den);
  }
  if (i0 >= L - 1) {
    i0 = L - 1;
    rem = 0;
  }
  w1 = (float)rem / (float)den;
  w0 = (float)(den - rem) / (float)den;
}

// The four neighbours of one output pixel, scaled: s[ci][a*2+b'] = wt[a][b'] * x[ci].
// rowoff[a]: (n*H + h) * W of the feature row under the logit row of parity a; wy[a] its weight.
// Columns are those of l' (the view's own grid); a mirrored view reads feature column W - 1 - col.
__device__ __forceinline__ void gather(const float* __restrict__ x, const long long (&rowoff)[2],
                                       const float (&wy)[2], int xo, int Wl, int Wo, int W, bool mir,
                                       f32x4 (&s)[16]) {
  int x0;
  float wx0, wx1;
  axis(xo, Wl, Wo, x0, wx0, wx1);
  const bool odd = x0 & 1;
  int c0 = x0 >> 1;                                          // feature column under x0
  int c1 = min((x0 + 1) >> 1, W - 1);                        // ... under x0 + 1 (weight 0 when clamped)
  if (mir) {
    c0 = W - 1 - c0;
    c1 = W - 1 - c1;
  }
  const int col[2] = {odd ? c1 : c0, odd ? c0 : c1};         // by parity b'
  const float wx[2] = {odd ? wx1 : wx0, odd ? wx0 : wx1};
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const float wt = wy[a] * wx[b];
      const float* p = x + (rowoff[a] + col[b]) * 16;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p + j * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[j * 4 + e][a * 2 + b] = wt * v[e];
      }
    }
  }
}

// The argmax step.  Strictly greater keeps the lowest index of a tie; a NaN replaces any number
// and is never replaced (both comparisons are false against a NaN `best`); class 0 always enters.
__device__ __forceinline__ void vote(int c, float u, float& best, int& bi) {
  const bool t = c == 0 || u > best || (u != u && best == best);
  best = t ? u : best;
  bi = t ? c : bi;
}

// The four logits (a*2+b) of class c for one feature pixel: bias first, then ci ascending.  Wc is
// Wl[c] of stage_head's table.  predict_head.hip and drift_head.hip walk the classes with it: one
// chain, so drift's labels are predict's labels bit for bit.
__device__ __forceinline__ f32x4 logits4(const f32x4 (&xv)[4], const float (*Wc)[4], float b) {
  f32x4 acc = {b, b, b, b};
#pragma unroll
  for (int ci = 0; ci < 16; ++ci) {
    const f32x4 wv = *reinterpret_cast<const f32x4*>(Wc[ci]);
    const float xs = xv[ci >> 2][ci & 3];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(xs, wv[k], acc[k]);
  }
  return acc;
}

// Stages the head's tables into LDS, by a work-group of WG lanes (the caller's barrier follows):
//   Wl[c][ci][a*2+b] = W[ci][c][a][b];  Bl[c] = bias[c];
//   Pl[c] = r | g << 8 | b << 16 of the palette (0 without a `colour` map);
//   IDS: Il[c], the byte written for class c (id_map, default c).
// ensemble_head.hip keeps its own staging: its two tables (plain and column-swapped) are flat
// arrays in dynamic LDS, and going through this routine changes its address arithmetic.
template <int WG, bool IDS>
__device__ __forceinline__ void stage_head(const float* w, const float* bias, const unsigned char* palette,
                                           const void* colour, const unsigned char* id_map, int nc,
                                           float (*Wl)[16][4], float* Bl, uint32_t* Pl, uint32_t* Il) {
  for (int i = threadIdx.x; i < nc * 64; i += WG) {
    const int k = i & 3, ci = (i >> 2) & 15, c = i >> 6;
    Wl[c][ci][k] = w[(ci * nc + c) * 4 + k];
  }
  for (int c = threadIdx.x; c < nc; c += WG) {
    Bl[c] = bias[c];
    Pl[c] = colour ? (uint32_t)palette[3 * c] | (uint32_t)palette[3 * c + 1] << 8 |
                         (uint32_t)palette[3 * c + 2] << 16
                   : 0u;
    if (IDS) Il[c] = id_map ? (uint32_t)id_map[c] : (uint32_t)c;
  }
}

// Confusion: zeroes the [nc][nc] histogram of 32-bit counters (row = target) and the counter of
// targets >= nc in LDS.  Counting a (target, prediction) pair and the work-group-uniform flush
// into the 64-bit matrix stay spelled out in fullres_head.hip and ensemble_head.hip: as inlined
// helpers they compile to different code in both kernels (a select instead of a branch, another
// block order), and the kernels' code is not to move.
template <int WG, int N>
__device__ __forceinline__ void confusion_zero(uint32_t (&hist)[N], uint32_t& bad, int nc) {
  for (int i = threadIdx.x; i < nc * nc; i += WG) hist[i] = 0u;
  if (threadIdx.x == 0) bad = 0u;
}

// Sum over the 64 lanes of a wave, every lane active: a fixed xor-shuffle tree, the same on every run.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// The second launch of drift_head and calib_head: sums[c] += the column c of the `rows` x `cols`
// workspace, one row per work-group of the main kernel.  One wavefront per entry of sums: lane l
// adds the rows l, l + 64, ... ascending, then the tree.  A template only so that the three
// libraries that never launch it do not carry it.
template <int LANES = 64>
__global__ __launch_bounds__(LANES) void fold_kernel(const double* __restrict__ workspace, int rows, int cols,
                                                     double* __restrict__ sums) {
  const int c = blockIdx.x;
  double v = 0.0;
  for (int b = threadIdx.x; b < rows; b += LANES) v += workspace[(long long)b * cols + c];
  v = wave_sum(v);
  if (threadIdx.x == 0) sums[c] += v;
}

// -------------------------------------------------------------------------------------- host
// Work-groups of `wg` lanes for `items`, at most `max_blocks`: beyond that the kernels' loops stride.
inline int bounded_grid(long long items, int wg, int max_blocks) {
  const long long blocks = (items + wg - 1) / wg;
  return (int)(blocks > max_blocks ? max_blocks : blocks);
}

// After hipLaunchKernelGGL: true when the launch was accepted.
inline bool launched(const char* fn) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return true;
  set_error("%s: launch failed: %s", fn, hipGetErrorString(e));
  return false;
}

// The argument checks: each sets the entry point's message and returns false on a refusal.
inline bool classes_ok(const char* fn, int nc, int lo, int hi) {
  if (nc >= lo && nc <= hi) return true;
  set_error("%s: nc=%d outside [%d, %d]", fn, nc, lo, hi);
  return false;
}

inline bool out_size_ok(const char* fn, int Ho, int Wo, int max_size) {
  if (Ho <= max_size && Wo <= max_size) return true;
  set_error("%s: output size %d x %d above %d", fn, Ho, Wo, max_size);
  return false;
}

inline bool colour_ok(const char* fn, const void* colour, const void* palette) {
  if (!colour || palette) return true;
  set_error("%s: a colour map needs a palette", fn);
  return false;
}

inline bool ignore_ok(const char* fn, int ignore_index) {
  if (ignore_index >= -1 && ignore_index <= 255) return true;
  set_error("%s: ignore_index=%d outside [-1, 255]", fn, ignore_index);
  return false;
}

// The annotator's entry points (acquire_apply, ripu_apply): an id that is a byte; at least one output; the
// counters that need a target; every pointer of `ptrs` (`what` names them) on an 8-byte boundary.
inline bool byte_id_ok(const char* fn, const char* name, int id) {
  if (id >= 0 && id <= 255) return true;
  set_error("%s: %s=%d outside [0, 255]", fn, name, id);
  return false;
}

inline bool apply_outputs_ok(const char* fn, std::initializer_list<const void*> outputs) {
  for (const void* p : outputs)
    if (p) return true;
  set_error("%s: nothing to write (out, mask and every counter are NULL)", fn);
  return false;
}

inline bool apply_target_ok(const char* fn, const void* target, const void* annotated, const void* bad_targets) {
  if (target || (!annotated && !bad_targets)) return true;
  set_error("%s: annotated and bad_targets need a target", fn);
  return false;
}

inline bool aligned8_ok(const char* fn, const char* what, std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= (uintptr_t)p;
  if (!(bits & 7)) return true;
  set_error("%s: alignment (%s 8 B)", fn, what);
  return false;
}

inline bool scoring_ok(const char* fn, const void* target, const void* confusion, const void* bad_targets,
                       int ignore_index) {
  if (target && (!confusion || !bad_targets)) {
    set_error("%s: a target needs a confusion matrix and a bad_targets counter", fn);
    return false;
  }
  return ignore_ok(fn, ignore_index);
}

// Features [N,H,W,16] the grid-stride kernels can index: at most max_pixels of them, 2 W in an int.
// Sets no message: the callers word their own.
inline bool shape_ok(int N, int H, int W, long long max_pixels) {
  return N > 0 && H > 0 && W > 0 && 2LL * W <= 0x7fffffffLL && (long long)N * H <= max_pixels / W;
}

// `sums` come with a workspace of at least `need` bytes (one row per work-group of the main kernel).
inline bool workspace_ok(const char* fn, const void* sums, const void* workspace, long long workspace_bytes,
                         long long need) {
  if (!sums || (workspace && workspace_bytes >= need)) return true;
  set_error("%s: sums need a workspace of %lld bytes (got %p, %lld bytes)", fn, need, workspace, workspace_bytes);
  return false;
}

}  // namespace
