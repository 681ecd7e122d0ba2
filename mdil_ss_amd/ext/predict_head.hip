// libmdil_predict.so: Decoder.output_conv fused with the per-pixel argmax (gfx950).
//
//   l[n, 2h+a, 2w+b, c] = bias[c] + sum_ci x[n, h, w, ci] * W[ci][c][a][b]
//   label = argmax_c l,  colour = palette[label],  confidence = 1 / sum_c exp(l_c - l_max)
//
// The logits are never stored: at batch 6 and 1024x512 they are 252 MB that the unfused path
// (mdil_outconv_fwd, then an argmax) writes and reads back, against 50 MB of features in and 3 to
// 25 MB of maps out here.
//
// Layout.  A thread owns one feature pixel: its 16 channels (four 16-byte loads) stay in registers
// and it walks the classes, forming the four logits (a, b) of one class at a time, so the class
// count is a run-time loop bound and no logit array is indexed.  The weights sit in LDS as
// Wl[c][ci][a*2+b]: one 16-byte read gives the four parity weights of a (class, input channel)
// pair, and every lane of a wave reads the same address (a broadcast, no bank conflict).  The
// confidence needs l_max before the sum, so it is a second walk that RECOMPUTES the logits with
// the same FMA chain (same bits) instead of keeping 4 x 32 of them; it runs only when asked for.
// Per feature pixel that is 64 * nc FMAs (twice with the confidence) against 64 B in, 4 to 32 B
// out.  Stores: a thread writes the two adjacent pixels 2w, 2w+1 of output rows 2h and 2h+1 as one
// packed store per row and map (2 B label, 6 B colour, 8 B confidence); consecutive lanes continue
// the row.  Grid-stride loop over feature pixels with 64-bit indices, bounded grid, any N*H*W.
#include "../../include/mdil_predict.h"
#include "head_common.h"

namespace {

constexpr int kWG = 256;                             // 4 wavefronts of 64 lanes
constexpr int kMaxC = MDIL_PREDICT_MAX_CLASSES;
constexpr int kMaxBlocks = 2048;                     // beyond 524,288 feature pixels the loop strides
constexpr char kFn[] = "predict_head";

__global__ __launch_bounds__(kWG) void predict_head_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
    long long npix, int W, int nc, const unsigned char* __restrict__ palette,
    unsigned char* __restrict__ label, unsigned char* __restrict__ colour,
    float* __restrict__ confidence) {
  __shared__ __attribute__((aligned(16))) float Wl[kMaxC][16][4];   // [c][ci][a*2+b]
  __shared__ float Bl[kMaxC];
  __shared__ uint32_t Pl[kMaxC];                                     // r | g << 8 | b << 16
  stage_head<kWG, false>(w, bias, palette, colour, nullptr, nc, Wl, Bl, Pl, nullptr);
  __syncthreads();

  for (long long q = (long long)blockIdx.x * kWG + threadIdx.x; q < npix;
       q += (long long)gridDim.x * kWG) {
    f32x4 xv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xv[k] = *reinterpret_cast<const f32x4*>(x + q * 16 + k * 4);

    const f32x4 l0 = logits4(xv, Wl[0], Bl[0]);
    float best[4] = {l0[0], l0[1], l0[2], l0[3]};
    int bi[4] = {0, 0, 0, 0};
    for (int c = 1; c < nc; ++c) {
      const f32x4 l = logits4(xv, Wl[c], Bl[c]);
#pragma unroll
      for (int k = 0; k < 4; ++k) vote(c, l[k], best[k], bi[k]);   // c >= 1: class 0 entered above
    }

    const long long r = q / W;                                   // n * H + h
    const long long o0 = (2 * r * 2 * W) + 2 * (q - r * W);      // pixel (2h, 2w); row below: + 2W
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const long long o = o0 + (long long)a * 2 * W;
      const int i0 = bi[a * 2], i1 = bi[a * 2 + 1];
      *reinterpret_cast<uint16_t*>(label + o) = (uint16_t)(i0 | i1 << 8);
      if (colour) {
        const uint32_t p0 = Pl[i0], p1 = Pl[i1];
        uint16_t* cp = reinterpret_cast<uint16_t*>(colour + o * 3);
        cp[0] = (uint16_t)(p0 & 0xffffu);
        cp[1] = (uint16_t)((p0 >> 16) | (p1 & 0xffu) << 8);
        cp[2] = (uint16_t)(p1 >> 8);
      }
    }

    if (confidence) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
      for (int c = 0; c < nc; ++c) {
        const f32x4 l = logits4(xv, Wl[c], Bl[c]);
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += expf(l[k] - best[k]);
      }
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        float2 v;
        v.x = 1.f / s[a * 2];
        v.y = 1.f / s[a * 2 + 1];
        *reinterpret_cast<float2*>(confidence + o0 + (long long)a * 2 * W) = v;
      }
    }
  }
}

}  // namespace

API int mdil_predict_version(void) { return 100; }
API const char* mdil_predict_last_error(void) { return g_err; }

API int mdil_predict_head(const float* x, const float* w, const float* bias, int N, int H, int W,
                          int nc, const unsigned char* palette, unsigned char* label,
                          unsigned char* colour, float* confidence, void* stream) {
  if (!x || !w || !bias || !label || N <= 0 || H <= 0 || W <= 0) {
    set_error("predict_head: bad argument (x %p w %p bias %p label %p N %d H %d W %d)", (const void*)x,
              (const void*)w, (const void*)bias, (void*)label, N, H, W);
    return MDIL_PREDICT_ERR_INVALID;
  }
  if (!classes_ok(kFn, nc, MDIL_PREDICT_MIN_CLASSES, MDIL_PREDICT_MAX_CLASSES) ||
      !colour_ok(kFn, colour, palette))
    return MDIL_PREDICT_ERR_INVALID;
  if (((uintptr_t)x & 15) || ((uintptr_t)label & 1) || ((uintptr_t)colour & 1) ||
      ((uintptr_t)confidence & 7)) {
    set_error("predict_head: alignment (x 16 B, label and colour 2 B, confidence 8 B)");
    return MDIL_PREDICT_ERR_INVALID;
  }
  if (2LL * W > 0x7fffffffLL) {
    set_error("predict_head: W=%d too wide", W);
    return MDIL_PREDICT_ERR_INVALID;
  }
  const long long npix = (long long)N * H * W;
  const int grid = bounded_grid(npix, kWG, kMaxBlocks);
  hipLaunchKernelGGL(predict_head_kernel, dim3(grid), dim3(kWG), 0, (hipStream_t)stream, x, w, bias,
                     npix, W, nc, palette, label, colour, confidence);
  return launched(kFn) ? MDIL_PREDICT_OK : MDIL_PREDICT_ERR_LAUNCH;
}
