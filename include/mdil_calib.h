/*
 * libmdil_calib.so -- C ABI of the calibration add-on: how far a head's confidence can be trusted.
 * Decoder.output_conv (ConvTranspose2d(16, nc, 2, stride 2)), the softmax at up to 16 temperatures
 * at once, and per temperature the top-class confidence, the negative log-likelihood, the Brier
 * score, the entropy and the full reliability histogram, in one pass over the 16-channel feature
 * map; the logit tensor is never stored.
 *
 * A library of its own, beside libmdil_hip.so: nothing of the training path is compiled into it
 * or changed by it ("Calibration").  Same conventions as include/mdil_drift.h:
 *
 *   - plain pointers and sizes only; every pointer but `temps` is DEVICE memory owned by the
 *     caller; the library allocates nothing, keeps no state but the thread-local error text, and
 *     every call is re-entrant.
 *   - `temps` is the one deliberate exception: a HOST pointer to K floats.  They are read during
 *     the call and passed to the kernel by value, so "finite and > 0" is checked before the launch.
 *   - `stream` is a hipStream_t passed as void*; the work is enqueued there, no implicit sync.
 *   - return 0 on success, negative on error; mdil_calib_last_error() gives thread-local text.
 *     Every refusal comes before any launch.
 *   - arithmetic is fp32 on the VALU; the histogram is integer; the sums are fp64.
 */
#ifndef MDIL_CALIB_H
#define MDIL_CALIB_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDIL_CALIB_OK 0
#define MDIL_CALIB_ERR_INVALID (-1)
#define MDIL_CALIB_ERR_LAUNCH (-2)

#define MDIL_CALIB_MIN_CLASSES 2
#define MDIL_CALIB_MAX_CLASSES 32
#define MDIL_CALIB_MAX_TEMPS 16
#define MDIL_CALIB_MAX_BINS 32

int mdil_calib_version(void);
const char* mdil_calib_last_error(void);

/* Bytes of `workspace` that a call with `sums` needs for this shape: one fp64 row of 3 K partials
 * per work-group of the (shape-determined) grid.  -1 on a bad shape, class count or K. */
long long mdil_calib_workspace_bytes(int N, int H, int W, int nc, int K);

/* x [N][H][W][16] fp32 (NHWC decoder features, 16-byte aligned), w [16][nc][2][2], bias [nc] (the
 * ConvTranspose2d parameters in PyTorch's layout), 2 <= nc <= 32.  target u8 [N][2H][2W] in train
 * ids, REQUIRED; ignore_index in [-1, 255].  A pixel is COUNTED when its target is < nc and is not
 * ignore_index; a target >= nc that is not ignore_index adds 1 to bad_targets.
 * temps: HOST pointer, K floats, 1 <= K <= 16, each finite and > 0.  bins in [1, 32].  class_temp in
 * [-1, K): the temperature class_hist is taken at; class_hist needs it >= 0.
 *
 * For every output pixel (n, 2h+a, 2w+b)
 *      l_c = bias[c] + sum_ci x[n,h,w,ci] * w[ci][c][a][b]   (fp32 FMA chain, bias first, ci ascending:
 *                                                             mdil_predict_head's bits)
 *      label = argmax_c l_c; ties go to the lowest class, the first NaN wins;  m = max_c l_c
 *      d_c = l_c - m, and for d_c = -inf the largest negative float where it is a factor (so 0 * d_c = 0)
 * and for every temperature k, beta = 1 / T_k and beta2 = beta * log2(e), both rounded to fp32 on the host,
 *      e_c  = exp2(d_c * beta2)                       (one hardware exp2 per class)
 *      s    = sum_c e_c,  A = sum_c e_c d_c,  B = sum_c e_c^2      (c ascending; s in [1, nc] for finite logits)
 *      conf = 1 / s                                   (the top-class probability; IEEE division)
 *      nll  = log s - d_y * beta                      (y the target)
 *      brier = (B conf) conf + (1 - 2 (e_y conf))     (= sum_c p_c^2 - 2 p_y + 1)
 *      ent  = log s - beta ((A conf))                 (= -sum_c p_c log p_c)
 *      bin  = min(bins - 1, (int)(conf * bins)),  q = (uint32)(conf * 2^24), truncating
 * A counted pixel whose s or nll is not finite at k is not binned at k and adds 1 to nonfinite[k].
 *
 * Outputs; each may be NULL (not written / not added to):
 *   label        u8  [N][2H][2W]
 *   conf_map     f32 [K][N][2H][2W]   conf at every pixel, counted or not
 *   nll_map      f32 [K][N][2H][2W]   nll at the counted pixels, 0 elsewhere
 *   ADDED to (never cleared):
 *   hist         i64 [K][bins][3]     per bin: pixels, pixels with label == target, sum of q
 *   class_hist   i64 [nc][bins][3]    the same triple at temperature class_temp, row = the PREDICTED class
 *   nonfinite    i64 [K]
 *   bad_targets  i64 [1]
 *   sums         f64 [K][3]           sum of nll, brier, ent over the counted pixels: fp32 values in fp64
 *                                     sums, in an order fixed by N, H, W and K alone: no floating-point
 *                                     atomics, two calls agree bit for bit.  Needs `workspace` (8-byte
 *                                     aligned) of at least mdil_calib_workspace_bytes(N, H, W, nc, K)
 *                                     bytes; a second small launch folds the partials into `sums`.
 * The histograms go through integer atomics only: exact, independent of order, bit-reproducible.
 * x needs 16-byte alignment, the counters, sums and workspace 8, conf_map and nll_map 4, label and
 * target 2. */
int mdil_calib_head(const float* x, const float* w, const float* bias, int N, int H, int W, int nc,
                    const unsigned char* target, int ignore_index, const float* temps, int K, int bins,
                    int class_temp, unsigned char* label, float* conf_map, float* nll_map, long long* hist,
                    long long* class_hist, double* sums, long long* nonfinite, long long* bad_targets,
                    void* workspace, long long workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
