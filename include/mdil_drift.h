/*
 * libmdil_drift.so -- C ABI of the drift add-on: two checkpoints compared at their heads.  Both
 * Decoder.output_conv (ConvTranspose2d(16, nc, 2, stride 2)), both softmaxes, the per-pixel KL
 * divergence, both argmaxes, the class-transition counts and the retained / forgotten / gained
 * counts in one pass over the two 16-channel feature maps; neither logit tensor is ever stored.
 *
 * A library of its own, beside libmdil_hip.so: nothing of the training path is compiled into it
 * or changed by it ("Drift").  Same conventions as include/mdil_predict.h:
 *
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller; the
 *     library allocates nothing, keeps no state but the thread-local error text, and every call is
 *     re-entrant.
 *   - `stream` is a hipStream_t passed as void*; the work is enqueued there, no implicit sync.
 *   - return 0 on success, negative on error; mdil_drift_last_error() gives thread-local text.
 *     Every refusal comes before any launch.
 *   - arithmetic is fp32 on the VALU; the sums are fp64.
 */
#ifndef MDIL_DRIFT_H
#define MDIL_DRIFT_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDIL_DRIFT_OK 0
#define MDIL_DRIFT_ERR_INVALID (-1)
#define MDIL_DRIFT_ERR_LAUNCH (-2)

#define MDIL_DRIFT_MIN_CLASSES 2
#define MDIL_DRIFT_MAX_CLASSES 32

int mdil_drift_version(void);
const char* mdil_drift_last_error(void);

/* Bytes of `workspace` that a call with `sums` needs for this shape: one fp64 row of nc + 1
 * partials per work-group of the (shape-determined) grid.  -1 on a bad shape or class count. */
long long mdil_drift_workspace_bytes(int N, int H, int W, int nc);

/* Model A ("before"): xa [N][H][W][16] fp32 (NHWC decoder features, 16-byte aligned), wa
 * [16][nc][2][2], ba [nc] (the ConvTranspose2d parameters in PyTorch's layout); model B ("after"):
 * xb, wb, bb of the same N, H, W, nc; 2 <= nc <= 32.  For every output pixel (n, 2h+a, 2w+b) and
 * M in {A, B}
 *      l^M_c = bias[c] + sum_ci x[n,h,w,ci] * w[ci][c][a][b]   (fp32 FMA chain, bias first, ci
 *                                                               ascending: mdil_predict_head's bits)
 *      label_M = argmax_c l^M_c; ties go to the lowest class, the first NaN wins
 *      z^M_c = l^M_c - max - log sum_c exp(l^M_c - max),  p^M_c = exp(z^M_c)
 *      kl = sum_c p^A_c (z^A_c - z^B_c)       (c ascending, fp32, not clamped)
 *      kd = sum_c p^A_c (z^A_c - p^B_c)       (KLDivLoss fed with probabilities, as the trainers do)
 *
 * target u8 [N][2H][2W] in train ids (NULL: none); ignore_index in [-1, 255].  A pixel is COUNTED
 * when there is no target, or when its target is < nc and is not ignore_index.
 *
 * Outputs; each may be NULL (not written / not added to):
 *   label_a, label_b  u8  [N][2H][2W]
 *   kl_map            f32 [N][2H][2W]  kl at every pixel, counted or not; 8-byte aligned
 *   change            u8  [N][2H][2W]  without a target: 0 labels equal, 1 labels differ; with one:
 *                                      0 both right, 1 A right and B wrong (forgotten), 2 A wrong
 *                                      and B right (gained), 3 both wrong with the same class,
 *                                      4 both wrong with different classes, 255 pixel not counted
 *   ADDED to, over counted pixels (never cleared):
 *   transition        i64 [nc][nc]     row = label_a, column = label_b
 *   confusion_a       i64 [nc][nc]     row = target, column = label_a          (needs a target)
 *   confusion_b       i64 [nc][nc]     row = target, column = label_b          (needs a target)
 *   outcome           i64 [nc][4]      row = target; both right, forgotten, gained, both wrong
 *                                                                              (needs a target)
 *   bad_targets       i64 [1]          pixels whose target is >= nc and not ignore_index
 *   sums              f64 [nc + 1]     [c]: kl summed over the counted pixels of class c, the class
 *                                      being the target when there is one, else label_a; [nc]: kd
 *                                      summed over ALL pixels.  fp32 values in fp64 sums, in an
 *                                      order fixed by N, H, W alone: no floating-point atomics, two
 *                                      calls agree bit for bit.  Needs `workspace` (8-byte aligned)
 *                                      of at least mdil_drift_workspace_bytes(N, H, W, nc) bytes;
 *                                      a second small launch folds the partials into `sums`.
 * label_a, label_b, change and target need 2-byte alignment, the counters and sums 8-byte. */
int mdil_drift_head(const float* xa, const float* wa, const float* ba, const float* xb, const float* wb,
                    const float* bb, int N, int H, int W, int nc, const unsigned char* target,
                    int ignore_index, unsigned char* label_a, unsigned char* label_b, float* kl_map,
                    unsigned char* change, long long* transition, long long* confusion_a,
                    long long* confusion_b, long long* outcome, long long* bad_targets, double* sums,
                    void* workspace, long long workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
