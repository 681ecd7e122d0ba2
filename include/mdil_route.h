/*
 * libmdil_route.so -- C ABI of the routing add-on: which domain's head to run on an image whose
 * domain is not known.  Two kernels, each with a per-image reduction:
 *
 *   mdil_route_stem  the shared stem (Conv2d(3, 13, 3, stride 2, padding 1) + 2x2 max-pool of the 3
 *                    input channels), fused with the per-image first and second moments of its 16
 *                    channels: what each domain's encoder.initial_block.bn_ini[t] keeps running
 *                    statistics of.  One pass over the image, no network forward.
 *   mdil_route_head  Decoder.output_conv (ConvTranspose2d(16, nc, 2, stride 2)), the softmax, and per
 *                    image the sums of the entropy, the top-class confidence and the top-2 margin;
 *                    the logit tensor is never stored.
 *
 * A library of its own, beside libmdil_hip.so: nothing of the training path is compiled into it
 * or changed by it ("Route").  Same conventions as include/mdil_calib.h:
 *
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller; the
 *     library allocates nothing, keeps no state but the thread-local error text, and every call is
 *     re-entrant.
 *   - `stream` is a hipStream_t passed as void*; the work is enqueued there, no implicit sync.
 *   - return 0 on success, negative on error; mdil_route_last_error() gives thread-local text.
 *     Every refusal comes before any launch.
 *   - arithmetic is fp32 on the VALU; the sums are fp64, without floating-point atomics, in an
 *     order that is fixed by the size of ONE image: image n's numbers are the same bits whether it is
 *     alone or in a batch, wherever it stands in the batch, and on every call.
 */
#ifndef MDIL_ROUTE_H
#define MDIL_ROUTE_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDIL_ROUTE_OK 0
#define MDIL_ROUTE_ERR_INVALID (-1)
#define MDIL_ROUTE_ERR_LAUNCH (-2)

#define MDIL_ROUTE_MIN_CLASSES 2
#define MDIL_ROUTE_MAX_CLASSES 32
#define MDIL_ROUTE_STEM_CHANNELS 16

int mdil_route_version(void);
const char* mdil_route_last_error(void);

/* Bytes of `workspace` that mdil_route_stem needs for `moments`: one fp64 row of 32 partials per
 * work-group, and the work-groups of one image are a function of Hi and Wi alone.  -1 on a bad shape. */
long long mdil_route_stem_workspace_bytes(int N, int Hi, int Wi);

/* image f32 [N][3][Hi][Wi] (planar, 4-byte aligned), Hi and Wi even and >= 2; w f32 [13][3][3][3] and
 * bias f32 [13] in the layout of Conv2d(3, 13, 3, stride=2, padding=1).  H = Hi / 2, W = Wi / 2.
 *
 * For every position (n, h, w)
 *      a_c      = bias[c], then one fp32 FMA chain over ci, ky, kx ascending of
 *                 image[n][ci][2h-1+ky][2w-1+kx] * w[c][ci][ky][kx]; taps outside the image are skipped   (c < 13)
 *      a_{13+ci} = max of image[n][ci][2h..2h+1][2w..2w+1]; a NaN in the block gives a NaN
 *
 * Outputs; each may be NULL (not written / not added to), but not all three:
 *   moments    f64 [N][16][2]   OVERWRITTEN: per image and channel sum a and sum a*a, every a converted
 *                               to fp64 and squared there (exact).  Needs `workspace` (8-byte aligned) of
 *                               at least mdil_route_stem_workspace_bytes(N, Hi, Wi) bytes; a second small
 *                               launch folds the partials.
 *   act        f32 [N][H][W][16] the activation itself, 16-byte aligned
 *   nonfinite  i64 [N]          ADDED to: positions with a non-finite a
 * moments, nonfinite and workspace need 8-byte alignment. */
int mdil_route_stem(const float* image, const float* w, const float* bias, int N, int Hi, int Wi, double* moments,
                    float* act, long long* nonfinite, void* workspace, long long workspace_bytes, void* stream);

/* Bytes of `workspace` that mdil_route_head needs for `scores`: one fp64 row of 3 partials per
 * work-group; the work-groups of one image are a function of H and W alone.  -1 on a bad shape or
 * class count. */
long long mdil_route_head_workspace_bytes(int N, int H, int W, int nc);

/* x [N][H][W][16] fp32 (NHWC decoder features, 16-byte aligned), w [16][nc][2][2], bias [nc] (the
 * ConvTranspose2d parameters in PyTorch's layout), 2 <= nc <= 32.
 *
 * For every output pixel (n, 2h+a, 2w+b)
 *      l_c = bias[c] + sum_ci x[n,h,w,ci] * w[ci][c][a][b]   (fp32 FMA chain, bias first, ci ascending:
 *                                                             mdil_predict_head's bits)
 *      label = argmax_c l_c; ties go to the lowest class, the first NaN wins;  m = max_c l_c
 *      d_c = l_c - m, and for d_c = -inf the largest negative float (so 0 * d_c = 0)
 *      e_c = exp2(d_c * log2(e))                       (log2(e) rounded to fp32; one hardware exp2 per class)
 *      s   = sum_c e_c,  A = sum_c e_c d_c             (c ascending, A as an FMA chain)
 *      conf   = 1 / s                                  (the top-class probability; IEEE division)
 *      ent    = log s - (A conf)                       (= -sum_c p_c log p_c; the product is rounded first)
 *      margin = conf (1 - e2),  e2 = max of e_c over c != label   (= p_top - p_second; 1 - e2 is rounded first)
 *
 * Outputs; each may be NULL (not written / not added to), but not all six:
 *   label       u8  [N][2H][2W]
 *   conf_map, ent_map, margin_map   f32 [N][2H][2W] each
 *   scores      f64 [N][3]     OVERWRITTEN: per image the sums of ent, conf and margin (in this order)
 *                              over its 4 H W pixels, fp32 values in fp64 sums.  Needs `workspace` (8-byte
 *                              aligned) of at least mdil_route_head_workspace_bytes(N, H, W, nc) bytes; a
 *                              second small launch folds the partials.
 *   nonfinite   i64 [N]        ADDED to: pixels whose s is not finite; they enter no sum
 * x needs 16-byte alignment, scores, nonfinite and workspace 8, the float maps 4, label 2. */
int mdil_route_head(const float* x, const float* w, const float* bias, int N, int H, int W, int nc,
                    unsigned char* label, float* conf_map, float* ent_map, float* margin_map, double* scores,
                    long long* nonfinite, void* workspace, long long workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
