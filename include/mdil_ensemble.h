/*
 * libmdil_ensemble.so -- C ABI of the ensemble add-on: multi-scale and flip test-time augmentation
 * scored in one kernel.  For each of up to 8 views (the decoder's 16-channel features of the image
 * run at some scale, plain or mirrored) it forms Decoder.output_conv (ConvTranspose2d(16, nc, 2,
 * stride 2)), un-mirrors and resizes the LOGITS bilinearly to the output size, turns them into
 * probabilities (or not), adds the views up, and writes the argmax of the sum, with the confusion
 * matrix against a ground truth of that size counted in the same pass.  No view's logits, resized
 * logits or probabilities are ever stored.
 *
 * A fourth library, beside libmdil_hip.so, libmdil_predict.so and libmdil_fullres.so: nothing of
 * them is compiled into it or changed by it ("Ensembles").  Same conventions as
 * include/mdil_fullres.h:
 *
 *   - plain pointers and sizes only; every pointer but `views` is DEVICE memory owned by the
 *     caller; the library allocates nothing, keeps no state but the thread-local error text, and
 *     every call is re-entrant.
 *   - `stream` is a hipStream_t passed as void*; the work is enqueued there, no implicit sync.
 *   - return 0 on success, negative on error; mdil_ensemble_last_error() gives thread-local text.
 *     Every argument is checked before any launch.
 *   - arithmetic is fp32 on the VALU; source coordinates and interpolation weights come from
 *     exact integers.
 */
#ifndef MDIL_ENSEMBLE_H
#define MDIL_ENSEMBLE_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDIL_ENSEMBLE_OK 0
#define MDIL_ENSEMBLE_ERR_INVALID (-1)
#define MDIL_ENSEMBLE_ERR_LAUNCH (-2)

#define MDIL_ENSEMBLE_MIN_CLASSES 2
#define MDIL_ENSEMBLE_MAX_CLASSES 32
#define MDIL_ENSEMBLE_MAX_SIZE (1 << 22)          /* Ho and Wo */
#define MDIL_ENSEMBLE_MAX_PIXELS (1LL << 40)      /* N*H_v*W_v and N*Ho*Wo */

#define MDIL_ENSEMBLE_MAX_VIEWS 8
#define MDIL_ENSEMBLE_MODE_PROB  0      /* S_c = sum_v softmax_c(U_v)   */
#define MDIL_ENSEMBLE_MODE_LOGIT 1      /* S_c = sum_v U_v,c            */

/* One view: x [N][H][W][16] fp32 (NHWC decoder features, DEVICE memory, 16-byte aligned),
 * H, W >= 1; mirrored != 0: the features were computed from the horizontally mirrored image. */
typedef struct { const float* x; int H; int W; int mirrored; } mdil_ensemble_view;

int mdil_ensemble_version(void);
const char* mdil_ensemble_last_error(void);

/* views: a HOST array of nviews entries, 1 <= nviews <= 8, read before the call returns (the
 * caller may free or reuse it at once).  All views share N, w [16][nc][2][2] and bias [nc] (the
 * ConvTranspose2d parameters in PyTorch's layout), 2 <= nc <= 32.  For view v, with Hl = 2 H_v,
 * Wl = 2 W_v,
 *      l_v[n, 2h+a, 2w+b, c] = bias[c] + sum_ci x_v[n,h,w,ci] * w[ci][c][a][b]
 *      l'_v[y, j] = l_v[y, j]              (plain view)
 *      l'_v[y, j] = l_v[y, Wl - 1 - j]     (mirrored view: its logit column j stands for image
 *                                           column Wl - 1 - j)
 *      U_v,c = bilinear(l'_v -> Ho x Wo)   half-pixel centres, edges clamped (torch's
 *                                          align_corners=False, no antialias)
 * for ANY Ho, Wo in [1, 2^22], with the source row of yo
 *      num = (2 yo + 1) Hl - Ho, den = 2 Ho;  num < 0: y0 = 0, rem = 0;  else y0 = num / den,
 *      rem = num % den;  y0 == Hl - 1: rem = 0;  weights (den - rem) / den on y0, rem / den on y0 + 1
 * (columns alike; each weight is one correctly rounded quotient of exact integers).  The vote is
 *      MODE_PROB   p_v,c = exp(U_v,c - max_c U_v) * (1 / sum_c exp(U_v,c - max_c U_v)),
 *                  S_c = p_0,c + p_1,c + ...      views ascending, fp32
 *      MODE_LOGIT  S_c = U_0,c + U_1,c + ...      views ascending, fp32
 * and the call writes, for every output pixel (n, yo, xo),
 *   label      u8 [N][Ho][Wo]     id_map[argmax_c S_c]; ties go to the lowest class, a NaN wins over
 *                                 every number and the first NaN wins (torch.max(1) semantics).  In
 *                                 MODE_PROB one NaN logit makes every p_v,c of that view and pixel
 *                                 NaN, so the label is that of class 0 (torch's softmax alike).
 *                                 id_map is [nc] u8 or NULL (the class index itself)
 *   colour     u8 [N][Ho][Wo][3]  palette[argmax_c S_c]; palette is [nc][3] u8.  NULL: not written
 *                                 (palette may then be NULL too)
 *   confidence f32 [N][Ho][Wo]    MODE_PROB: S_max / nviews, the mean probability of the winner;
 *                                 MODE_LOGIT: the winner's softmax of S / nviews,
 *                                 1 / sum_c exp((S_c - S_max) / nviews).  NULL: not written
 * and, when target (u8 [N][Ho][Wo], train ids) is given, ADDS to
 *   confusion   i64 [nc][nc]      row = target, column = argmax (the train id, whatever id_map
 *                                 says), one count per pixel whose target is < nc and not
 *                                 ignore_index
 *   bad_targets i64 [1]           the pixels whose target is >= nc and not ignore_index
 * ignore_index = -1 ignores nothing.  With target NULL neither is touched (both may be NULL).
 *
 * One plain view in MODE_LOGIT gives the bytes of mdil_fullres_head (the same operations in the
 * same order).  A mirrored view gives exactly the labels of the plain view whose features are
 * flipped along W and whose kernel columns are swapped (w[ci][c][a][1-b]): the same arithmetic on
 * the same numbers in the same order.
 * label, colour, target and confidence need 4-byte alignment, confusion and bad_targets 8-byte
 * alignment. */
int mdil_ensemble_head(const mdil_ensemble_view* views, int nviews, const float* w, const float* bias,
                       int N, int nc, int Ho, int Wo, int mode, const unsigned char* id_map,
                       const unsigned char* palette, const unsigned char* target, int ignore_index,
                       unsigned char* label, unsigned char* colour, float* confidence,
                       long long* confusion, long long* bad_targets, void* stream);

#ifdef __cplusplus
}
#endif
#endif
