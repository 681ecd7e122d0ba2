/*
 * libmdil_fullres.so -- C ABI of the full-resolution add-on: Decoder.output_conv
 * (ConvTranspose2d(16, nc, 2, stride 2)), a bilinear resize of the LOGITS to any output size and
 * the per-pixel argmax in one kernel, with the confusion matrix against a ground truth of that
 * size counted in the same pass.  Neither the logits nor the resized logits are ever stored.
 *
 * A third library, beside libmdil_hip.so and libmdil_predict.so: nothing of either is compiled
 * into it or changed by it ("Full resolution").  Same conventions as
 * include/mdil_predict.h:
 *
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller; the
 *     library allocates nothing, keeps no state but the thread-local error text, and every call is
 *     re-entrant.
 *   - `stream` is a hipStream_t passed as void*; the work is enqueued there, no implicit sync.
 *   - return 0 on success, negative on error; mdil_fullres_last_error() gives thread-local text.
 *   - arithmetic is fp32 on the VALU; source coordinates and interpolation weights come from
 *     exact integers.
 */
#ifndef MDIL_FULLRES_H
#define MDIL_FULLRES_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDIL_FULLRES_OK 0
#define MDIL_FULLRES_ERR_INVALID (-1)
#define MDIL_FULLRES_ERR_LAUNCH (-2)

#define MDIL_FULLRES_MIN_CLASSES 2
#define MDIL_FULLRES_MAX_CLASSES 32
#define MDIL_FULLRES_MAX_SIZE (1 << 22)          /* Ho and Wo */
#define MDIL_FULLRES_MAX_PIXELS (1LL << 40)      /* N*H*W and N*Ho*Wo */

int mdil_fullres_version(void);
const char* mdil_fullres_last_error(void);

/* x [N][H][W][16] fp32 (NHWC decoder features, 16-byte aligned), w [16][nc][2][2] and bias [nc]
 * (the ConvTranspose2d parameters in PyTorch's layout), 2 <= nc <= 32.  With Hl = 2H, Wl = 2W and
 *      l[n, 2h+a, 2w+b, c] = bias[c] + sum_ci x[n,h,w,ci] * w[ci][c][a][b]
 * the call forms, for every output pixel (n, yo, xo), 0 <= yo < Ho, 0 <= xo < Wo,
 *      U_c = bilinear(l -> Ho x Wo)   half-pixel centres, edges clamped
 *                                     (torch's align_corners=False, no antialias)
 * for ANY Ho, Wo in [1, 2^22] (up, down, identity, non-integer ratios), with the source row of yo
 *      num = (2 yo + 1) Hl - Ho, den = 2 Ho;  num < 0: y0 = 0, rem = 0;  else y0 = num / den,
 *      rem = num % den;  y0 == Hl - 1: rem = 0;  weights (den - rem) / den on y0, rem / den on y0 + 1
 * (columns alike), and writes
 *   label   u8 [N][Ho][Wo]     id_map[argmax_c U_c]; ties go to the lowest class, a NaN wins over
 *                              every number and the first NaN wins (torch.max(1) semantics).
 *                              id_map is [nc] u8 or NULL (the class index itself)
 *   colour  u8 [N][Ho][Wo][3]  palette[argmax_c U_c]; palette is [nc][3] u8.  NULL: not written
 *                              (palette may then be NULL too)
 * and, when target (u8 [N][Ho][Wo], train ids) is given, ADDS to
 *   confusion   i64 [nc][nc]   row = target, column = argmax (the train id, whatever id_map says),
 *                              one count per pixel whose target is < nc and not ignore_index
 *   bad_targets i64 [1]        the pixels whose target is >= nc and not ignore_index
 * ignore_index = -1 ignores nothing.  With target NULL neither is touched (both may be NULL).
 * label, colour and target need 4-byte alignment, confusion and bad_targets 8-byte alignment. */
int mdil_fullres_head(const float* x, const float* w, const float* bias, int N, int H, int W, int nc,
                      int Ho, int Wo, const unsigned char* id_map, const unsigned char* palette,
                      const unsigned char* target, int ignore_index, unsigned char* label,
                      unsigned char* colour, long long* confusion, long long* bad_targets,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
