/*
 * libmdil_predict.so -- C ABI of the inference add-on: Decoder.output_conv
 * (ConvTranspose2d(16, nc, 2, stride 2)) fused with the per-pixel argmax, so a checkpoint can be
 * turned into label / colour / confidence maps without the logits ever being stored.
 *
 * A library of its own, beside libmdil_hip.so: nothing of the training path is compiled into it
 * or changed by it ("Predict").  Same conventions as include/mdil_hip.h:
 *
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller; the
 *     library allocates nothing, keeps no state but the thread-local error text, and every call is
 *     re-entrant.
 *   - `stream` is a hipStream_t passed as void*; the work is enqueued there, no implicit sync.
 *   - return 0 on success, negative on error; mdil_predict_last_error() gives thread-local text.
 *   - arithmetic is fp32 on the VALU.
 */
#ifndef MDIL_PREDICT_H
#define MDIL_PREDICT_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDIL_PREDICT_OK 0
#define MDIL_PREDICT_ERR_INVALID (-1)
#define MDIL_PREDICT_ERR_LAUNCH (-2)

#define MDIL_PREDICT_MIN_CLASSES 2
#define MDIL_PREDICT_MAX_CLASSES 32

int mdil_predict_version(void);
const char* mdil_predict_last_error(void);

/* x [N][H][W][16] fp32 (NHWC decoder features, 16-byte aligned), w [16][nc][2][2] and bias [nc]
 * (the ConvTranspose2d parameters in PyTorch's layout), 2 <= nc <= 32.  For every output pixel
 * (n, 2h+a, 2w+b) the nc logits are
 *      l_c = bias[c] + sum_ci x[n,h,w,ci] * w[ci][c][a][b]          (fp32 FMA chain, ci ascending)
 * and the call writes
 *   label      u8  [N][2H][2W]     argmax_c l_c; ties go to the lowest class, a NaN logit wins over
 *                                  every number and the first NaN wins (torch.max(1) semantics)
 *   colour     u8  [N][2H][2W][3]  palette[label]; palette is [nc][3] u8.  NULL: not written
 *                                  (palette may then be NULL too)
 *   confidence f32 [N][2H][2W]     softmax probability of the winner, 1 / sum_c exp(l_c - l_max),
 *                                  8-byte aligned.  NULL: not written
 * label and colour need 2-byte alignment. */
int mdil_predict_head(const float* x, const float* w, const float* bias, int N, int H, int W, int nc,
                      const unsigned char* palette, unsigned char* label, unsigned char* colour,
                      float* confidence, void* stream);

#ifdef __cplusplus
}
#endif
#endif
