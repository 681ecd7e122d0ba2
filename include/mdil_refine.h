/*
 * libmdil_refine.so -- C ABI of the refinement add-on: an image-guided mean-field refinement of the
 * head's softmax (a local fully-connected CRF: Kraehenbuehl & Koltun 2011, truncated to a dilated
 * window as in Teichmann & Cipolla 2018, Potts compatibility, parallel updates), fused with
 * Decoder.output_conv.  The logits are never stored: every launch forms them again from the
 * 16-channel decoder features.
 *
 *   Hl = 2H, Wl = 2W;   l_i(c) = bias[c] + sum_ci x[n,h,w,ci] * w[ci][c][a][b]   (mdil_predict_head's chain)
 *   Q0   = softmax_c(l)
 *   m_i(c) = sum_j k(i,j) * Q^{t-1}_j(c),   Q^t_i = softmax_c(l_i(c) + m_i(c)),   t = 1..T
 *   j = i + (dy*d, dx*d),  dy, dx in [-r, r],  (dy,dx) != (0,0),  j inside the image
 *   k(i,j) = (w_a/Z_a) exp(-|dp|^2/(2 theta_a^2) - |I_i - I_j|^2/(2 theta_b^2)) + (w_s/Z_s) exp(-|dp|^2/(2 theta_g^2))
 *   |dp|^2 = (dy^2 + dx^2) d^2;  |I_i - I_j|^2 over the 3 channels;  Z_a, Z_s: the sums of the two
 *   spatial factors over the full window (constants: nothing is divided by a data-dependent sum).
 *   label = argmax_c (l + m) of the last step (the argmax of Q^T; lowest index on a tie),
 *   confidence = max_c Q^T.   T = 0 is plain prediction: mdil_predict_head's label and confidence.
 *
 * A library of its own, beside libmdil_hip.so: nothing of the training path is compiled into it
 * or changed by it ("Refine").  Same conventions as include/mdil_predict.h:
 *
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller; the
 *     library allocates nothing, keeps no state but the thread-local error text, and every call is
 *     re-entrant.
 *   - `stream` is a hipStream_t passed as void*; the work is enqueued there, no implicit sync.
 *   - return 0 on success, negative on error; every refusal comes before any launch;
 *     mdil_refine_last_error() gives thread-local text.
 *   - fp32 on the VALU.  The message of a pixel is summed by one lane in one fixed order (dy
 *     ascending, then dx ascending, one FMA chain per class), so a pixel's result depends neither on
 *     the batch nor on the launch geometry.  Counters are 64-bit integers ADDED to with integer
 *     atomics, never cleared: every output is the same bytes on every run.
 */
#ifndef MDIL_REFINE_H
#define MDIL_REFINE_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDIL_REFINE_OK 0
#define MDIL_REFINE_ERR_INVALID (-1)
#define MDIL_REFINE_ERR_LAUNCH (-2)

#define MDIL_REFINE_MIN_CLASSES 2
#define MDIL_REFINE_MAX_CLASSES 32
#define MDIL_REFINE_MAX_ITERATIONS 16
#define MDIL_REFINE_MAX_RADIUS 5
#define MDIL_REFINE_MAX_DILATION 4
#define MDIL_REFINE_MAX_PIXELS (1LL << 40)

int mdil_refine_version(void);
const char* mdil_refine_last_error(void);

/* Bytes of workspace mdil_refine_head needs: 0 for iterations = 0, one Q buffer [N][2H][2W][nc] f32
 * for iterations = 1, two for iterations >= 2.  -1 (with the error text set) for sizes it refuses. */
long long mdil_refine_workspace_bytes(int N, int H, int W, int nc, int iterations);

/* features [N][H][W][16] fp32 (NHWC decoder features, 16-byte aligned), weight [16][nc][2][2] and
 * bias [nc] (the ConvTranspose2d parameters in PyTorch's layout), 2 <= nc <= 32.
 * image f32 [N][3][2H][2W], the network's own input in [0, 1], read as given (may be NULL when
 * iterations = 0).  0 <= iterations <= 16, 1 <= radius <= 5, 1 <= dilation <= 4; theta_alpha
 * (pixels), theta_beta (colour), theta_gamma (pixels) finite and > 0; w_app, w_smooth finite and >= 0.
 * workspace: at least mdil_refine_workspace_bytes() bytes, 16-byte aligned (NULL when that is 0).
 *   label       u8  [N][2H][2W]      argmax of the refined distribution; required
 *   confidence  f32 [N][2H][2W]      its maximum; 4-byte aligned
 *   q_out       f32 [N][2H][2W][nc]  the refined distribution Q^T; 16-byte aligned
 *   changed     i64 [1]              += pixels whose refined label differs from argmax_c l
 * With a target (u8 [N][2H][2W]; -1 <= ignore_index <= 255, -1: none), for every pixel whose target
 * is not ignore_index:
 *   confusion   i64 [2][nc][nc]      [0][target][argmax_c l] += 1 and [1][target][label] += 1 where target < nc
 *   bad_targets i64 [1]              += 1 where target >= nc
 * confidence, q_out, target, confusion, bad_targets and changed may be NULL (not written); a target
 * needs confusion and bad_targets.
 * Launches: one that writes Q0 (iterations >= 1), iterations - 1 steps, and a last one that is a
 * step fused with the argmax, the label / confidence writes and the counters. */
int mdil_refine_head(const float* features, const float* weight, const float* bias, const float* image, int N,
                     int H, int W, int nc, int iterations, int radius, int dilation, float w_app, float w_smooth,
                     float theta_alpha, float theta_beta, float theta_gamma, void* workspace,
                     long long workspace_bytes, unsigned char* label, float* confidence, float* q_out,
                     const unsigned char* target, int ignore_index, long long* confusion, long long* bad_targets,
                     long long* changed, void* stream);

#ifdef __cplusplus
}
#endif
#endif
