/*
 * libmdil_audit.so -- C ABI of the label-audit add-on: which labels of a dataset does the head
 * confidently contradict?  Confident learning (Northcutt, Jiang and Chuang, JAIR 2021): per class the
 * mean self-confidence of the pixels GIVEN that class is the threshold; every pixel is counted under
 * (given class, most probable class among those at or above their own threshold), the confident
 * joint; its off-diagonal pixels are the label issues.  Two entry points:
 *
 *   mdil_audit_head   Decoder.output_conv (ConvTranspose2d(16, nc, 2, stride 2)) fused with the softmax
 *                     quantised to 16 bits per class, the per-class counts and sums of the
 *                     self-confidence (sweep 1), and with thresholds the suggested class, the
 *                     confident joint and the per-image issue counts (sweep 2); the logits are never
 *                     stored.  One kernel serves both sweeps.
 *   mdil_audit_apply  over stored maps: the cleaned label map (issues pruned or relabelled), the issue
 *                     mask, and the counters of what was acted on.
 *
 * A library of its own, beside libmdil_hip.so: nothing of the training path is compiled into it
 * or changed by it ("Label audit").  Same conventions as include/mdil_openset.h:
 *
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller; the
 *     library allocates nothing, keeps no state but the thread-local error text, and every call is
 *     re-entrant.
 *   - `stream` is a hipStream_t passed as void*; the work is enqueued there, no implicit sync.
 *   - return 0 on success, negative on error; every refusal comes before any launch;
 *     mdil_audit_last_error() gives thread-local text.
 *   - the softmax is fp32 on the VALU; everything after the 16-bit q is integer arithmetic.
 *     Counters are 64-bit integers ADDED to with integer atomics, never cleared: every output is
 *     the same bytes on every run.
 */
#ifndef MDIL_AUDIT_H
#define MDIL_AUDIT_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDIL_AUDIT_OK 0
#define MDIL_AUDIT_ERR_INVALID (-1)
#define MDIL_AUDIT_ERR_LAUNCH (-2)

#define MDIL_AUDIT_MIN_CLASSES 2
#define MDIL_AUDIT_MAX_CLASSES 32
#define MDIL_AUDIT_MAX_PIXELS (1LL << 40)
#define MDIL_AUDIT_Q_ONE 65536          /* q = min(65535, floor(p * 65536)); a threshold of 65536 is never met */
#define MDIL_AUDIT_PRUNE 0
#define MDIL_AUDIT_RELABEL 1

int mdil_audit_version(void);
const char* mdil_audit_last_error(void);

/* x [N][H][W][16] fp32 (NHWC decoder features, 16-byte aligned), w [16][nc][2][2] and bias [nc]
 * (the ConvTranspose2d parameters in PyTorch's layout), 2 <= nc <= 32.  For every output pixel
 * (n, 2h+a, 2w+b), by the chain include/mdil_openset.h spells out for mdil_route_head (same bits):
 *      l_c = bias[c] + sum_ci x[n,h,w,ci] * w[ci][c][a][b]   (fp32 FMA chain, bias first, ci ascending)
 *      m   = max_c l_c
 *      d_c = l_c - m, and for d_c = -inf the largest negative float
 *      e_c = exp2(d_c * log2(e))                       (one hardware exp2 per class)
 *      s   = sum_c e_c (c ascending),  conf = 1 / s
 * and then
 *      p_c = e_c * conf                                (one rounding)
 *      q_c = min(65535, (uint32)(p_c * 65536.0f))      (exact scaling, truncation: mdil_pseudo_head's
 *                                                       quantisation, applied to every class)
 * The softmax runs over ALL nc logits.  A pixel whose s or m is not finite adds 1 to nonfinite[0],
 * gets none_id in `suggest` and 0 in `qmap`, and enters no other counter but bad_targets.
 *
 * target u8 [N][2H][2W] (2-byte aligned) or NULL; -1 <= ignore_index <= 255 (-1: none).  A pixel is
 * VALID when there is a target, target < nc and target != ignore_index.  A target >= nc that is not
 * ignore_index adds 1 to bad_targets[0] (whether or not the pixel is finite) and counts nowhere else.
 *
 * thr i32 [nc] on the device (4-byte aligned) or NULL: class c is CONFIDENT when q_c >= thr[c]; thr[c]
 * is meant to lie in [0, 65536] (0: always, 65536: never), the kernel compares q with any int.
 * 0 <= none_id <= 255.
 *
 * Outputs; each may be NULL (not written / not added to), but not all of them:
 *   qmap        u16 [N][2H][2W]   q of class q_class for 0 <= q_class < nc; with q_class == nc the q of
 *                                 the pixel's GIVEN class (the self-confidence), 0 where the pixel is
 *                                 not valid; that needs a target.  q_class is checked only with a
 *                                 qmap.  4-byte aligned
 *   suggest     u8  [N][2H][2W]   needs thr.  The confident class with the largest logit: c ascending,
 *                                 a confident class replaces the best so far when its logit is
 *                                 strictly greater (ties go to the lowest class; the rule of
 *                                 mdil_predict_head restricted to the confident classes, so with thr
 *                                 all 0 it is that label bit for bit); none_id where no class is
 *                                 confident.  Written for every pixel, valid or not.  2-byte aligned
 *   count       i64 [nc]          count[target] += 1 over the valid finite pixels
 *   qsum        i64 [nc]          qsum[target] += q_target over the valid finite pixels
 *   joint       i64 [nc][nc + 1]  joint[target][suggested class, or column nc for none] += 1 over the
 *                                 valid finite pixels; needs thr
 *   per_image   i64 [N][nc][2]    [n][target][0] += 1 over the valid finite pixels, [n][target][1] += 1
 *                                 where the pixel is an ISSUE: valid, a class is suggested and it is
 *                                 not the target; needs thr
 *   bad_targets i64 [1]
 *   nonfinite   i64 [1]
 * count, qsum, joint, per_image and bad_targets need a target; all counters 8-byte alignment. */
int mdil_audit_head(const float* x, const float* w, const float* bias, int N, int H, int W, int nc,
                    const unsigned char* target, int ignore_index, const int* thr, int q_class, int none_id,
                    unsigned short* qmap, unsigned char* suggest, long long* count, long long* qsum,
                    long long* joint, long long* per_image, long long* bad_targets, long long* nonfinite,
                    void* stream);

/* target u8, suggest u8 (8-byte aligned), selfq u16 (16-byte aligned; the qmap of q_class == nc), all
 * [npix], any 1 <= npix <= 2^40; nc, ignore_index and none_id as above.  A pixel is an ISSUE when its
 * target is valid, suggest != none_id, suggest < nc and suggest != target.  An issue of given class c
 * is ACTED ON when selfq <= max_q[c]; max_q i32 [nc] on the device: 65535 acts on every issue of the
 * class, -1 on none.  mode: 0 prune, 1 relabel; 0 <= drop_id <= 255.
 *   out         u8  [npix]     acted on ? (prune: drop_id, relabel: suggest) : target, unchanged, ignored
 *                              and out-of-range values included.  8-byte aligned
 *   mask        u8  [npix]     255 issue and acted on, 128 issue and not acted on, 0 otherwise.  8-byte aligned
 *   seen        i64 [nc]       seen[c] += valid pixels of given class c
 *   acted       i64 [nc][nc]   acted[given][suggested] += 1 over the pixels acted on
 *   bad_targets i64 [1]        += targets >= nc that are not ignore_index
 * out, mask and each counter may be NULL (not written), but not all of them. */
int mdil_audit_apply(const unsigned char* target, const unsigned char* suggest, const unsigned short* selfq,
                     long long npix, int nc, int ignore_index, int none_id, int mode, const int* max_q,
                     int drop_id, unsigned char* out, unsigned char* mask, long long* seen, long long* acted,
                     long long* bad_targets, void* stream);

#ifdef __cplusplus
}
#endif
#endif
