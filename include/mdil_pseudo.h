/*
 * libmdil_pseudo.so -- C ABI of the pseudo-label add-on: class-balanced self-training labels
 * (Zou et al., ECCV 2018) for a domain that has images but no label files.  Three entry points:
 *
 *   mdil_pseudo_head    Decoder.output_conv (ConvTranspose2d(16, nc, 2, stride 2)) fused with the
 *                       argmax, the winner's softmax confidence quantised to 16 bits and a
 *                       [class][high byte] histogram of it; the logits are never stored.
 *   mdil_pseudo_refine  over stored maps: per class the histogram of the low byte inside one chosen
 *                       high byte, so that a per-class order statistic of the confidence is found
 *                       exactly from two 256-bin passes instead of a sort.
 *   mdil_pseudo_apply   over stored maps: the thresholded label map the trainers read (everything
 *                       below its class's threshold becomes `drop_id`), with its counters.
 *
 * A library of its own, beside libmdil_hip.so: nothing of the training path is compiled into it
 * or changed by it ("Pseudo-labels").  Same conventions as include/mdil_predict.h:
 *
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller; the
 *     library allocates nothing, keeps no state but the thread-local error text, and every call is
 *     re-entrant.
 *   - `stream` is a hipStream_t passed as void*; the work is enqueued there, no implicit sync.
 *   - return 0 on success, negative on error; every refusal comes before any launch;
 *     mdil_pseudo_last_error() gives thread-local text.
 *   - the logits are fp32 on the VALU; everything after the quantisation is integer arithmetic.
 *     Counters are 64-bit integers ADDED to with integer atomics, never cleared: every output is
 *     the same bytes on every run.
 */
#ifndef MDIL_PSEUDO_H
#define MDIL_PSEUDO_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDIL_PSEUDO_OK 0
#define MDIL_PSEUDO_ERR_INVALID (-1)
#define MDIL_PSEUDO_ERR_LAUNCH (-2)

#define MDIL_PSEUDO_MIN_CLASSES 2
#define MDIL_PSEUDO_MAX_CLASSES 32
#define MDIL_PSEUDO_MAX_PIXELS (1LL << 40)

int mdil_pseudo_version(void);
const char* mdil_pseudo_last_error(void);

/* x [N][H][W][16] fp32 (NHWC decoder features, 16-byte aligned), w [16][nc][2][2] and bias [nc]
 * (the ConvTranspose2d parameters in PyTorch's layout), 2 <= nc <= 32.  For every output pixel
 * (n, 2h+a, 2w+b) the nc logits, the label and the confidence are those of mdil_predict_head, by
 * the same chain of operations (same bits):
 *      l_c  = bias[c] + sum_ci x[n,h,w,ci] * w[ci][c][a][b]          (fp32 FMA chain, ci ascending)
 *      conf = 1 / sum_c exp(l_c - l_max)                              (c ascending)
 *      q    = min(65535, (uint32)(conf * 65536.0f))                   (exact scaling, truncation)
 * conf lies in (0, 1] for finite logits.  A NaN conf gives q = 0 and adds 1 to nonfinite[0].
 *   label     u8  [N][2H][2W]  argmax_c l_c (ties to the lowest class, the first NaN wins); 2-byte aligned
 *   qconf     u16 [N][2H][2W]  q; 4-byte aligned
 *   hist      i64 [nc][256]    hist[label][q >> 8] += 1 for every output pixel
 *   nonfinite i64 [1]          may be NULL (not counted); with label alone no confidence is formed
 *                              and nothing is counted
 * Each of label, qconf and hist may be NULL (not written), but not all three. */
int mdil_pseudo_head(const float* x, const float* w, const float* bias, int N, int H, int W, int nc,
                     unsigned char* label, unsigned short* qconf, long long* hist, long long* nonfinite,
                     void* stream);

/* label u8 [npix] (8-byte aligned), qconf u16 [npix] (16-byte aligned), any 1 <= npix <= 2^40.
 * sel i32 [nc] on the device: the high byte chosen per class, or -1 (or any value outside
 * [0, 255]) to skip the class.
 *   hist2      i64 [nc][256]  hist2[label][q & 255] += 1 for every pixel with (q >> 8) == sel[label]
 *   bad_labels i64 [1]        += 1 for every label >= nc; such a pixel counts nowhere else */
int mdil_pseudo_refine(const unsigned char* label, const unsigned short* qconf, long long npix, int nc,
                       const int* sel, long long* hist2, long long* bad_labels, void* stream);

/* label, qconf, npix as above.  thr i32 [nc] on the device: a pixel of class c is kept when
 * q >= thr[c], so 0 keeps the class and 65536 keeps nothing of it.  id_map u8 [nc] or NULL
 * (identity); 0 <= drop_id <= 255.
 *   out         u8  [npix]    kept ? id_map[label] : drop_id; drop_id where label >= nc.  8-byte aligned
 *   seen        i64 [nc]      seen[c] += pixels with label c
 *   kept        i64 [nc]      kept[c] += those of them that were kept
 *   bad_labels  i64 [1]       += pixels with label >= nc (they count nowhere else but in bad_targets)
 * With a target (u8 [npix], 8-byte aligned; -1 <= ignore_index <= 255, -1: none):
 *   confusion   i64 [nc][nc]  confusion[target][label] += 1 over the KEPT pixels whose target is
 *                             < nc and is not ignore_index
 *   bad_targets i64 [1]       += every pixel, kept or not, whose target is >= nc and is not ignore_index
 * out and each counter may be NULL (not written); a target needs confusion and bad_targets. */
int mdil_pseudo_apply(const unsigned char* label, const unsigned short* qconf, long long npix, int nc,
                      const int* thr, const unsigned char* id_map, int drop_id, const unsigned char* target,
                      int ignore_index, unsigned char* out, long long* seen, long long* kept,
                      long long* confusion, long long* bad_targets, long long* bad_labels, void* stream);

#ifdef __cplusplus
}
#endif
#endif
