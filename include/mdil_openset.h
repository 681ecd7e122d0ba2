/*
 * libmdil_openset.so -- C ABI of the open-set add-on: which pixels does the head not know?  The
 * anomaly report of driving segmentation (maximum softmax probability, max logit, free energy,
 * entropy; AUROC / AUPR / FPR at 95 % TPR against pixels outside the head's label set) and label
 * maps with a reject id.  Two entry points:
 *
 *   mdil_openset_head   Decoder.output_conv (ConvTranspose2d(16, nc, 2, stride 2)) fused with the
 *                       argmax, four per-pixel "unknown" scores, a 16-bit order-preserving code of
 *                       one of them as a map, and for each score a [group][code] histogram; the
 *                       logits are never stored.
 *   mdil_openset_apply  over stored maps: the label map with `unknown_id` where the code reaches a
 *                       threshold, the 8-bit score map, and the counters of what was rejected.
 *
 * A library of its own, beside libmdil_hip.so: nothing of the training path is compiled into it
 * or changed by it ("Open-set").  Same conventions as include/mdil_pseudo.h:
 *
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller; the
 *     library allocates nothing, keeps no state but the thread-local error text, and every call is
 *     re-entrant.
 *   - `stream` is a hipStream_t passed as void*; the work is enqueued there, no implicit sync.
 *   - return 0 on success, negative on error; every refusal comes before any launch;
 *     mdil_openset_last_error() gives thread-local text.
 *   - the scores are fp32 on the VALU; everything after the 16-bit code is integer arithmetic.
 *     Counters are 64-bit integers ADDED to with integer atomics, never cleared: every output is
 *     the same bytes on every run.
 */
#ifndef MDIL_OPENSET_H
#define MDIL_OPENSET_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDIL_OPENSET_OK 0
#define MDIL_OPENSET_ERR_INVALID (-1)
#define MDIL_OPENSET_ERR_LAUNCH (-2)

#define MDIL_OPENSET_MIN_CLASSES 2
#define MDIL_OPENSET_MAX_CLASSES 32
#define MDIL_OPENSET_MAX_PIXELS (1LL << 40)
#define MDIL_OPENSET_KINDS 4          /* 0 msp, 1 maxlogit, 2 energy, 3 entropy */
#define MDIL_OPENSET_CODES 65536
#define MDIL_OPENSET_NONFINITE_CODE 65535

int mdil_openset_version(void);
const char* mdil_openset_last_error(void);

/* x [N][H][W][16] fp32 (NHWC decoder features, 16-byte aligned), w [16][nc][2][2] and bias [nc]
 * (the ConvTranspose2d parameters in PyTorch's layout), 2 <= nc <= 32.  For every output pixel
 * (n, 2h+a, 2w+b), by the chain include/mdil_route.h documents for mdil_route_head (same bits):
 *      l_c = bias[c] + sum_ci x[n,h,w,ci] * w[ci][c][a][b]   (fp32 FMA chain, bias first, ci ascending)
 *      label = argmax_c l_c (ties to the lowest class, the first NaN wins);  m = max_c l_c
 *      d_c = l_c - m, and for d_c = -inf the largest negative float
 *      e_c = exp2(d_c * log2(e))                       (one hardware exp2 per class)
 *      s   = sum_c e_c,  A = sum_c e_c d_c             (c ascending, A as an FMA chain)
 *      conf = 1 / s,  ent = log s - (A conf)           (the product is rounded first)
 * so `label` is mdil_predict_head's and `ent` is mdil_route_head's.  The softmax runs over ALL nc
 * logits, the never-trained void logit (class nc - 1) included, as in predict, calibrate and pseudo.
 *
 * Four scores, higher = more likely unknown; each ends with + 0.0f, so that -0 becomes +0:
 *      kind 0  msp       (s - 1.0f) * conf     = 1 - p_top without cancelling against 1; one rounding of the product
 *      kind 1  maxlogit  -m
 *      kind 2  energy    -(m + log s)          the sum is rounded, then negated; log s as in ent
 *      kind 3  entropy   ent
 * The 16-bit code of a score u is a parameter-free, order-preserving key:
 *      bits = float_as_uint(u);  key = (bits & 0x80000000) ? ~bits : (bits | 0x80000000);  code = key >> 16
 * u <= v implies code(u) <= code(v); finite scores give codes in [128, 65407], -inf 127, +inf 65408.
 * A pixel whose s or m is not finite gets code 65535 in the map, adds 1 to nonfinite[0] and
 * enters no histogram.
 *
 * Groups: g = target ? group_lut[target[pixel]] : const_group; 0 = known, 1 = unknown, anything
 * else = ignored.  target u8 [N][2H][2W] (2-byte aligned) or NULL; group_lut u8 [256] on the
 * device, needed with a target; const_group in {0, 1, 2}.
 *
 * Outputs; each may be NULL (not written / not added to), but not all four:
 *   label     u8  [N][2H][2W]     2-byte aligned
 *   code      u16 [N][2H][2W]     the code of kind `map_kind` (0..3; -1 exactly when code is NULL), for
 *                                 every pixel whatever its group; 4-byte aligned
 *   hist      i64 [4][2][65536]   hist[k][g][code_k] += 1 for every kind k set in the bit mask `kinds`
 *                                 (1..15) and every finite pixel with g in {0, 1}; rows of kinds not in
 *                                 the mask are not touched.  `kinds` is checked with or without a hist.
 *   nonfinite i64 [1]
 * hist and nonfinite need 8-byte alignment. */
int mdil_openset_head(const float* x, const float* w, const float* bias, int N, int H, int W, int nc,
                      const unsigned char* target, const unsigned char* group_lut, int const_group, int kinds,
                      int map_kind, unsigned char* label, unsigned short* code, long long* hist,
                      long long* nonfinite, void* stream);

/* label u8 [npix] (8-byte aligned), code u16 [npix] (16-byte aligned), any 1 <= npix <= 2^40.  A
 * pixel is rejected when code >= thr, thr a plain int in [0, 65536]: 0 rejects everything, 65536
 * nothing.  id_map u8 [nc] or NULL (identity); 0 <= unknown_id <= 255.
 *   out         u8  [npix]    rejected ? unknown_id : id_map[label]; unknown_id where label >= nc.  8-byte aligned
 *   score       u8  [npix]    cdf_lut[code]; cdf_lut u8 [65536] on the device, needed exactly when
 *                             score is given.  8-byte aligned
 *   seen        i64 [nc]      seen[c] += pixels with label c
 *   rejected    i64 [nc]      rejected[c] += those of them that were rejected
 *   bad_labels  i64 [1]       += pixels with label >= nc; they count nowhere else
 * With a target (u8 [npix], 8-byte aligned) and its group_lut (u8 [256], as above):
 *   detect      i64 [2][2]    detect[g][rejected] += 1 for g in {0, 1}
 *   confusion   i64 [nc][nc]  confusion[target][label] += 1 over the ACCEPTED pixels of group 0 with target < nc
 *   bad_targets i64 [1]       += pixels of group 0 with target >= nc
 * out, score and each counter may be NULL (not written), but not all of them; a target needs its
 * group_lut and detect, confusion and bad_targets. */
int mdil_openset_apply(const unsigned char* label, const unsigned short* code, long long npix, int nc, int thr,
                       const unsigned char* id_map, int unknown_id, const unsigned char* cdf_lut,
                       const unsigned char* target, const unsigned char* group_lut, unsigned char* out,
                       unsigned char* score, long long* seen, long long* rejected, long long* detect,
                       long long* confusion, long long* bad_targets, long long* bad_labels, void* stream);

#ifdef __cplusplus
}
#endif
#endif
