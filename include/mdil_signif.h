/*
 * libmdil_signif.so -- C ABI of the significance add-on: how far an mIoU would move on another
 * validation set of the same size.  The image is the sampling unit: per-image class counts of two
 * u8 label maps (mdil_signif_count), and replicates of their sum over resampled images, scored by
 * the iouEval rule (mdil_signif_resample): the image-level bootstrap, the jackknife and, for two
 * predictors on the same images, the label-swap randomisation.  The counts and the replicate sums
 * are integers and exact; a replicate is a function of (seed, replicate index) alone.
 *
 * A fourteenth library, beside libmdil_hip.so and the add-ons: nothing of them is compiled into it
 * or changed by it ("Significance").  Same conventions as include/mdil_segments.h:
 *
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller; the library
 *     allocates nothing, keeps no state but the thread-local error text, and every call is re-entrant.
 *   - `stream` is a hipStream_t passed as void*; the work is enqueued there, no implicit sync.
 *   - return 0 on success, negative on error; mdil_signif_last_error() gives thread-local text.
 *   - every argument check answers before any launch.
 *   - u8 maps and the u32 masks need 4-byte alignment, the i64 and f64 tables 8-byte.
 */
#ifndef MDIL_SIGNIF_H
#define MDIL_SIGNIF_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDIL_SIGNIF_OK 0
#define MDIL_SIGNIF_ERR_INVALID (-1)
#define MDIL_SIGNIF_ERR_LAUNCH (-2)

#define MDIL_SIGNIF_MIN_CLASSES 2
#define MDIL_SIGNIF_MAX_CLASSES 32
#define MDIL_SIGNIF_MAX_GROUPS 2
#define MDIL_SIGNIF_MAX_SIZE (1 << 15)            /* H and W */
#define MDIL_SIGNIF_MAX_PIXELS (1LL << 40)        /* N*H*W */
#define MDIL_SIGNIF_MAX_IMAGES (1LL << 20)        /* M, the rows of a count table */
#define MDIL_SIGNIF_MAX_REPLICATES (1LL << 32)    /* first_replicate + B */

#define MDIL_SIGNIF_BOOTSTRAP 0
#define MDIL_SIGNIF_JACKKNIFE 1
#define MDIL_SIGNIF_SWAP 2

int mdil_signif_version(void);
const char* mdil_signif_last_error(void);

/* pred, target: u8 [N][H][W].  nc in [2, 32]; ignore_index in [-1, 255], -1 ignores nothing.
 * counts: i64 [M][G][3][nc], 1 <= M <= 2^20, G in {1, 2}; the call ADDS to the rows first_image ..
 * first_image + N - 1 (within [0, M)) of group g < G and touches no other entry.  The three planes
 * are tp, predicted and labelled.  For a pixel with target t and prediction p:
 *   t == ignore_index      nothing is counted
 *   else t >= nc           bad_targets[0] += 1, nothing else
 *   else                   labelled[t] += 1;  predicted[p] += 1 when p < nc, unpredicted[0] += 1
 *                          otherwise (a 255 of a pseudo-label map);  tp[t] += 1 when p == t
 * bad_targets and unpredicted (i64 [1]) are required and ADDED to.  Summed over the images the
 * planes are the diagonal, the column sums and the row sums of the confusion matrix that
 * mdil_fullres_head counts (row = target). */
int mdil_signif_count(const unsigned char* pred, const unsigned char* target, int N, int H, int W, int nc,
                      int ignore_index, long long first_image, long long M, int G, int g, long long* counts,
                      long long* bad_targets, long long* unpredicted, void* stream);

/* counts: i64 [M][G][3][nc] with every entry in [0, 2^31) -- a sum of up to 2^20 of them stays
 * below 2^51, exact as an i64 and as a double; entries outside that range are not detected.  For
 * each replicate b = first_replicate .. first_replicate + B - 1 (B >= 1, first_replicate + B <=
 * 2^32) the call writes, at index b - first_replicate:
 *   sums  i64 [B][G][3][nc], or NULL   the replicate's table (below)
 *   miou  f64 [B][G]
 *   iou   f64 [B][G][k], or NULL
 *   empty u32 [B][G], or NULL          bit c: class c has predicted + labelled == 0 in the replicate
 *
 * The random numbers are SplitMix64 on a counter: with K = (b << 32) + j + 1,
 *   z = seed + 0x9E3779B97F4A7C15 * K;  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;
 *   z *= 0x94D049BB133111EB;  z ^= z >> 31                                   (all mod 2^64)
 * so seed 0, b 0, j 0 and 1 give 0xE220A8397B1DCDAF and 0x6E789E6AA1B965F4.
 *
 *   MDIL_SIGNIF_BOOTSTRAP  sums[b] = sum over j < M of counts[idx(b, j)], idx = ((z >> 32) * M) >> 32.
 *                          The mapping of 2^32 values onto M rows is not exactly uniform: a row's
 *                          probability differs from 1/M by at most 2^-32, a relative bias of at
 *                          most M / 2^32 (2.4e-4 at the largest M, 1.2e-7 at M = 500).
 *   MDIL_SIGNIF_JACKKNIFE  sums[b] = the sum of all rows minus row b; first_replicate + B <= M.
 *   MDIL_SIGNIF_SWAP       G == 2:  sums[b][g] = sum over i < M of counts[i][g ^ (z(b, i) >> 63)]:
 *                          each image's two predictors are exchanged by a fair bit.
 *
 * Scoring is the iouEval rule in fp64, in this order: k = nc - 1 when ignore_index == nc - 1, k = nc
 * when ignore_index is outside [0, nc); any other ignore_index is refused.  With the integers
 * converted to double, iou[c] = tp / (tp + (predicted - tp) + (labelled - tp) + 1e-15), summed left
 * to right; miou = (iou[0] + iou[1] + ... + iou[k-1]) / k, added in that order.  A class that is
 * absent from a replicate scores 0 and stays in the mean, as iouEval has it. */
int mdil_signif_resample(const long long* counts, long long M, int G, int nc, int ignore_index, int mode,
                         long long first_replicate, long long B, unsigned long long seed, long long* sums,
                         double* miou, double* iou, unsigned int* empty, void* stream);

#ifdef __cplusplus
}
#endif
#endif
