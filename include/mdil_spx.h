/*
 * libmdil_spx.so -- C ABI of the superpixel acquisition add-on: regions that follow the image instead of a
 * grid (Cai et al., "Revisiting Superpixels for Active Learning in Semantic Segmentation with Realistic
 * Annotation Costs", CVPR 2021).  libmdil_acquire.so ranks the tiles of a fixed grid and libmdil_ripu.so
 * sliding square windows; here the image is over-segmented by an integer SLIC (Achanta et al., 2012, with
 * gSLICr's 3 x 3 search), every superpixel is scored from the table acquire's tiles are scored from, and the
 * annotator answers a chosen superpixel with ONE label, its dominant one.  Three calls:
 *
 *   mdil_spx_slic    image -> the id map, the centres and the sums of the final assignment
 *   mdil_spx_table   stored label / q / target maps + an id map -> per superpixel [pixels, sum q, wrong, valid,
 *                    label counts] and the valid-target counts per class
 *   mdil_spx_apply   mdil_ripu_apply's rule with the region read through the id map and one answer per region
 *
 * A library of its own, beside libmdil_hip.so, libmdil_acquire.so and libmdil_ripu.so: nothing of the training
 * path or of the other add-ons is compiled into it or changed by it ("Superpixel"); no head code is
 * compiled into the library.  Conventions of include/mdil_ripu.h:
 *
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller; the library
 *     allocates nothing, keeps no state but the thread-local error text, and every call is re-entrant.
 *   - `stream` is a hipStream_t passed as void*; the work is enqueued there, no implicit sync.
 *   - return 0 on success, negative on error; every refusal comes before any launch;
 *     mdil_spx_last_error() gives thread-local text.
 *   - integers only after the colour quantisation of mdil_spx_slic: no other float is held anywhere.
 *     Counters are 64-bit integers ADDED to with integer atomics, never cleared (mdil_spx_slic's `sums`, a
 *     workspace, is WRITTEN): every output is the same bytes on every run, whatever the grid.
 *
 * Limits of all three calls: maps are [N][H][W] with 1 <= H, W <= 4096 and at most 2^40 pixels in all;
 * 2 <= nc <= 32; every base pointer 8-byte aligned (rows need no alignment).
 *
 * What is simplified: the colour space is the RGB codes below, not CIELAB; there is no connectivity
 * enforcement, so a superpixel may be disconnected; there is no gradient perturbation of the first centres.
 */
#ifndef MDIL_SPX_H
#define MDIL_SPX_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDIL_SPX_OK 0
#define MDIL_SPX_ERR_INVALID (-1)
#define MDIL_SPX_ERR_LAUNCH (-2)

#define MDIL_SPX_MIN_CLASSES 2
#define MDIL_SPX_MAX_CLASSES 32
#define MDIL_SPX_MAX_PIXELS (1LL << 40)
#define MDIL_SPX_MAX_SIDE 4096               /* of H and of W */
#define MDIL_SPX_MIN_STEP 4
#define MDIL_SPX_MAX_STEP 64
#define MDIL_SPX_MIN_COMPACTNESS 1
#define MDIL_SPX_MAX_COMPACTNESS 64
#define MDIL_SPX_MAX_ITERATIONS 32
#define MDIL_SPX_MAX_CELLS (1LL << 31)       /* of `table`: N * K * (4 + nc) */
#define MDIL_SPX_FRACTION_BITS 4             /* a centre's state is in 1/16 of a pixel and of a colour code */
#define MDIL_SPX_FIELDS 4                    /* pixels, sum q, wrong, valid: acquire's */

int mdil_spx_version(void);
const char* mdil_spx_last_error(void);

/* The over-segmentation.  S = step in [4, 64], m = compactness in [1, 64], T = iterations in [0, 32].
 *
 * Colour code.  Of every value v of the image:  c8 = (uint32) fmaf(min(max(v, 0), 1), 255.0f, 0.5f), a NaN
 * taken as 0.  After this everything is an integer; (r, g, b) are the codes of a pixel's three channels.
 *
 * Grid.  Gy = ceil(H / S), Gx = ceil(W / S), K = Gy * Gx.  Centre k = gy * Gx + gx starts at the pixel
 * (y0, x0) = (min(H-1, gy*S + S/2), min(W-1, gx*S + S/2)); its state (Y, X, R, G, B) is 16 x that pixel's
 * position and colour codes (four fractional bits).  There is no gradient perturbation.
 *
 * Assign.  Pixel (y, x) has the home cell (y / S, x / S); its candidates are the centres of the 3 x 3 cells
 * around the home cell that lie inside the grid (gSLICr's search).  In unsigned 64-bit integers
 *      D(k) = S^2 * [(16r-R)^2 + (16g-G)^2 + (16b-B)^2] + m^2 * [(16y-Y)^2 + (16x-X)^2]
 * which is SLIC's dc^2 + (m/S)^2 ds^2 multiplied by S^2 (and by 256); it stays below 2^39.  The smallest D
 * wins; ties go to the lowest k.
 *
 * Update.  Over a centre's n pixels each of the five values becomes (16 * sum + n / 2) / n with floor
 * divisions (half up); a centre with n = 0 keeps its state.
 *
 * Schedule.  Init; T times: assign, then update; a final assign.
 *   image    f32 [N][3][H][W]       the network's input in [0, 1]
 *   id       i32 [N][H][W]          written: every pixel's k of the final assign.  During the call it holds
 *                                   the pixels' colour codes (r | g << 8 | b << 16)
 *   centres  i32 [N][K][5]          written: the state (Y, X, R, G, B) that the final assign read
 *   sums     i64 [N][K][6]          caller workspace, written and not added to: on return
 *                                   (n, sum y, sum x, sum r, sum g, sum b) of the final assignment
 * All three are required.  The assign is fused with the accumulation of the next update's sums. */
int mdil_spx_slic(const float* image, int N, int H, int W, int step, int compactness, int iterations, int* id,
                  int* centres, long long* sums, void* stream);

/* What every score is computed from, over STORED maps (mdil_acquire_head's `label` and `qmap`) and any id
 * map; K >= 1 superpixels per image.  A pixel whose id lies outside [0, K) counts in bad_ids and nowhere else.
 * For every other pixel, with s = id and F = 4 + nc:
 *      table[n][s][0] += 1                       pixels
 *      table[n][s][1] += q                       sum q
 *      table[n][s][2] += 1 where the target is valid (target < nc and != ignore_index) and label != target
 *      table[n][s][3] += 1 where the target is valid
 *      table[n][s][4 + label] += 1               a label >= nc counts in pixels and in no class
 *      tcount[n][s][target] += 1 where the target is valid
 *   label  u8  [N][H][W]
 *   qmap   u16 [N][H][W]
 *   target u8  [N][H][W] or NULL;  -1 <= ignore_index <= 255 (-1: none)
 *   id     i32 [N][H][W]
 * Outputs, all ADDED to; each may be NULL, but not all of them:
 *   table       i64 [N][K][4 + nc]    at most 2^31 cells
 *   tcount      i64 [N][K][nc]        needs a target
 *   bad_targets i64 [1]               += pixels whose target is >= nc and not ignore_index; needs a target
 *   bad_ids     i64 [1]
 * Correct for any id map in range; fast where ids are local (SLIC's): the adds of a work-group meet in LDS. */
int mdil_spx_table(const unsigned char* label, const unsigned short* qmap, const unsigned char* target, int ignore_index,
                   const int* id, int N, int H, int W, int K, int nc, long long* table, long long* tcount,
                   long long* bad_targets, long long* bad_ids, void* stream);

/* mdil_ripu_apply's rule with the region read through the id map.  A pixel is CHOSEN iff its id lies in
 * [0, K) and selected[n][id] == 255.  0 <= drop_id <= 255.  For every pixel
 *   chosen:                                        out = answer[n][id] if `answer` is given, else target if
 *                                                  given, else drop_id;                     mask = 255
 *   else, previous given and previous != drop_id:  out = previous;                          mask = 128
 *   else, fill given and fill != drop_id:          out = fill;                              mask = 64
 *   else:                                          out = drop_id;                           mask = 0
 *   id       i32 [N][H][W]
 *   selected u8  [N][K];  answer u8 [N][K] or NULL
 *   target, previous, fill, label u8 [N][H][W] or NULL
 * Outputs; each may be NULL, but not all of them:
 *   out, mask   u8 [N][H][W]
 *   shown       i64 [1]     += chosen pixels
 *   annotated   i64 [nc]    [c] += chosen pixels whose out is c, c < nc and c != ignore_index; needs an answer
 *                           or a target (without an answer: mdil_ripu_apply's count)
 *   kept        i64 [nc]    [c] += pixels kept from previous (mask 128) with previous == c < nc
 *   filled      i64 [nc]    [c] += pixels filled (mask 64) with fill == c < nc
 *   bad_targets i64 [1]     += chosen pixels whose target is >= nc and not ignore_index; needs a target
 *   wrong_shown i64 [1]     += chosen pixels with a valid target and label != target; needs target and label
 *   wrong_all   i64 [1]     += the same over every pixel; needs target and label
 *   noisy       i64 [1]     += chosen pixels with a valid target and out != target: the label noise of one-click
 *                           answers; needs a target
 *   bad_ids     i64 [1]     += pixels whose id lies outside [0, K): never chosen, otherwise treated as any pixel */
int mdil_spx_apply(const int* id, const unsigned char* selected, const unsigned char* answer, const unsigned char* target,
                   const unsigned char* previous, const unsigned char* fill, const unsigned char* label, int N, int H, int W,
                   int K, int nc, int ignore_index, int drop_id, unsigned char* out, unsigned char* mask, long long* shown,
                   long long* annotated, long long* kept, long long* filled, long long* bad_targets, long long* wrong_shown,
                   long long* wrong_all, long long* noisy, long long* bad_ids, void* stream);

#ifdef __cplusplus
}
#endif
#endif
