/*
 * libmdil_ripu.so -- C ABI of the sliding-region acquisition add-on: RIPU as published (Xie et al.,
 * "Towards Fewer Annotations: Active Learning via Region Impurity and Prediction Uncertainty", CVPR 2022).
 * Every pixel is scored by the uncertainty and the label impurity of the (2k+1)^2 window CENTRED on it, and
 * the best centres are picked greedily, each taking its (2r+1)^2 region out of the pool (r = k: region mode,
 * "RA"; r = 0: pixel mode, "PA").  libmdil_acquire.so ranks the tiles of a fixed grid instead.  Three calls,
 * all over STORED maps (mdil_acquire_head's `label` and `qmap`); no head code is compiled into the library:
 *
 *   mdil_ripu_score    label + q maps -> one 32-bit integer key per pixel, from its clipped window
 *   mdil_ripu_select   keys -> the greedy picks of every image under a pixel budget, and the `taken` map
 *   mdil_ripu_apply    the `taken` map + stored maps -> the label map an annotator of the picked regions hands
 *                      back (on top of an earlier round's and of fill labels), its mask and its counters
 *
 * A library of its own, beside libmdil_hip.so and libmdil_acquire.so: nothing of the training path or of
 * the tile add-on is compiled into it or changed by it ("Ripu").  Conventions of
 * include/mdil_acquire.h:
 *
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller; the library
 *     allocates nothing, keeps no state but the thread-local error text, and every call is re-entrant.
 *   - `stream` is a hipStream_t passed as void*; the work is enqueued there, no implicit sync.
 *   - return 0 on success, negative on error; every refusal comes before any launch;
 *     mdil_ripu_last_error() gives thread-local text.
 *   - integers only: the library holds no float and no logarithm (the caller hands the table of h ln h in).
 *     Counters are 64-bit integers ADDED to with integer atomics, never cleared: every output is the same
 *     bytes on every run, whatever the grid.
 *
 * Limits of all three calls: maps are [N][Hl][Wl] with any Hl, Wl >= 1, at most 2^24 pixels per image and
 * 2^40 pixels in all; 2 <= nc <= 32; every base pointer 8-byte aligned (rows need no alignment).
 */
#ifndef MDIL_RIPU_H
#define MDIL_RIPU_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDIL_RIPU_OK 0
#define MDIL_RIPU_ERR_INVALID (-1)
#define MDIL_RIPU_ERR_LAUNCH (-2)

#define MDIL_RIPU_MIN_CLASSES 2
#define MDIL_RIPU_MAX_CLASSES 32
#define MDIL_RIPU_MAX_PIXELS (1LL << 40)
#define MDIL_RIPU_MAX_IMAGE_PIXELS (1 << 24)
#define MDIL_RIPU_MIN_RADIUS 1               /* of the score window */
#define MDIL_RIPU_MAX_RADIUS 32              /* of the score window and of the selected region */
#define MDIL_RIPU_MAX_PICKS 65536
#define MDIL_RIPU_TLOG_SHIFT 14              /* tlog[h] = round(h ln h * 2^14) */
#define MDIL_RIPU_CRITERIA 5
#define MDIL_RIPU_UNCERTAINTY 0
#define MDIL_RIPU_IMPURITY 1
#define MDIL_RIPU_RIPU 2
#define MDIL_RIPU_ORACLE 3
#define MDIL_RIPU_RANDOM 4
#define MDIL_RIPU_STOP_EMPTY 0               /* no pixel left, or the best key left is 0 */
#define MDIL_RIPU_STOP_BUDGET 1
#define MDIL_RIPU_STOP_PICKS 2

int mdil_ripu_version(void);
const char* mdil_ripu_last_error(void);

/* The window of pixel p = (y, x) is Wd(p) = {(y', x') : |y' - y| <= k, |x' - x| <= k} clipped to the image
 * (nothing is padded), 1 <= k <= 32.  Over it:
 *      cnt = |Wd(p)|                           (closed form)
 *      h_c = pixels of Wd with label == c      (a label >= nc counts in cnt and in no h_c)
 *      sq  = sum of q over Wd
 *      wr  = pixels of Wd with a valid target (target < nc and != ignore_index) and label != target
 *      E   = max(0, tlog[cnt] - sum_c tlog[h_c])
 * tlog i32 [(2k+1)^2 + 1] is meant to be round(h ln h * 2^14) with tlog[0] = tlog[1] = 0, built by the caller
 * in fp64; it is read as it is (entries in [0, 2^30] keep every product below inside 64 bits).  The key, in
 * 64-bit integers with floor division, saturated at 2^32 - 1:
 *      by 0 uncertainty  (sq << 16) / cnt
 *      by 1 impurity     (E << 16) / cnt
 *      by 2 ripu         (sq * E) / (cnt * cnt)        = 65536 * 2^14 * U * I * ln nc
 *      by 3 oracle       (wr << 32) / (cnt + 1)
 *      by 4 random       max(1, mix(mix(seed, image0 + n + 1), y * Wl + x + 1) >> 32)
 * mix(s, j) is SplitMix64's finaliser of s + 0x9E3779B97F4A7C15 * j (mdil_signif's generator).  A pixel with
 * taken != 0 gets key 0; it still counts in its neighbours' windows.
 *   label  u8  [N][Hl][Wl]
 *   qmap   u16 [N][Hl][Wl] or NULL    required for by 0 and 2
 *   target u8  [N][Hl][Wl] or NULL    required for by 3; -1 <= ignore_index <= 255 (-1: none)
 *   taken  u8  [N][Hl][Wl] or NULL
 *   tlog   i32 [(2k+1)^2 + 1] or NULL required for by 1 and 2
 *   key    u32 [N][Hl][Wl]            written
 * No buffer proportional to nc x pixels exists anywhere: the per-class window counts live in LDS. */
int mdil_ripu_score(const unsigned char* label, const unsigned short* qmap, const unsigned char* target,
                    int ignore_index, const unsigned char* taken, const int* tlog, int N, int Hl, int Wl, int nc, int k,
                    int by, long long seed, long long image0, unsigned int* key, void* stream);

/* The greedy pick, one work-group per image.  0 <= r <= 32, budget_pixels >= 0 (the same for every image),
 * 1 <= max_picks <= 65536.  Per image, starting from shown = 0, at most max_picks times:
 *   1. p* = the pixel with taken == 0 and the largest key; ties go to the lowest y * Wl + x
 *   2. stop (0) if there is no such pixel or key[p*] == 0
 *   3. fresh = pixels of the clipped (2r+1)^2 region around p* with taken == 0
 *   4. stop (1) if shown + fresh > budget_pixels
 *   5. those pixels get taken = 255, shown += fresh, and the pick is recorded
 * and stop (2) after max_picks picks.  Keys are NOT recomputed between picks (RIPU's rule).
 *   key    u32 [N][Hl][Wl]
 *   taken  u8  [N][Hl][Wl]            read and written; marks of an earlier round (any non-zero byte) stay
 * Outputs; each may be NULL:
 *   picks  i64 [N][max_picks][4]      (y, x, key, fresh) per pick; rows past the count are untouched
 *   count  i64 [N]                    written
 *   shown  i64 [N]                    written, not added to
 *   stop   i64 [N]                    written: why the image stopped, MDIL_RIPU_STOP_* */
int mdil_ripu_select(const unsigned int* key, unsigned char* taken, int N, int Hl, int Wl, int r, long long budget_pixels,
                     int max_picks, long long* picks, long long* count, long long* shown, long long* stop, void* stream);

/* mdil_acquire_apply's rule with a per-pixel mask instead of tiles.  A pixel is CHOSEN iff selected == 255
 * (mdil_ripu_select's marks; an earlier round's marks, 128 say, are not chosen again).  0 <= drop_id <= 255;
 * nc and ignore_index are used by the counters alone.  For every pixel
 *   chosen:                                        out = target if given, else drop_id;     mask = 255
 *   else, previous given and previous != drop_id:  out = previous;                          mask = 128
 *   else, fill given and fill != drop_id:          out = fill;                              mask = 64
 *   else:                                          out = drop_id;                           mask = 0
 *   selected u8 [N][Hl][Wl];  target, previous, fill, label u8 [N][Hl][Wl] or NULL
 * Outputs; each may be NULL, but not all of them:
 *   out, mask   u8 [N][Hl][Wl]
 *   shown       i64 [1]     += chosen pixels
 *   annotated   i64 [nc]    [c] += chosen pixels whose target is valid and c; needs a target
 *   kept        i64 [nc]    [c] += pixels kept from previous (mask 128) with previous == c < nc
 *   filled      i64 [nc]    [c] += pixels filled (mask 64) with fill == c < nc
 *   bad_targets i64 [1]     += chosen pixels whose target is >= nc and not ignore_index; needs a target
 *   wrong_shown i64 [1]     += chosen pixels with a valid target and label != target; needs target and label
 *   wrong_all   i64 [1]     += the same over every pixel; needs target and label */
int mdil_ripu_apply(const unsigned char* selected, const unsigned char* target, const unsigned char* previous,
                    const unsigned char* fill, const unsigned char* label, int N, int Hl, int Wl, int nc, int ignore_index,
                    int drop_id, unsigned char* out, unsigned char* mask, long long* shown, long long* annotated,
                    long long* kept, long long* filled, long long* bad_targets, long long* wrong_shown,
                    long long* wrong_all, void* stream);

#ifdef __cplusplus
}
#endif
#endif
