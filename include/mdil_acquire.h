/*
 * libmdil_acquire.so -- C ABI of the acquisition add-on: which regions of a new domain should be
 * labelled first?  Region-based active learning over fixed tiles (Mackowiak et al., CEREALS, BMVC 2018)
 * with the criteria of Xie et al. (RIPU, CVPR 2022): per tile the mean prediction uncertainty, the
 * impurity of the predicted labels and their product.  Two entry points:
 *
 *   mdil_acquire_head   Decoder.output_conv (ConvTranspose2d(16, nc, 2, stride 2)) fused with the softmax,
 *                       one uncertainty per pixel quantised LINEARLY to 16 bits, and per tile of the
 *                       label grid the integer table that every tile score is computed from; the
 *                       logits are never stored.
 *   mdil_acquire_apply  over stored maps: the label map an annotator of the selected tiles would hand
 *                       back (on top of an earlier round's and of fill labels), the mask of where each
 *                       label came from, and the counters of what was shown and annotated.
 *
 * A library of its own, beside libmdil_hip.so: nothing of the training path is compiled into it
 * or changed by it ("Acquire").  Same conventions as include/mdil_audit.h:
 *
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller; the
 *     library allocates nothing, keeps no state but the thread-local error text, and every call is
 *     re-entrant.
 *   - `stream` is a hipStream_t passed as void*; the work is enqueued there, no implicit sync.
 *   - return 0 on success, negative on error; every refusal comes before any launch;
 *     mdil_acquire_last_error() gives thread-local text.
 *   - the softmax is fp32 on the VALU; everything after the 16-bit q is integer arithmetic.
 *     Counters are 64-bit integers ADDED to with integer atomics, never cleared: every output is
 *     the same bytes on every run, whatever the grid.
 */
#ifndef MDIL_ACQUIRE_H
#define MDIL_ACQUIRE_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDIL_ACQUIRE_OK 0
#define MDIL_ACQUIRE_ERR_INVALID (-1)
#define MDIL_ACQUIRE_ERR_LAUNCH (-2)

#define MDIL_ACQUIRE_MIN_CLASSES 2
#define MDIL_ACQUIRE_MAX_CLASSES 32
#define MDIL_ACQUIRE_MAX_PIXELS (1LL << 40)
#define MDIL_ACQUIRE_MAX_CELLS (1LL << 31)   /* cells of a tile table: N * Ty * Tx * (4 + nc) */
#define MDIL_ACQUIRE_MIN_TILE 2
#define MDIL_ACQUIRE_MAX_TILE 256
#define MDIL_ACQUIRE_Q_ONE 65536             /* q = min(65535, floor(max(u, 0) * 65536)) */
#define MDIL_ACQUIRE_KINDS 3
#define MDIL_ACQUIRE_MSP 0
#define MDIL_ACQUIRE_ENTROPY 1
#define MDIL_ACQUIRE_MARGIN 2
#define MDIL_ACQUIRE_TILE_FIELDS 4           /* pixels, sum of q, wrong, with a valid target; then nc label counts */

int mdil_acquire_version(void);
const char* mdil_acquire_last_error(void);

/* x [N][H][W][16] fp32 (NHWC decoder features, 16-byte aligned), w [16][nc][2][2] and bias [nc]
 * (the ConvTranspose2d parameters in PyTorch's layout), 2 <= nc <= 32.  A tile is th x tw pixels of the
 * label grid [2H][2W], th and tw EVEN and in [2, 256]: the four outputs of one feature pixel fall into
 * one tile.  Ty = ceil(2H / th), Tx = ceil(2W / tw); the last row and column of tiles may be ragged.
 *
 * For every output pixel (n, 2h+a, 2w+b), by the chain include/mdil_route.h spells out for
 * mdil_route_head (same bits):
 *      l_c = bias[c] + sum_ci x[n,h,w,ci] * w[ci][c][a][b]   (fp32 FMA chain, bias first, ci ascending)
 *      label = argmax_c l_c; ties go to the lowest class, the first NaN wins;  m = max_c l_c
 *      d_c = l_c - m, and for d_c = -inf the largest negative float
 *      e_c = exp2(d_c * log2(e))                       (one hardware exp2 per class)
 *      s   = sum_c e_c,  A = sum_c e_c d_c             (c ascending, A as an FMA chain)
 *      conf   = 1 / s,  ent = log s - (A conf),  margin = conf (1 - e2),  e2 = max of e_c over c != label
 * and then ONE uncertainty u, chosen by `kind`:
 *      0 msp      u = (s - 1.0f) * conf                (= 1 - p_top; mdil_openset_head's kind 0)
 *      1 entropy  u = ent * inv_log_nc                 (inv_log_nc: a float argument, meant to be float32(1 / ln nc))
 *      2 margin   u = 1.0f - margin
 *      q = min(65535, (uint32)(max(u, 0.0f) * 65536.0f))
 * The code is LINEAR in u, so sums of q mean something.  inv_log_nc must be finite and >= 0; it is read
 * with kind 1 only.  A pixel whose s or m is not finite adds 1 to nonfinite[0], gets q = 0 in `qmap`,
 * its label in `label`, and enters no tile field.
 *
 * target u8 [N][2H][2W] (2-byte aligned) or NULL; -1 <= ignore_index <= 255 (-1: none).  A pixel is
 * VALID when there is a target, target < nc and target != ignore_index.  A target >= nc that is not
 * ignore_index adds 1 to bad_targets[0] (whether or not the pixel is finite) and counts nowhere else.
 *
 * Outputs; each may be NULL (not written / not added to), but not all of them:
 *   label       u8  [N][2H][2W]            2-byte aligned
 *   qmap        u16 [N][2H][2W]            4-byte aligned
 *   tiles       i64 [N][Ty][Tx][4 + nc]    ADDED to, over the FINITE pixels of the tile:
 *                 [0]      pixels
 *                 [1]      sum of q
 *                 [2]      pixels with a valid target whose label differs from it
 *                 [3]      pixels with a valid target
 *                 [4 + c]  pixels labelled c
 *               [2] and [3] need a target: without one they are not touched.  The table may hold at
 *               most 2^31 cells.
 *   nonfinite   i64 [1]
 *   bad_targets i64 [1]                    needs a target (refused without one)
 * All counters 8-byte alignment. */
int mdil_acquire_head(const float* x, const float* w, const float* bias, int N, int H, int W, int nc, int th, int tw,
                      int kind, float inv_log_nc, const unsigned char* target, int ignore_index, unsigned char* label,
                      unsigned short* qmap, long long* tiles, long long* nonfinite, long long* bad_targets,
                      void* stream);

/* Maps u8 [N][Hl][Wl], any Hl, Wl >= 1 and at most 2^40 pixels in all; tiles as above over [Hl][Wl]:
 * Ty = ceil(Hl / th), Tx = ceil(Wl / tw), th and tw even and in [2, 256].
 *   selected u8 [N][Ty][Tx]   non-zero: the tile is chosen
 *   target   u8 or NULL       what the annotator answers inside a chosen tile
 *   previous u8 or NULL       an earlier round's label map; previous == drop_id means "no label yet"
 *   fill     u8 or NULL       labels for what is still empty, pseudo-labels for instance
 * 0 <= drop_id <= 255; nc and ignore_index as above, used by the counters alone.  For every pixel
 *   in a chosen tile:   out = target if given, else drop_id;                        mask = 255
 *   else, previous given and previous != drop_id:  out = previous;                  mask = 128
 *   else, fill given and fill != drop_id:          out = fill;                      mask = 64
 *   else:                                          out = drop_id;                   mask = 0
 * Outputs; each may be NULL, but not all of them:
 *   out, mask   u8 [N][Hl][Wl]   8-byte aligned
 *   shown       i64 [1]          += pixels in chosen tiles
 *   annotated   i64 [nc]         [c] += pixels in chosen tiles whose target is valid and c; needs a target
 *   kept        i64 [nc]         [c] += pixels kept from previous (mask 128) with previous == c < nc
 *   filled      i64 [nc]         [c] += pixels filled (mask 64) with fill == c < nc
 *   bad_targets i64 [1]          += pixels in chosen tiles whose target is >= nc and not ignore_index; needs a target
 * target, previous, fill, out and mask need 8-byte alignment (a lane handles 8 consecutive pixels; row
 * ends and tile borders may fall inside them), the counters too. */
int mdil_acquire_apply(const unsigned char* selected, const unsigned char* target, const unsigned char* previous,
                       const unsigned char* fill, int N, int Hl, int Wl, int th, int tw, int nc, int ignore_index,
                       int drop_id, unsigned char* out, unsigned char* mask, long long* shown, long long* annotated,
                       long long* kept, long long* filled, long long* bad_targets, void* stream);

#ifdef __cplusplus
}
#endif
#endif
