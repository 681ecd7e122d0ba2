/*
 * libmdil_density.so -- C ABI of the density add-on: open-set scores in FEATURE space.  The four
 * scores of libmdil_openset.so are functions of the head's nc logits; what the 16 -> nc projection
 * discards is invisible to them.  Here every feature row is scored against class-conditional
 * Gaussians with one tied covariance (Lee et al., NeurIPS 2018; "embedding density" in Fishyscapes),
 * in the relative form of Ren et al. (2021) as well, and the nearest class mean comes out of the same
 * distances (the nearest-class-mean classifier of iCaRL).  Two entry points:
 *
 *   mdil_density_head   the penultimate layer (16 channels): Decoder.output_conv + argmax fused with
 *                       both scores of the feature pixel, from the same registers
 *   mdil_density_rows   any layer: feature rows [rows][C], C a multiple of 16 up to 128; the whitening
 *                       runs on the fp32 MFMA
 *
 * A library of its own, beside libmdil_hip.so ("Density").  The conventions are those of
 * include/mdil_openset.h: device pointers only, owned by the caller; the library allocates nothing and
 * keeps no state but the thread-local error text; `stream` is a hipStream_t passed as void*; 0 on
 * success, negative on error, every refusal before any launch; counters are 64-bit integers ADDED to
 * with integer atomics, never cleared, so equal inputs give equal bytes.
 *
 * The model: fp32 [MDIL_DENSITY_MODEL_FLOATS(C, K)] on the device, prepared by the host in fp64, and
 * `cls` u8 [K], the class id of mean k, ascending, 1 <= K <= 32:
 *      pivot [C] | A [C][C] | A0 [C][C] | m0 [C] | m [K][C]
 * A is the inverse Cholesky factor of the tied covariance (row-major, ZEROS above the diagonal: the
 * kernels may or may not read them), m[k] = A (mu_k - pivot) the whitened class means; A0 and m0 the same for the single
 * Gaussian fitted to all rows.  Per feature row x, in fp32:
 *      w    = x - pivot
 *      z    = A w,  z0 = A0 w                     (FMA chains over j ascending)
 *      d_k  = sum_i (z_i - m_k,i)^2,  d0 = sum_i (z0_i - m0_i)^2      (differences, never the expanded form)
 *      maha    = min_k d_k + 0.0f                 kind 0
 *      rmaha   = (min_k d_k - d0) + 0.0f          kind 1
 *      nearest = cls[argmin_k d_k]                ties to the lowest k
 * Higher = more likely unknown.  The 16-bit code of a score is mdil_openset.h's key.  A row of which
 * any d_k or d0 is not finite gets code 65535 and nearest 255, is counted in nonfinite[0] and enters
 * no histogram.
 *
 * Groups as in mdil_openset_head: 0 known, 1 unknown, anything else ignored.
 */
#ifndef MDIL_DENSITY_H
#define MDIL_DENSITY_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDIL_DENSITY_OK 0
#define MDIL_DENSITY_ERR_INVALID (-1)
#define MDIL_DENSITY_ERR_LAUNCH (-2)

#define MDIL_DENSITY_MIN_CLASSES 2
#define MDIL_DENSITY_MAX_CLASSES 32
#define MDIL_DENSITY_MAX_MEANS 32
#define MDIL_DENSITY_MAX_PIXELS (1LL << 40)
#define MDIL_DENSITY_MAX_ROWS (1LL << 24)
#define MDIL_DENSITY_MAX_CHANNELS 128
#define MDIL_DENSITY_KINDS 2          /* 0 maha, 1 rmaha */
#define MDIL_DENSITY_CODES 65536
#define MDIL_DENSITY_NONFINITE_CODE 65535
#define MDIL_DENSITY_NO_CLASS 255
#define MDIL_DENSITY_MODEL_FLOATS(C, K) (2 * (C) + 2 * (C) * (C) + (K) * (C))

int mdil_density_version(void);
const char* mdil_density_last_error(void);

/* x [N][H][W][16] fp32 (16-byte aligned), w [16][nc][2][2] and bias [nc] as in mdil_openset_head,
 * 2 <= nc <= 32; model (4-byte aligned) and cls for C = 16.  `label` is mdil_predict_head's, bit for
 * bit (the same chain through the same helpers).  The scores belong to the FEATURE pixel; its four
 * output pixels (n, 2h+a, 2w+b) share them.  target u8 [N][2H][2W] (2-byte aligned) or NULL;
 * g = target ? group_lut[target[pixel]] : const_group.
 * Outputs; each may be NULL, but not all of them:
 *   label     u8  [N][2H][2W]     2-byte aligned
 *   nearest   u8  [N][2H][2W]     2-byte aligned; the feature pixel's value at its four output pixels
 *   code      u16 [N][2H][2W]     4-byte aligned; the code of kind `map_kind` (0, 1; -1 exactly when code is
 *                                 NULL), replicated likewise, so mdil_openset_apply reads label + code unchanged
 *   hist      i64 [2][2][65536]   hist[k][g][code_k] += 1 per OUTPUT pixel, under its own target's group, for
 *                                 every kind k of the bit mask `kinds` (1..3; checked with or without a hist)
 *   nonfinite i64 [1]             += 4 per feature pixel that is not finite (its output pixels)
 *   agree     i64 [2]             [0] += output pixels of group 0, [1] += those of them with nearest == label
 * hist, nonfinite and agree need 8-byte alignment. */
int mdil_density_head(const float* x, const float* w, const float* bias, int N, int H, int W, int nc,
                      const float* model, const unsigned char* cls, int K, const unsigned char* target,
                      const unsigned char* group_lut, int const_group, int kinds, int map_kind,
                      unsigned char* label, unsigned char* nearest, unsigned short* code, long long* hist,
                      long long* nonfinite, long long* agree, void* stream);

/* x [rows][C] fp32, contiguous, 16-byte aligned; C a multiple of 16 in [16, 128]; 1 <= rows <= 2^24;
 * model and cls for that C.  z and z0 are formed by v_mfma_f32_16x16x4_f32 (exact fp32 FMA chains over
 * j ascending, the zero tiles above the diagonal skipped; the tiles of A and A0 on and below it are
 * staged in LDS once per work-group).  group u8 [rows] (0, 1, anything else) or
 * NULL with const_group.
 * Outputs; each may be NULL, but not all of them:
 *   nearest   u8  [rows]
 *   code      u16 [rows]          2-byte aligned; kind `map_kind` (-1 exactly when NULL)
 *   hist      i64 [2][2][65536]   one count per row, as above
 *   nonfinite i64 [1]             += 1 per row that is not finite */
int mdil_density_rows(const float* x, long long rows, int C, const float* model, const unsigned char* cls, int K,
                      const unsigned char* group, int const_group, int kinds, int map_kind,
                      unsigned char* nearest, unsigned short* code, long long* hist, long long* nonfinite,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
