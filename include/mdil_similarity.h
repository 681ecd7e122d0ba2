/*
 * libmdil_similarity.so -- C ABI of the representation-similarity add-on: the first and second
 * moments of feature rows of one or two populations, with labels, from which linear CKA, the
 * Frechet distance, per-class centroid shifts and class separability follow by small fp64 algebra
 * on the host (mdil_ss_amd/similarity.py).
 *
 * A seventh library, beside libmdil_hip.so and the other add-ons: nothing of any of them is
 * compiled into it or changed by it ("Similarity").  Same conventions as
 * include/mdil_tsne.h:
 *
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller; the
 *     library allocates nothing, keeps no state but the thread-local error text, and every call is
 *     re-entrant (on different states and workspaces).
 *   - `stream` is a hipStream_t passed as void*; the work is enqueued there, no implicit sync and
 *     no host synchronisation inside any call.
 *   - return 0 on success, negative on error; mdil_sim_last_error() gives thread-local text.
 *   - no float atomics: every reduction runs in a fixed order, so equal inputs give equal bits.
 */
#ifndef MDIL_SIMILARITY_H
#define MDIL_SIMILARITY_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDIL_SIM_OK 0
#define MDIL_SIM_ERR_INVALID (-1)
#define MDIL_SIM_ERR_LAUNCH (-2)

#define MDIL_SIM_MAX_CX 128
#define MDIL_SIM_MAX_CY 128
#define MDIL_SIM_MAX_CLASSES 32
#define MDIL_SIM_MAX_ROWS 16777216
/* Rows one fp32 accumulation chain covers at most; after that the partial is summed in fp64. */
#define MDIL_SIM_CHAIN 1024

int mdil_sim_version(void);
const char* mdil_sim_last_error(void);

/* Bytes of `state` for cx, cy channels and nc classes: fp64, in this order
 *      n[nc]          rows of each class
 *      skipped        rows whose label was >= nc
 *      sx[nc][cx]     per-class sums of w_x
 *      sy[nc][cy]     per-class sums of w_y
 *      gxx[cx][cx]    sum of w_x^T w_x   (whole; the two triangles are bit-identical)
 *      gyy[cy][cy]    sum of w_y^T w_y   (whole; the two triangles are bit-identical)
 *      gxy[cx][cy]    sum of w_x^T w_y
 * with w_x = fl32(x - pivot_x) and w_y = fl32(y - pivot_y), rows with a label >= nc left out.
 * -1 when cx is outside [1, 128], cy outside [0, 128] or nc outside [1, 32]. */
long long mdil_sim_state_bytes(int cx, int cy, int nc);

/* Bytes of `workspace` of one mdil_sim_accumulate call on `rows` rows; -1 when an argument is
 * outside its limits (rows: 1 to MDIL_SIM_MAX_ROWS). */
long long mdil_sim_workspace_bytes(long long rows, int cx, int cy, int nc);

/* Adds the moments of `rows` feature rows to `state` (fp64, zeroed by the caller before the first
 * call, accumulated into across calls).
 *      x       f32 [rows][cx], contiguous
 *      y       f32 [rows][cy], contiguous; NULL exactly when cy == 0 (one population)
 *      labels  u8 [rows] or NULL; NULL needs nc == 1 and puts every row in class 0.  A row whose
 *              label is >= nc adds to `skipped` and to nothing else.
 *      pivot_x f32 [cx], pivot_y f32 [cy] (NULL exactly when cy == 0): subtracted from every row
 *              in fp32 before anything is accumulated; the caller undoes the shift in fp64.
 * Every product is formed and summed by the exact-fp32 matrix instruction, in row order, in chains
 * of at most MDIL_SIM_CHAIN rows; the chains' partials are added in fp64 in a fixed order: an
 * entry is within (MDIL_SIM_CHAIN + 2) 2^-24 sum |w_a| |w_b| of the exact value, exact when every
 * partial sum is representable in fp32, and the same call on the same input gives the same bits.
 * x, y, state and workspace 16-byte aligned, the pivots 4-byte; state and workspace must overlap
 * neither each other nor any input.  workspace: mdil_sim_workspace_bytes(rows, cx, cy, nc). */
int mdil_sim_accumulate(const float* x, const float* y, const unsigned char* labels, long long rows,
                        int cx, int cy, int nc, const float* pivot_x, const float* pivot_y,
                        double* state, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
