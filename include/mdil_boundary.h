/*
 * libmdil_boundary.so -- C ABI of the boundary add-on: for two label maps of the labels' own size
 * (a prediction and its ground truth) the distance of every pixel to its region's contour, binned
 * by up to 8 band widths, and the counters from which boundary IoU (Cheng et al., CVPR 2021) and
 * trimap mIoU are derived.  A pure integer kernel: every output is exact.
 *
 * An eighth add-on library, beside libmdil_hip.so and the seven others: nothing of them is
 * compiled into it or changed by it ("Boundary quality").  Same conventions as
 * include/mdil_fullres.h:
 *
 *   - plain pointers and sizes only; every pointer but `widths` is DEVICE memory owned by the
 *     caller; the library allocates nothing, keeps no state but the thread-local error text, and
 *     every call is re-entrant.
 *   - `stream` is a hipStream_t passed as void*; the work is enqueued there, no implicit sync.
 *   - return 0 on success, negative on error; mdil_boundary_last_error() gives thread-local text.
 *   - every argument check answers before any launch.
 */
#ifndef MDIL_BOUNDARY_H
#define MDIL_BOUNDARY_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDIL_BOUNDARY_OK 0
#define MDIL_BOUNDARY_ERR_INVALID (-1)
#define MDIL_BOUNDARY_ERR_LAUNCH (-2)

#define MDIL_BOUNDARY_MIN_CLASSES 2
#define MDIL_BOUNDARY_MAX_CLASSES 32
#define MDIL_BOUNDARY_MAX_SIZE (1 << 22)          /* H and W */
#define MDIL_BOUNDARY_MAX_PIXELS (1LL << 40)      /* N*H*W */
#define MDIL_BOUNDARY_MAX_WIDTHS 8
#define MDIL_BOUNDARY_MAX_WIDTH 128

int mdil_boundary_version(void);
const char* mdil_boundary_last_error(void);

/* Bytes of workspace a call on [N][H][W] maps needs: 2*N*H*W (the capped horizontal run distances
 * of both maps) rounded up to a multiple of 16; -1 for sizes the call refuses. */
long long mdil_boundary_workspace_bytes(int N, int H, int W);

/* pred and target: u8 [N][H][W] label maps, any byte value is a label.  For a map L, d(L, p) is
 * the Chebyshev distance from pixel p to the nearest pixel whose label differs from L[p] or that
 * lies outside its image (so d >= 1, and the images of a batch never see each other): d <= k iff k
 * iterations of 3x3 erosion with a zero border remove p from its own label's mask.
 *
 * widths (HOST memory, read before the call returns): n_widths in [1, 8] strictly increasing
 * integers in [1, 128]; cap = widths[n_widths - 1], nb = n_widths + 1 bins: bin k < nb - 1 holds
 * widths[k-1] < d <= widths[k] (0 for widths[-1]), the last bin d > cap.
 *
 * With dt = d(target, p), dp = d(pred, p), g = target[p], q = pred[p]:
 *   g == ignore_index                 the pixel adds to nothing (-1 ignores nothing)
 *   else g >= nc                      bad_targets[0] += 1, nothing else
 *   else q >= nc                      bad_preds[0] += 1, nothing else
 *   else    target_hist [nc][nb]      [g][bin(dt)] += 1
 *           pred_hist   [nc][nb]      [q][bin(dp)] += 1
 *           both_hist   [nc][nb]      [g][bin(max(dt, dp))] += 1   when g == q
 *           confusion   [nb][nc][nc]  [bin(dt)][g][q] += 1
 * All six counters are i64, required, and ADDED to, never cleared.  The ignore label is a label
 * like any other where distances are formed.
 *
 * dist_pred and dist_target (u8 [N][H][W], either may be NULL) receive min(d, cap + 1).
 * workspace: at least mdil_boundary_workspace_bytes(N, H, W) bytes, overwritten.
 * The maps, the distance maps and the workspace need 4-byte alignment, the counters 8-byte. */
int mdil_boundary_count(const unsigned char* pred, const unsigned char* target, int N, int H, int W, int nc,
                        const int* widths, int n_widths, int ignore_index,
                        unsigned char* workspace, long long workspace_bytes,
                        unsigned char* dist_pred, unsigned char* dist_target,
                        long long* target_hist, long long* pred_hist, long long* both_hist,
                        long long* confusion, long long* bad_targets, long long* bad_preds, void* stream);

#ifdef __cplusplus
}
#endif
#endif
