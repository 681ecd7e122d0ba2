/*
 * libmdil_segments.so -- C ABI of the segments add-on: a u8 label map seen as a set of objects.
 * Connected-component labelling of full-size label maps (4- or 8-connectivity) by a lock-free
 * union-find over pixels, the per-segment overlap with a second map binned by segment size (segment
 * recall / precision, missed and hallucinated segments), and a despeckle filter that removes
 * segments below a per-label area.  A pure integer kernel set: every output is exact and a function
 * of the input alone.
 *
 * An eleventh add-on library, beside libmdil_hip.so and the ten others: nothing of them is compiled
 * into it or changed by it ("Segments").  Same conventions as include/mdil_boundary.h:
 *
 *   - plain pointers and sizes only; every pointer but `edges` is DEVICE memory owned by the
 *     caller; the library allocates nothing, keeps no state but the thread-local error text, and
 *     every call is re-entrant.
 *   - `stream` is a hipStream_t passed as void*; the work is enqueued there, no implicit sync.
 *   - return 0 on success, negative on error; mdil_segments_last_error() gives thread-local text.
 *   - every argument check answers before any launch.
 *   - u8 maps, i32 maps, min_area and the workspace need 4-byte alignment, the i64 counters 8-byte.
 */
#ifndef MDIL_SEGMENTS_H
#define MDIL_SEGMENTS_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDIL_SEGMENTS_OK 0
#define MDIL_SEGMENTS_ERR_INVALID (-1)
#define MDIL_SEGMENTS_ERR_LAUNCH (-2)

#define MDIL_SEGMENTS_MIN_CLASSES 2
#define MDIL_SEGMENTS_MAX_CLASSES 32
#define MDIL_SEGMENTS_MAX_SIZE (1 << 15)          /* H and W: H*W <= 2^30, a root fits an i32 */
#define MDIL_SEGMENTS_MAX_PIXELS (1LL << 40)      /* N*H*W */
#define MDIL_SEGMENTS_MAX_EDGES 8
#define MDIL_SEGMENTS_MAX_EDGE (1 << 30)
#define MDIL_SEGMENTS_MAX_COVER_DEN 1000

int mdil_segments_version(void);
const char* mdil_segments_last_error(void);

/* Bytes of workspace the calls on [N][H][W] maps need: 8*N*H*W (the parents of the union-find in
 * mdil_segments_label; two i32 accumulators per pixel in mdil_segments_count) rounded up to a
 * multiple of 16; -1 for sizes the calls refuse. */
long long mdil_segments_workspace_bytes(int N, int H, int W);

/* map: u8 [N][H][W], any byte is a label.  Two pixels of one image are connected when a path of
 * pixels of their label joins them, each step to one of the 4 (connectivity 4) or 8 (connectivity 8)
 * neighbours inside the image: the images of a batch never see each other, and the last pixel of a
 * row is no neighbour of the first pixel of the next.  A segment is a maximal set of connected pixels.
 *   root [N][H][W] i32: the smallest y*W + x among the pixels of p's segment.
 *   area [N][H][W] i32: the segment's pixel count at its root pixel, 0 everywhere else (cleared
 *                       by the call).
 * workspace: at least mdil_segments_workspace_bytes(N, H, W) bytes, overwritten. */
int mdil_segments_label(const unsigned char* map, int N, int H, int W, int connectivity, int* root, int* area,
                        unsigned char* workspace, long long workspace_bytes, void* stream);

/* map, other: u8 [N][H][W]; root, area: those of `map` (mdil_segments_label).  nc in [2, 32];
 * map_ignore, other_ignore in [-1, 255], -1 ignores nothing.  edges (HOST memory, read before the
 * call returns): n_edges in [1, 8] strictly increasing integers in [1, 2^30]; nb = n_edges + 1 bins
 * of the area a: bin k < nb - 1 holds edges[k-1] < a <= edges[k] (0 for edges[-1]), the last bin
 * a > edges[n_edges - 1].  0 < cover_num <= cover_den <= 1000.
 *
 * For a segment s of `map` with label c and area a:  void_s = its pixels with other == other_ignore,
 * hit_s = its pixels with other == c, j_s = a - void_s, k = bin(a):
 *   c == map_ignore        the segment adds to nothing
 *   else c >= nc           bad_labels[0] += a, nothing else
 *   else j_s == 0          unjudged[c][k] += 1, nothing else
 *   else                   segments[c][k] += 1; pixels[c][k] += j_s; hit_pixels[c][k] += hit_s;
 *                          covered[c][k] += 1 when hit_s * cover_den >= cover_num * j_s;
 *                          missed[c][k] += 1 when hit_s == 0
 * The six [nc][nb] counters and bad_labels [1] are i64, required, and ADDED to, never cleared.
 *
 * hit and void_ (i32 [N][H][W], either may be NULL) receive hit_s and void_s at the roots and 0
 * everywhere else.  workspace: at least mdil_segments_workspace_bytes(N, H, W) bytes, overwritten. */
int mdil_segments_count(const unsigned char* map, const unsigned char* other, const int* root, const int* area,
                        int N, int H, int W, int nc, int map_ignore, int other_ignore, const int* edges,
                        int n_edges, int cover_num, int cover_den, unsigned char* workspace,
                        long long workspace_bytes, int* hit, int* void_, long long* segments, long long* pixels,
                        long long* hit_pixels, long long* covered, long long* missed, long long* unjudged,
                        long long* bad_labels, void* stream);

/* The despeckle filter.  min_area: i32 [256] (DEVICE), indexed by the label byte; keep_id in
 * [-1, 255]; fill in [0, 255].
 *   out[p] = fill    when map[p] != keep_id and area[root[p]] < min_area[map[p]]
 *   out[p] = map[p]  otherwise
 * removed_segments and removed_pixels (i64 [256], indexed by the label byte) are ADDED to.
 * out (u8 [N][H][W]) may not alias map. */
int mdil_segments_filter(const unsigned char* map, const int* root, const int* area, int N, int H, int W,
                         const int* min_area, int keep_id, int fill, unsigned char* out,
                         long long* removed_segments, long long* removed_pixels, void* stream);

#ifdef __cplusplus
}
#endif
#endif
