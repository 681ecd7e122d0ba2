// libmdil_segments.so: connected components of u8 label maps by a lock-free union-find over pixels,
// the per-segment overlap counters and the despeckle filter (gfx950; include/mdil_segments.h has
// the definitions).  Integers only: nothing is rounded, and every output is a function of the
// input alone -- the root of a segment is its smallest pixel index whatever order the atomics
// arrive in, and every sum is an integer sum.
//
// mdil_segments_label, three launches.  P is the parent array (i32 per pixel, in the workspace),
// indices are y*W + x inside the pixel's own image, and P[p] <= p always.
//
//   rows (segments_rows_kernel).  One wavefront owns a row and walks it in chunks of 256 pixels,
//   four per lane as one dword: the start s of the run of equal labels around x is the running
//   maximum of the positions where a run starts, the max-scan over the lanes that boundary.hip
//   uses, carried from chunk to chunk.  P[y*W + x] = y*W + s, area = 0.  Plain stores: the launch
//   boundary hands them to the next kernel.
//
//   merge (segments_merge_kernel).  A lane owns four adjacent pixels of a row y > 0 and looks at
//   the row above.  A vertical contact (the pixel above has the same label) joins two runs; where
//   the contact to the left joins the same two runs (left, above and above-left all carry the
//   label) it is skipped, so one union is issued per contact run, not per pixel.  With
//   8-connectivity a diagonal contact is issued only where no vertical contact already implies it:
//   above-left when neither the pixel above nor the one to the left has the label, above-right
//   likewise.  Every access to P in this launch is an agent-scope atomic: a relaxed
//   __hip_atomic_load (an L1-bypassing load: a plain load could be served by a line this CU's L1
//   holds from before another CU's atomicMin) or an atomic min.  No wave waits for another: find()
//   walks strictly decreasing indices, unite() retries only when its atomic min met a value smaller
//   than the root it believed in, and then goes on from that smaller value.  Why a stale parent
//   cannot give a wrong root: DESIGN.md, "Segments".
//
//   flatten (segments_flatten_kernel), a later launch than the last union: root[p] = the end of
//   p's parent chain, by plain loads; area[root] += 1, aggregated inside the wave first.
//
// Aggregation (wave_add).  The lanes of a wave hold up to four (key, values) entries each.  The wave
// takes the first pending key of its first pending lane, every lane sums its entries of that key,
// a shuffle tree sums over the wave, and the leader issues ONE atomic add per value: the lanes of
// a wave that share a root add once.  The loop runs once per distinct key of the wave, so a map of
// one label costs one atomic per 256 pixels, and every iteration retires at least the leader's entry.
//
// mdil_segments_count: hit_s and void_s are summed at the roots the same way (two values per key;
// pixels that add nothing do not enter), then a pass over the root pixels (area > 0) applies the
// rules and counts into 64-bit tables in LDS, flushed with one global add per non-zero entry and
// work-group as boundary_count_kernel does.  mdil_segments_filter is one gather pass.
//
// Grids are capped (kMaxRowBlocks, kMaxBlocks) and the loops stride past the cap.
#include "../../include/mdil_segments.h"
#include "head_common.h"
#include <initializer_list>

namespace {

constexpr int kWG = 256;                             // 4 wavefronts of 64 lanes
constexpr int kWaves = kWG / 64;
constexpr int kChunk = 256;                          // pixels a wavefront covers per step of the row pass
constexpr int kMaxEdges = MDIL_SEGMENTS_MAX_EDGES;
constexpr int kMaxRowBlocks = 4096;                  // row pass: 4 rows per work-group
constexpr int kMaxBlocks = 2048;                     // item passes: 256 lanes of 4 pixels per work-group
constexpr int kCounters = 6;                         // segments pixels hit_pixels covered missed unjudged

struct Edges {
  int e[kMaxEdges];
};

typedef int i32x4 __attribute__((ext_vector_type(4)));

// Four pixels of a row starting at column x0 (a multiple of 4), one per byte; 0 past W.
__device__ __forceinline__ uint32_t load4(const unsigned char* row, int x0, int W, bool packed) {
  if (packed) return x0 < W ? *reinterpret_cast<const uint32_t*>(row + x0) : 0u;
  uint32_t v = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (x0 + j < W) v |= (uint32_t)row[x0 + j] << (8 * j);
  return v;
}

__device__ __forceinline__ void store4(unsigned char* row, int x0, int W, bool packed, uint32_t v) {
  if (packed) {
    if (x0 < W) *reinterpret_cast<uint32_t*>(row + x0) = v;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (x0 + j < W) row[x0 + j] = (unsigned char)(v >> (8 * j));
}

__device__ __forceinline__ int byte_of(uint32_t v, int j) { return (int)((v >> (8 * j)) & 0xffu); }

// The same for the i32 maps; `wide`: W is a multiple of 4 and the map is 16-byte aligned.
__device__ __forceinline__ i32x4 load4i(const int* row, int x0, int W, bool wide) {
  if (wide) return x0 < W ? *reinterpret_cast<const i32x4*>(row + x0) : i32x4{0, 0, 0, 0};
  i32x4 v = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (x0 + j < W) v[j] = row[x0 + j];
  return v;
}

__device__ __forceinline__ void store4i(int* row, int x0, int W, bool wide, i32x4 v) {
  if (wide) {
    if (x0 < W) *reinterpret_cast<i32x4*>(row + x0) = v;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (x0 + j < W) row[x0 + j] = v[j];
}

// Sum over the 64 lanes of a wave, every lane active.
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// dst[v][key] += the sum of val[.][v] over every pending entry of the wave with that key, one
// atomic per key, value and wave.  Called by all 64 lanes; ends with nothing pending.
template <int NV>
__device__ __forceinline__ void wave_add(const long long (&key)[4], const int (&val)[4][NV], bool (&pend)[4],
                                         int* const (&dst)[NV]) {
  const int lane = threadIdx.x & 63;
  for (;;) {
    const long long mine = pend[0] ? key[0] : pend[1] ? key[1] : pend[2] ? key[2] : pend[3] ? key[3] : -1;
    const unsigned long long have = __ballot(mine >= 0);
    if (!have) break;
    const int leader = __ffsll((long long)have) - 1;
    const long long k = __shfl(mine, leader, 64);
    int s[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) s[v] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool take = pend[j] && key[j] == k;
#pragma unroll
      for (int v = 0; v < NV; ++v) s[v] += take ? val[j][v] : 0;
      pend[j] = pend[j] && !take;
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      s[v] = wave_sum_i32(s[v]);
      if (lane == leader && s[v]) atomicAdd(dst[v] + k, s[v]);
    }
  }
}

// Item `item` of the item passes: four pixels of one row.  -> r = n*H + y, x0, n, y.
struct Item {
  long long r, n;
  int x0, y;
};

__device__ __forceinline__ Item item_of(long long item, long long G, int H) {
  Item it;
  it.r = item / G;
  it.x0 = (int)(item - it.r * G) * 4;
  it.n = it.r / H;
  it.y = (int)(it.r - it.n * H);
  return it;
}

// ---------------------------------------------------------------------------------- label: rows
__global__ __launch_bounds__(kWG) void segments_rows_kernel(const unsigned char* __restrict__ map, long long rows,
                                                            int H, int W, bool wide, int* __restrict__ parent,
                                                            int* __restrict__ area) {
  const int lane = threadIdx.x & 63;
  const bool packed = (W & 3) == 0;
  const int nchunks = (W + kChunk - 1) / kChunk;
  // wave-uniform loop: every shuffle below runs with all 64 lanes
  for (long long row = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); row < rows;
       row += (long long)gridDim.x * kWaves) {
    const unsigned char* __restrict__ L = map + row * W;
    const int base = (int)(row % H) * W;
    int carry = -1;                                  // the last run start so far (x = 0 starts one)
    for (int c = 0; c < nchunks; ++c) {
      const int x0 = c * kChunk + lane * 4;
      const uint32_t v = load4(L, x0, W, packed);
      int before = (x0 > 0 && x0 <= W) ? (int)L[x0 - 1] : -1;
      bool brk[4];
      int m = -1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int b = byte_of(v, j);
        brk[j] = x0 + j < W && b != before;          // before = -1 at x = 0
        before = b;
        m = brk[j] ? x0 + j : m;
      }
      int inc = m;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off, 64);
        inc = lane >= off ? max(inc, t) : inc;
      }
      inc = max(inc, carry);
      const int up = __shfl_up(inc, 1, 64);
      int s = lane ? up : carry;
      carry = __shfl(inc, 63, 64);
      i32x4 out;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s = brk[j] ? x0 + j : s;
        out[j] = base + s;                           // past W: never stored
      }
      store4i(parent + row * W, x0, W, wide, out);
      store4i(area + row * W, x0, W, wide, i32x4{0, 0, 0, 0});
    }
  }
}

// --------------------------------------------------------------------------------- label: merge
__device__ __forceinline__ int parent_of(int* P, int x) {
  return __hip_atomic_load(P + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The end of x's parent chain as far as this wave sees it: indices strictly decrease.
__device__ __forceinline__ int find_shared(int* P, int x) {
  for (int t; (t = parent_of(P, x)) != x;) x = t;
  return x;
}

__device__ __forceinline__ void unite(int* P, int a, int b) {
  for (;;) {
    a = find_shared(P, a);
    b = find_shared(P, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(P + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;                            // a was a root and now hangs below b
    a = old;                                         // old < a: a had a parent already; join that one with b
  }
}

__global__ __launch_bounds__(kWG) void segments_merge_kernel(const unsigned char* __restrict__ map, long long nitems,
                                                             int H, int W, bool eight, int* parent) {
  const long long G = ((long long)W + 3) >> 2;      // items per row
  const bool packed = (W & 3) == 0;
  for (long long item = (long long)blockIdx.x * kWG + threadIdx.x; item < nitems;
       item += (long long)gridDim.x * kWG) {
    const Item it = item_of(item, G, H);
    if (it.y == 0) continue;
    const int x0 = it.x0;
    const unsigned char* __restrict__ cur = map + it.r * W;
    const unsigned char* __restrict__ abv = cur - W;
    const uint32_t c4 = load4(cur, x0, W, packed), u4 = load4(abv, x0, W, packed);
    // columns x0 - 1 .. x0 + 4 of both rows; outside the row: -1 below, -2 above (they match nothing)
    int c[6], u[6];
    c[0] = x0 > 0 ? (int)cur[x0 - 1] : -1;
    u[0] = x0 > 0 ? (int)abv[x0 - 1] : -2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c[j + 1] = x0 + j < W ? byte_of(c4, j) : -1;
      u[j + 1] = x0 + j < W ? byte_of(u4, j) : -2;
    }
    c[5] = x0 + 4 < W ? (int)cur[x0 + 4] : -1;
    u[5] = x0 + 4 < W ? (int)abv[x0 + 4] : -2;
    int* P = parent + it.n * H * W;
#pragma unroll
    for (int j = 1; j <= 4; ++j) {
      const int lab = c[j];
      if (lab < 0) continue;
      const int p = it.y * W + x0 + j - 1;
      if (u[j] == lab) {
        if (!(c[j - 1] == lab && u[j - 1] == lab)) unite(P, p, p - W);
      } else if (eight) {
        if (u[j - 1] == lab && c[j - 1] != lab) unite(P, p, p - W - 1);
        if (u[j + 1] == lab && c[j + 1] != lab) unite(P, p, p - W + 1);
      }
    }
  }
}

// ------------------------------------------------------------------------------- label: flatten
__global__ __launch_bounds__(kWG) void segments_flatten_kernel(const int* __restrict__ parent, long long nitems,
                                                               int H, int W, bool wide, int* __restrict__ root,
                                                               int* area) {
  const long long G = ((long long)W + 3) >> 2;
  const int lane = threadIdx.x & 63;
  // wave-uniform loop: wave_add runs with all 64 lanes
  for (long long first = (long long)blockIdx.x * kWG + (threadIdx.x & ~63); first < nitems;
       first += (long long)gridDim.x * kWG) {
    const long long item = first + lane;
    long long key[4] = {0, 0, 0, 0};
    int val[4][1] = {{1}, {1}, {1}, {1}};
    bool pend[4] = {false, false, false, false};
    if (item < nitems) {
      const Item it = item_of(item, G, H);
      const long long img = it.n * H * W;
      const int* __restrict__ P = parent + img;
      i32x4 out = {0, 0, 0, 0};
      int prev_parent = -1, prev_root = -1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (it.x0 + j >= W) continue;
        int q = P[it.y * W + it.x0 + j];
        if (q == prev_parent) {
          q = prev_root;
        } else {
          prev_parent = q;
          for (int t; (t = P[q]) != q;) q = t;       // strictly decreasing
          prev_root = q;
        }
        out[j] = q;
        key[j] = img + q;
        pend[j] = true;
      }
      store4i(root + it.r * W, it.x0, W, wide, out);
    }
    int* const dst[1] = {area};
    wave_add<1>(key, val, pend, dst);
  }
}

// ------------------------------------------------------------------------------------- count
__global__ __launch_bounds__(kWG) void segments_overlap_kernel(const unsigned char* __restrict__ map,
                                                               const unsigned char* __restrict__ other,
                                                               const int* __restrict__ root, long long nitems, int H,
                                                               int W, bool wide, int other_ignore, int* hit,
                                                               int* void_) {
  const long long G = ((long long)W + 3) >> 2;
  const int lane = threadIdx.x & 63;
  const bool packed = (W & 3) == 0;
  for (long long first = (long long)blockIdx.x * kWG + (threadIdx.x & ~63); first < nitems;
       first += (long long)gridDim.x * kWG) {
    const long long item = first + lane;
    long long key[4] = {0, 0, 0, 0};
    int val[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    bool pend[4] = {false, false, false, false};
    if (item < nitems) {
      const Item it = item_of(item, G, H);
      const long long img = it.n * H * W, o = it.r * W;
      const uint32_t m4 = load4(map + o, it.x0, W, packed), o4 = load4(other + o, it.x0, W, packed);
      const i32x4 r4 = load4i(root + o, it.x0, W, wide);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int q = byte_of(o4, j);
        val[j][0] = q == byte_of(m4, j) ? 1 : 0;
        val[j][1] = q == other_ignore ? 1 : 0;
        key[j] = img + r4[j];
        pend[j] = it.x0 + j < W && (val[j][0] || val[j][1]);
      }
    }
    int* const dst[2] = {hit, void_};
    wave_add<2>(key, val, pend, dst);
  }
}

struct CountArgs {
  const unsigned char* map;
  const int* area;
  const int* hit;
  const int* void_;
  unsigned long long* counters[kCounters];           // segments pixels hit_pixels covered missed unjudged
  unsigned long long* bad_labels;
  long long nitems;                                  // N * H * ceil(W / 4)
  int H, W, nc, nb, map_ignore, cover_num, cover_den;
  bool wide;
  Edges edges;
};

__global__ __launch_bounds__(kWG) void segments_count_kernel(const CountArgs p) {
  // [6][nc * nb] then bad_labels
  __shared__ unsigned long long counts[kCounters * MDIL_SEGMENTS_MAX_CLASSES * (kMaxEdges + 1) + 1];
  const int nc = p.nc, nb = p.nb, H = p.H, W = p.W;
  const int n_hist = nc * nb, n_all = kCounters * n_hist + 1;
  for (int i = threadIdx.x; i < n_all; i += kWG) counts[i] = 0ull;
  __syncthreads();

  const long long G = ((long long)W + 3) >> 2;
  for (long long item = (long long)blockIdx.x * kWG + threadIdx.x; item < p.nitems;
       item += (long long)gridDim.x * kWG) {
    const Item it = item_of(item, G, H);
    const long long o = it.r * W;
    const i32x4 a4 = load4i(p.area + o, it.x0, W, p.wide);
    if (!(a4[0] | a4[1] | a4[2] | a4[3])) continue;  // no root among the four
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int a = a4[j];
      if (a <= 0) continue;                          // past W: 0
      const long long at = o + it.x0 + j;
      const int c = (int)p.map[at];
      if (c == p.map_ignore) continue;
      if (c >= nc) {
        atomicAdd(&counts[n_all - 1], (unsigned long long)a);
        continue;
      }
      int k = 0;
#pragma unroll
      for (int i = 0; i < kMaxEdges; ++i) k += (i < nb - 1 && p.edges.e[i] < a) ? 1 : 0;
      const int h = p.hit[at], v = p.void_[at], judged = a - v, cell = c * nb + k;
      if (judged == 0) {
        atomicAdd(&counts[5 * n_hist + cell], 1ull);
        continue;
      }
      atomicAdd(&counts[cell], 1ull);
      atomicAdd(&counts[n_hist + cell], (unsigned long long)judged);
      if (h) atomicAdd(&counts[2 * n_hist + cell], (unsigned long long)h);
      if ((long long)h * p.cover_den >= (long long)p.cover_num * judged) atomicAdd(&counts[3 * n_hist + cell], 1ull);
      if (h == 0) atomicAdd(&counts[4 * n_hist + cell], 1ull);
    }
  }

  __syncthreads();
  for (int i = threadIdx.x; i < n_all; i += kWG) {
    const unsigned long long v = counts[i];
    if (!v) continue;
    atomicAdd(i == n_all - 1 ? p.bad_labels : p.counters[i / n_hist] + i % n_hist, v);
  }
}

// ------------------------------------------------------------------------------------ filter
// A work-group meets at most 2^40 / kMaxBlocks pixels, so the 32-bit tables in LDS do not wrap.
__global__ __launch_bounds__(kWG) void segments_filter_kernel(const unsigned char* __restrict__ map,
                                                              const int* __restrict__ root,
                                                              const int* __restrict__ area,
                                                              const int* __restrict__ min_area, long long nitems,
                                                              int H, int W, bool wide, int keep_id, int fill,
                                                              unsigned char* __restrict__ out,
                                                              unsigned long long* removed_segments,
                                                              unsigned long long* removed_pixels) {
  __shared__ int least[256];
  __shared__ uint32_t gone[2][256];                  // segments, pixels
  for (int i = threadIdx.x; i < 256; i += kWG) {
    least[i] = min_area[i];
    gone[0][i] = gone[1][i] = 0u;
  }
  __syncthreads();

  const long long G = ((long long)W + 3) >> 2;
  const bool packed = (W & 3) == 0;
  for (long long item = (long long)blockIdx.x * kWG + threadIdx.x; item < nitems;
       item += (long long)gridDim.x * kWG) {
    const Item it = item_of(item, G, H);
    const long long img = it.n * H * W, o = it.r * W;
    const uint32_t m4 = load4(map + o, it.x0, W, packed);
    const i32x4 r4 = load4i(root + o, it.x0, W, wide);
    uint32_t res = 0;
    int prev_root = -1, prev_area = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (it.x0 + j >= W) continue;
      const int c = byte_of(m4, j);
      if (r4[j] != prev_root) {
        prev_root = r4[j];
        prev_area = area[img + prev_root];
      }
      const bool drop = c != keep_id && prev_area < least[c];
      res |= (uint32_t)(drop ? fill : c) << (8 * j);
      if (drop) {
        atomicAdd(&gone[1][c], 1u);
        if (r4[j] == it.y * W + it.x0 + j) atomicAdd(&gone[0][c], 1u);
      }
    }
    store4(out + o, it.x0, W, packed, res);
  }

  __syncthreads();
  for (int i = threadIdx.x; i < 256; i += kWG) {
    if (gone[0][i]) atomicAdd(removed_segments + i, (unsigned long long)gone[0][i]);
    if (gone[1][i]) atomicAdd(removed_pixels + i, (unsigned long long)gone[1][i]);
  }
}

// -------------------------------------------------------------------------------------- host
bool size_ok(int N, int H, int W) {
  return N > 0 && H > 0 && W > 0 && H <= MDIL_SEGMENTS_MAX_SIZE && W <= MDIL_SEGMENTS_MAX_SIZE &&
         (long long)N * H <= MDIL_SEGMENTS_MAX_PIXELS / W;
}

long long workspace_need(int N, int H, int W) { return (8LL * N * H * W + 15) & ~15LL; }

bool sizes_ok(const char* fn, int N, int H, int W) {
  if (H > MDIL_SEGMENTS_MAX_SIZE || W > MDIL_SEGMENTS_MAX_SIZE) {
    set_error("%s: size %d x %d above %d", fn, H, W, MDIL_SEGMENTS_MAX_SIZE);
    return false;
  }
  if (!size_ok(N, H, W)) {
    set_error("%s: too large (N %d, maps %d x %d: at most 2^40 pixels)", fn, N, H, W);
    return false;
  }
  return true;
}

bool id_ok(const char* fn, const char* name, int id, int lo) {
  if (id >= lo && id <= 255) return true;
  set_error("%s: %s=%d outside [%d, 255]", fn, name, id, lo);
  return false;
}

bool space_ok(const char* fn, const void* workspace, long long workspace_bytes, long long need) {
  if (workspace && workspace_bytes >= need) return true;
  set_error("%s: needs a workspace of %lld bytes (got %p, %lld bytes)", fn, need, workspace, workspace_bytes);
  return false;
}

inline bool misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

inline bool is_wide(int W, std::initializer_list<const void*> maps) {
  bool wide = (W & 3) == 0;
  for (const void* m : maps) wide = wide && !misaligned(m, 15);
  return wide;
}

}  // namespace

API int mdil_segments_version(void) { return 100; }
API const char* mdil_segments_last_error(void) { return g_err; }

API long long mdil_segments_workspace_bytes(int N, int H, int W) {
  return size_ok(N, H, W) ? workspace_need(N, H, W) : -1;
}

API int mdil_segments_label(const unsigned char* map, int N, int H, int W, int connectivity, int* root, int* area,
                            unsigned char* workspace, long long workspace_bytes, void* stream) {
  constexpr char fn[] = "segments_label";
  if (!map || !root || !area || N <= 0 || H <= 0 || W <= 0) {
    set_error("segments_label: bad argument (map %p root %p area %p N %d H %d W %d)", (const void*)map, (void*)root,
              (void*)area, N, H, W);
    return MDIL_SEGMENTS_ERR_INVALID;
  }
  if (!sizes_ok(fn, N, H, W)) return MDIL_SEGMENTS_ERR_INVALID;
  if (connectivity != 4 && connectivity != 8) {
    set_error("segments_label: connectivity=%d is neither 4 nor 8", connectivity);
    return MDIL_SEGMENTS_ERR_INVALID;
  }
  if (misaligned(map, 3) || misaligned(root, 3) || misaligned(area, 3) || misaligned(workspace, 3)) {
    set_error("segments_label: alignment (map, root, area and workspace 4 B)");
    return MDIL_SEGMENTS_ERR_INVALID;
  }
  if (!space_ok(fn, workspace, workspace_bytes, workspace_need(N, H, W))) return MDIL_SEGMENTS_ERR_INVALID;

  const long long rows = (long long)N * H, nitems = rows * (((long long)W + 3) >> 2);
  int* parent = reinterpret_cast<int*>(workspace);
  const bool wide = is_wide(W, {root, area, workspace});
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(segments_rows_kernel, dim3(bounded_grid(rows, kWaves, kMaxRowBlocks)), dim3(kWG), 0, s, map,
                     rows, H, W, wide, parent, area);
  if (!launched(fn)) return MDIL_SEGMENTS_ERR_LAUNCH;
  const dim3 grid(bounded_grid(nitems, kWG, kMaxBlocks));
  if (H > 1) {
    hipLaunchKernelGGL(segments_merge_kernel, grid, dim3(kWG), 0, s, map, nitems, H, W, connectivity == 8, parent);
    if (!launched(fn)) return MDIL_SEGMENTS_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(segments_flatten_kernel, grid, dim3(kWG), 0, s, parent, nitems, H, W, wide, root, area);
  return launched(fn) ? MDIL_SEGMENTS_OK : MDIL_SEGMENTS_ERR_LAUNCH;
}

API int mdil_segments_count(const unsigned char* map, const unsigned char* other, const int* root, const int* area,
                            int N, int H, int W, int nc, int map_ignore, int other_ignore, const int* edges,
                            int n_edges, int cover_num, int cover_den, unsigned char* workspace,
                            long long workspace_bytes, int* hit, int* void_, long long* segments, long long* pixels,
                            long long* hit_pixels, long long* covered, long long* missed, long long* unjudged,
                            long long* bad_labels, void* stream) {
  constexpr char fn[] = "segments_count";
  long long* const counters[kCounters] = {segments, pixels, hit_pixels, covered, missed, unjudged};
  if (!map || !other || !root || !area || !edges || !segments || !pixels || !hit_pixels || !covered || !missed ||
      !unjudged || !bad_labels || N <= 0 || H <= 0 || W <= 0) {
    set_error("segments_count: bad argument (map %p other %p root %p area %p edges %p segments %p pixels %p "
              "hit_pixels %p covered %p missed %p unjudged %p bad_labels %p N %d H %d W %d)",
              (const void*)map, (const void*)other, (const void*)root, (const void*)area, (const void*)edges,
              (void*)segments, (void*)pixels, (void*)hit_pixels, (void*)covered, (void*)missed, (void*)unjudged,
              (void*)bad_labels, N, H, W);
    return MDIL_SEGMENTS_ERR_INVALID;
  }
  if (!classes_ok(fn, nc, MDIL_SEGMENTS_MIN_CLASSES, MDIL_SEGMENTS_MAX_CLASSES)) return MDIL_SEGMENTS_ERR_INVALID;
  if (!sizes_ok(fn, N, H, W)) return MDIL_SEGMENTS_ERR_INVALID;
  if (!id_ok(fn, "map_ignore", map_ignore, -1) || !id_ok(fn, "other_ignore", other_ignore, -1))
    return MDIL_SEGMENTS_ERR_INVALID;
  if (n_edges < 1 || n_edges > kMaxEdges) {
    set_error("segments_count: n_edges=%d outside [1, %d]", n_edges, kMaxEdges);
    return MDIL_SEGMENTS_ERR_INVALID;
  }
  Edges ed = {};
  for (int i = 0; i < n_edges; ++i) {
    ed.e[i] = edges[i];
    if (edges[i] < 1 || edges[i] > MDIL_SEGMENTS_MAX_EDGE || (i && edges[i] <= edges[i - 1])) {
      set_error("segments_count: edges must be strictly increasing within [1, %d] (edges[%d]=%d)",
                MDIL_SEGMENTS_MAX_EDGE, i, edges[i]);
      return MDIL_SEGMENTS_ERR_INVALID;
    }
  }
  if (cover_num < 1 || cover_num > cover_den || cover_den > MDIL_SEGMENTS_MAX_COVER_DEN) {
    set_error("segments_count: coverage %d/%d outside 0 < cover_num <= cover_den <= %d", cover_num, cover_den,
              MDIL_SEGMENTS_MAX_COVER_DEN);
    return MDIL_SEGMENTS_ERR_INVALID;
  }
  bool odd = misaligned(map, 3) || misaligned(other, 3) || misaligned(root, 3) || misaligned(area, 3) ||
             misaligned(workspace, 3) || misaligned(hit, 3) || misaligned(void_, 3) || misaligned(bad_labels, 7);
  for (int i = 0; i < kCounters; ++i) odd = odd || misaligned(counters[i], 7);
  if (odd) {
    set_error("segments_count: alignment (map, other, root, area, workspace, hit and void 4 B; the counters 8 B)");
    return MDIL_SEGMENTS_ERR_INVALID;
  }
  if (!space_ok(fn, workspace, workspace_bytes, workspace_need(N, H, W))) return MDIL_SEGMENTS_ERR_INVALID;

  const long long plane = (long long)N * H * W, nitems = (long long)N * H * (((long long)W + 3) >> 2);
  int* const hit_at = hit ? hit : reinterpret_cast<int*>(workspace);
  int* const void_at = void_ ? void_ : reinterpret_cast<int*>(workspace) + plane;
  hipStream_t s = (hipStream_t)stream;
  for (int* sums : {hit_at, void_at}) {
    const hipError_t e = hipMemsetAsync(sums, 0, (size_t)plane * sizeof(int), s);
    if (e != hipSuccess) {
      set_error("segments_count: clearing the sums failed: %s", hipGetErrorString(e));
      return MDIL_SEGMENTS_ERR_LAUNCH;
    }
  }
  const bool wide = is_wide(W, {root, area, hit_at, void_at});
  const dim3 grid(bounded_grid(nitems, kWG, kMaxBlocks));
  hipLaunchKernelGGL(segments_overlap_kernel, grid, dim3(kWG), 0, s, map, other, root, nitems, H, W, wide,
                     other_ignore, hit_at, void_at);
  if (!launched(fn)) return MDIL_SEGMENTS_ERR_LAUNCH;

  CountArgs p;
  p.map = map, p.area = area, p.hit = hit_at, p.void_ = void_at;
  for (int i = 0; i < kCounters; ++i) p.counters[i] = reinterpret_cast<unsigned long long*>(counters[i]);
  p.bad_labels = reinterpret_cast<unsigned long long*>(bad_labels);
  p.nitems = nitems;
  p.H = H, p.W = W, p.nc = nc, p.nb = n_edges + 1, p.map_ignore = map_ignore;
  p.cover_num = cover_num, p.cover_den = cover_den, p.wide = wide, p.edges = ed;
  hipLaunchKernelGGL(segments_count_kernel, grid, dim3(kWG), 0, s, p);
  return launched(fn) ? MDIL_SEGMENTS_OK : MDIL_SEGMENTS_ERR_LAUNCH;
}

API int mdil_segments_filter(const unsigned char* map, const int* root, const int* area, int N, int H, int W,
                             const int* min_area, int keep_id, int fill, unsigned char* out,
                             long long* removed_segments, long long* removed_pixels, void* stream) {
  constexpr char fn[] = "segments_filter";
  if (!map || !root || !area || !min_area || !out || !removed_segments || !removed_pixels || N <= 0 || H <= 0 ||
      W <= 0) {
    set_error("segments_filter: bad argument (map %p root %p area %p min_area %p out %p removed_segments %p "
              "removed_pixels %p N %d H %d W %d)",
              (const void*)map, (const void*)root, (const void*)area, (const void*)min_area, (void*)out,
              (void*)removed_segments, (void*)removed_pixels, N, H, W);
    return MDIL_SEGMENTS_ERR_INVALID;
  }
  if (!sizes_ok(fn, N, H, W)) return MDIL_SEGMENTS_ERR_INVALID;
  if (!id_ok(fn, "keep_id", keep_id, -1) || !id_ok(fn, "fill", fill, 0)) return MDIL_SEGMENTS_ERR_INVALID;
  if (out == map) {
    set_error("segments_filter: out may not alias map");
    return MDIL_SEGMENTS_ERR_INVALID;
  }
  if (misaligned(map, 3) || misaligned(root, 3) || misaligned(area, 3) || misaligned(min_area, 3) ||
      misaligned(out, 3) || misaligned(removed_segments, 7) || misaligned(removed_pixels, 7)) {
    set_error("segments_filter: alignment (map, root, area, min_area and out 4 B; the counters 8 B)");
    return MDIL_SEGMENTS_ERR_INVALID;
  }
  const long long nitems = (long long)N * H * (((long long)W + 3) >> 2);
  hipLaunchKernelGGL(segments_filter_kernel, dim3(bounded_grid(nitems, kWG, kMaxBlocks)), dim3(kWG), 0,
                     (hipStream_t)stream, map, root, area, min_area, nitems, H, W, is_wide(W, {root}), keep_id, fill,
                     out, reinterpret_cast<unsigned long long*>(removed_segments),
                     reinterpret_cast<unsigned long long*>(removed_pixels));
  return launched(fn) ? MDIL_SEGMENTS_OK : MDIL_SEGMENTS_ERR_LAUNCH;
}
