// libmdil_audit.so: which labels does the head confidently contradict (gfx950).  Two kernels:
//
//   audit_head    Decoder.output_conv + softmax quantised to 16 bits per class + the per-class counts and
//                 sums of the self-confidence (sweep 1) + with thresholds the suggested class, the confident
//                 joint and the per-image issue counts (sweep 2).  openset_head.hip's chain with other
//                 outputs; the logits are never stored.
//   audit_apply   stored maps -> the cleaned label map, the issue mask, their counters
//
// The chain is openset_head.hip's, spelled the same way (Wp[a*2+b][c][ci] in LDS, the logits of one parity in
// registers, vote for m, then c ascending: d_c, one hardware exp2, s), so m, s and conf = 1 / s are its bits.
// The class walk then runs a second time: e_c is formed again from the logit that is still in its register
// (the same operations on the same operands: the same bits), p_c = e_c * conf, q_c = min(65535, trunc(p_c *
// 65536)), q_c >= thr[c] makes the class confident, and the vote restricted to the confident classes gives the
// suggestion.  Keeping the 32 e_c beside the 32 logits instead would cost 32 more registers; see the occupancy
// note at the kernel.
//
// Layout of audit_head.  A lane owns one feature pixel (16 channels in registers) and walks its four
// parities.  The grid is bounded and the loop over feature pixels strides; its trip count is the same for
// every lane of a work-group (a lane past the end computes a clamped pixel, writes nothing and counts
// nothing), because the counting step below talks to the whole wave.
//
// The adds.  Labels are spatially coherent, so per parity the wave first merges by (image, given class): the
// lowest lane that still has something to add broadcasts its key (readlane), a ballot finds every lane with
// that key, the leader carries their number, the sum of their q (a xor-shuffle tree over the wave), the number
// of them on the diagonal and in the "none" column and the number of issues as ONE add each, and the matched
// lanes retire.  After kMergeRounds rounds whatever is left goes on lane by lane: per-pixel random targets pay
// kMergeRounds rounds and then what they would have paid anyway.  Off-diagonal cells of the joint (the issues,
// rare on real data) are always added lane by lane.  The adds go to tables in LDS -- count [32] u32, qsum [32]
// u64, joint [32][33] u32, per_image [32][2] u32: 4.9 KB -- and from there, once per work-group, to global
// memory by 64-bit atomics (relaxed, agent scope).  The per_image table holds ONE image: a trip whose 256
// feature pixels lie in one image adds there (the table is flushed when the image changes); a trip that spans
// images sends its per_image adds straight to global memory.
//
// No 32-bit LDS counter can wrap.  An add is at most one count per output pixel and table cell; a work-group
// sees at most ceil(2^38 / (kHeadMaxBlocks * 256)) trips of 256 feature pixels = 1024 output pixels each at the
// largest accepted input (2^40 output pixels), 1.44e9 < 2^31 adds in all, and the tables are flushed after its
// loop (static_assert below).  qsum grows by up to 65,535 per pixel: its LDS counters are 64-bit.  Integer
// sums: the result does not depend on the order of arrival.
//
// audit_apply.  pseudo_apply's layout (map_common.h's Run, load_bytes, store_bytes and flush_counters): a lane
// owns 8 consecutive pixels (8-byte target and suggest loads, one 16-byte selfq load, 8-byte out and mask
// stores; the last item of an odd-sized map goes byte by byte); the counters live in LDS as 32-bit integers,
// runs of equal keys inside a lane's 8 pixels are one LDS atomic, and a work-group flushes its non-zero
// counters every kFlushEvery trips and at its end by 64-bit global atomics.
#include "../../include/mdil_audit.h"
#include "map_common.h"

#include <float.h>

namespace {

constexpr int kMaxC = MDIL_AUDIT_MAX_CLASSES;
constexpr int kHeadWG = 256;                         // 4 wavefronts of 64 lanes
constexpr int kHeadMaxBlocks = 768;                  // three per CU; beyond 196,608 feature pixels the loop strides
constexpr int kMergeRounds = 4;                      // ballot rounds per parity before lane-by-lane adds; below 3 the
                                                     // compiler unrolls them: 186 VGPRs, two waves per SIMD, 1.5 x the time
constexpr int kMapWG = 256;
constexpr int kMapMaxBlocks = 512;                   // beyond 131,072 items (of 8 pixels) the loop strides
constexpr int kFlushEvery = 1 << 19;                 // trips; a trip adds at most 2048 counts per work-group
constexpr char kFnHead[] = "audit_head";
constexpr char kFnApply[] = "audit_apply";

// The quantisation rule of pseudo_head.hip: p * 65536 is exact, the cast truncates, p = 1 gives 65535.
// The comparison first keeps a NaN out of the cast (a NaN is not >= anything: it is sent to 0).
__device__ __forceinline__ uint32_t quantise(float p) {
  const float v = p * 65536.0f;
  return v >= 65535.0f ? 65535u : (v >= 0.0f ? (uint32_t)v : 0u);
}

// The work-group's tables and where they go.
struct Tables {
  uint32_t* Cl;        // [nc]
  u64* Ql;             // [nc]
  uint32_t* Jl;        // [nc][nc + 1]
  uint32_t* Pl;        // [nc][2], one image
  u64* per_image;      // global; used where the trip spans images
  bool count, qsum, joint, per_image_lds, per_image_global;
  int nc;
};

// `cnt` pixels of image n and given class t: the sum of their q, how many of them were suggested t, how many
// nothing, and how many are issues.
__device__ __forceinline__ void add_group(const Tables& T, uint32_t t, int n, uint32_t cnt, uint32_t qs, uint32_t diag,
                                          uint32_t none, uint32_t issues) {
  if (T.count) atomicAdd(&T.Cl[t], cnt);
  if (T.qsum) atomicAdd(&T.Ql[t], (u64)qs);
  if (T.joint) {
    if (diag) atomicAdd(&T.Jl[t * (uint32_t)(T.nc + 1) + t], diag);
    if (none) atomicAdd(&T.Jl[t * (uint32_t)(T.nc + 1) + (uint32_t)T.nc], none);
  }
  if (T.per_image_lds) {
    atomicAdd(&T.Pl[t * 2u], cnt);
    if (issues) atomicAdd(&T.Pl[t * 2u + 1u], issues);
  } else if (T.per_image_global) {
    u64* row = T.per_image + ((long long)n * T.nc + t) * 2;
    __hip_atomic_fetch_add(row, (u64)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (issues) __hip_atomic_fetch_add(row + 1, (u64)issues, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One parity's adds of a wave: every lane of the wave calls it (the caller's loops are wave-uniform).
// active: the lane's pixel is valid and finite; t < nc its given class, n its image, qt its self-q, sug its
// suggestion (nc: none).
__device__ __forceinline__ void wave_merged_adds(const Tables& T, bool active, uint32_t t, int n, uint32_t qt,
                                                 uint32_t sug) {
  const int lane = threadIdx.x & 63;
  const uint32_t nc = (uint32_t)T.nc;
  if (T.joint && active && sug != t && sug != nc) atomicAdd(&T.Jl[t * (nc + 1u) + sug], 1u);   // an issue's cell
  u64 todo = __ballot(active);
  for (int round = 0; round < kMergeRounds && todo; ++round) {
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
    const uint32_t t0 = (uint32_t)__builtin_amdgcn_readlane((int)t, leader);
    const int n0 = __builtin_amdgcn_readlane(n, leader);
    const bool match = active && t == t0 && n == n0;
    const u64 same = __ballot(match);
    const uint32_t qs = T.qsum ? wave_sum_u32(match ? qt : 0u) : 0u;
    const uint32_t diag = (uint32_t)__popcll(__ballot(match && sug == t0));
    const uint32_t none = (uint32_t)__popcll(__ballot(match && sug == nc));
    const uint32_t cnt = (uint32_t)__popcll(same);
    if (lane == leader) add_group(T, t0, n0, cnt, qs, diag, none, cnt - diag - none);
    active = active && !match;
    todo &= ~same;
  }
  if (active) add_group(T, t, n, 1u, qt, sug == t ? 1u : 0u, sug == nc ? 1u : 0u, sug != t && sug != nc ? 1u : 0u);
}

// Occupancy: __launch_bounds__(256, 2) as openset_head, with the 32 logits of a parity and the 16 features in
// registers.  The compiler reports 165 VGPRs and no scratch: three waves per SIMD, which is what openset_head
// runs at (124 VGPRs, held to three by its 41 KB of LDS).  Holding the 32 e_c as well would add about 32
// registers and fall to two waves per SIMD (Label audit).
__global__ __launch_bounds__(kHeadWG, 2) void audit_head_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, long long npix, int W,
    long long HW, int nc, const unsigned char* __restrict__ target, int ignore_index, const int* __restrict__ thr,
    int q_class, int none_id, unsigned short* __restrict__ qmap, unsigned char* __restrict__ suggest,
    u64* __restrict__ count, u64* __restrict__ qsum, u64* __restrict__ joint, u64* __restrict__ per_image,
    u64* __restrict__ bad_targets, u64* __restrict__ nonfinite) {
  __shared__ __attribute__((aligned(16))) float Wp[4][kMaxC][16];   // [a*2+b][c][ci]
  __shared__ float Bl[kMaxC];
  __shared__ int Tl[kMaxC];                                          // thresholds
  __shared__ uint32_t Cl[kMaxC];
  __shared__ u64 Ql[kMaxC];
  __shared__ uint32_t Jl[kMaxC * (kMaxC + 1)];
  __shared__ uint32_t Pl[kMaxC * 2];
  __shared__ uint32_t nf, bt;
  static_assert((MDIL_AUDIT_MAX_PIXELS / 4 + (long long)kHeadMaxBlocks * kHeadWG - 1) / ((long long)kHeadMaxBlocks * kHeadWG) *
                        kHeadWG * 4 < 0x80000000LL,
                "a 32-bit LDS counter could wrap");
  for (int i = threadIdx.x; i < nc * 64; i += kHeadWG) {
    const int k = i & 3, ci = (i >> 2) & 15, c = i >> 6;
    Wp[k][c][ci] = w[(ci * nc + c) * 4 + k];
  }
  for (int i = threadIdx.x; i < nc; i += kHeadWG) {
    Bl[i] = bias[i];
    Tl[i] = thr ? thr[i] : MDIL_AUDIT_Q_ONE;
    Cl[i] = 0u;
    Ql[i] = 0ull;
    Pl[2 * i] = Pl[2 * i + 1] = 0u;
  }
  for (int i = threadIdx.x; i < nc * (nc + 1); i += kHeadWG) Jl[i] = 0u;
  if (threadIdx.x == 0) nf = bt = 0u;
  __syncthreads();

  const bool counting = count || qsum || joint || per_image;        // uniform over the grid
  const bool deciding = thr && (suggest || joint || per_image);
  Tables T;
  T.Cl = Cl;
  T.Ql = Ql;
  T.Jl = Jl;
  T.Pl = Pl;
  T.per_image = per_image;
  T.count = count != nullptr;
  T.qsum = qsum != nullptr;
  T.joint = joint != nullptr;
  T.nc = nc;
  uint32_t bad = 0u, badt = 0u;
  long long held = -1;                                               // the image whose counts Pl holds
  // the trip count is the same for every lane of the work-group
  for (long long base = (long long)blockIdx.x * kHeadWG; base < npix; base += (long long)gridDim.x * kHeadWG) {
    const bool valid = base + threadIdx.x < npix;
    const long long p = valid ? base + threadIdx.x : npix - 1;     // a lane past the end: a clamped pixel, no writes
    const long long last = base + kHeadWG - 1 < npix ? base + kHeadWG - 1 : npix - 1;
    const long long n_lo = base / HW, n_hi = last / HW;            // uniform over the work-group
    const bool one_image = per_image && n_lo == n_hi;
    if (one_image && held >= 0 && held != n_lo) {
      __syncthreads();                                             // the adds of the trip before are in
      flush_counters<kHeadWG>(Pl, nc * 2, per_image + held * nc * 2);
      __syncthreads();
    }
    if (one_image) held = n_lo;
    T.per_image_lds = one_image;
    T.per_image_global = per_image && !one_image;

    f32x4 xv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xv[k] = *reinterpret_cast<const f32x4*>(x + p * 16 + k * 4);
    const long long r = p / W;                                     // n * H + h
    const int n = (int)(p / HW);
    const long long o0 = (2 * r * 2 * W) + 2 * (p - r * W);        // pixel (2h, 2w); row below: + 2W
    uint32_t given = 0u;                                           // byte a*2+b
    if (target) given = quad_bytes(target, o0, W);
    uint32_t sugs = 0u, q_top = 0u, q_bottom = 0u;                 // byte a*2+b; the two pixels of a row

#pragma unroll 1
    for (int par = 0; par < 4; ++par) {
      float d[kMaxC];
      // The logits of this parity: bias first, then ci ascending.  map_common.h's stage_parity and parity_logits,
      // spelled out here and above: through the helpers the compiler schedules this kernel differently (same
      // registers, same occupancy) and sweep 2 ran 0.5 to 0.9 % slower than before, past the run-to-run margin
      // (profiles/map_common_ab.json); spelled out, the kernel's code is what it was.
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) {
        if (c < nc) {
          float a = Bl[c];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(&Wp[par][c][k * 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e) a = __builtin_fmaf(xv[k][e], wv[e], a);
          }
          d[c] = a;
        }
      }
      float m = 0.f;
      int bi = 0;
#pragma unroll
      for (int c = 0; c < kMaxC; ++c)
        if (c < nc) vote(c, d[c], m, bi);
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) {
        if (c < nc) {
          float v = d[c] - m;
          v = v == -INFINITY ? -FLT_MAX : v;
          s += __builtin_amdgcn_exp2f(__fmul_rn(v, kLog2e));
        }
      }
      const float conf = 1.0f / s;
      const bool finite = is_finite(s) && is_finite(m);

      const uint32_t tb = (given >> (8 * par)) & 0xffu;
      const bool labelled = target && (int)tb != ignore_index;
      const bool usable = labelled && tb < (uint32_t)nc;           // a VALID pixel
      badt += valid && labelled && !usable ? 1u : 0u;
      bad += valid && !finite ? 1u : 0u;
      const int qc = q_class < nc ? q_class : (usable ? (int)tb : -1);

      // the second walk: e_c again (the same operations on the same operands), q_c, confident, vote
      uint32_t q_sel = 0u, q_given = 0u;
      float best = 0.f;
      int sug = -1;
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) {
        if (c < nc) {
          float v = d[c] - m;
          v = v == -INFINITY ? -FLT_MAX : v;
          const float e = __builtin_amdgcn_exp2f(__fmul_rn(v, kLog2e));
          const uint32_t q = quantise(__fmul_rn(e, conf));
          q_sel = c == qc ? q : q_sel;
          q_given = (uint32_t)c == tb ? q : q_given;
          if (deciding) {
            const bool in = (int)q >= Tl[c];
            const bool take = in && (sug < 0 || d[c] > best || (d[c] != d[c] && best == best));
            best = take ? d[c] : best;
            sug = take ? c : sug;
          }
        }
      }
      if (!finite) {
        q_sel = 0u;
        sug = -1;
      }
      sugs |= (sug < 0 ? (uint32_t)none_id : (uint32_t)sug) << (8 * par);
      if (par < 2)
        q_top |= q_sel << (16 * (par & 1));
      else
        q_bottom |= q_sel << (16 * (par & 1));
      if (counting)
        wave_merged_adds(T, valid && finite && usable, usable ? tb : 0u, n, q_given,
                         sug < 0 ? (uint32_t)nc : (uint32_t)sug);
    }

    if (valid && suggest) {
      *reinterpret_cast<uint16_t*>(suggest + o0) = (uint16_t)(sugs & 0xffffu);
      *reinterpret_cast<uint16_t*>(suggest + o0 + 2LL * W) = (uint16_t)(sugs >> 16);
    }
    if (valid && qmap) {
      *reinterpret_cast<uint32_t*>(qmap + o0) = q_top;
      *reinterpret_cast<uint32_t*>(qmap + o0 + 2LL * W) = q_bottom;
    }
  }

  if (bad) atomicAdd(&nf, bad);
  if (badt) atomicAdd(&bt, badt);
  __syncthreads();                                                 // every lane of the work-group is here
  if (threadIdx.x == 0) {
    if (nonfinite && nf) __hip_atomic_fetch_add(nonfinite, (u64)nf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (bad_targets && bt) __hip_atomic_fetch_add(bad_targets, (u64)bt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (count) flush_counters<kHeadWG>(Cl, nc, count);
  if (joint) flush_counters<kHeadWG>(Jl, nc * (nc + 1), joint);
  if (per_image && held >= 0) flush_counters<kHeadWG>(Pl, nc * 2, per_image + held * nc * 2);
  if (qsum) {
    for (int i = threadIdx.x; i < nc; i += kHeadWG)
      if (Ql[i]) __hip_atomic_fetch_add(qsum + i, Ql[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(kMapWG) void audit_apply_kernel(
    const unsigned char* __restrict__ target, const unsigned char* __restrict__ suggest,
    const unsigned short* __restrict__ selfq, long long npix, long long nitems, int nc, int ignore_index, int none_id,
    int mode, const int* __restrict__ max_q, int drop_id, unsigned char* __restrict__ out,
    unsigned char* __restrict__ mask, u64* __restrict__ seen, u64* __restrict__ acted, u64* __restrict__ bad_targets) {
  __shared__ uint32_t Al[kMaxC * kMaxC];                             // [given][suggested], acted on
  __shared__ uint32_t Sl[kMaxC];                                     // seen
  __shared__ int Ml[kMaxC];                                          // max_q
  __shared__ uint32_t bad_t;
  for (int i = threadIdx.x; i < nc * nc; i += kMapWG) Al[i] = 0u;
  for (int c = threadIdx.x; c < nc; c += kMapWG) {
    Sl[c] = 0u;
    Ml[c] = max_q[c];
  }
  if (threadIdx.x == 0) bad_t = 0u;
  __syncthreads();

  int trips = 0;
  for (long long base = (long long)blockIdx.x * kMapWG; base < nitems; base += (long long)gridDim.x * kMapWG) {
    const long long item = base + threadIdx.x;
    if (item < nitems) {
      const long long o = item * kPerItem;
      const int n = o + kPerItem <= npix ? kPerItem : (int)(npix - o);
      uint32_t tg[kPerItem], sg[kPerItem], sq[kPerItem];
      load_bytes(target, o, n, tg);
      load_bytes(suggest, o, n, sg);
      if (n == kPerItem) {
        const uint4 cv = *reinterpret_cast<const uint4*>(selfq + o);
        const uint32_t cw[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
        for (int j = 0; j < kPerItem; ++j) sq[j] = (cw[j >> 1] >> (16 * (j & 1))) & 0xffffu;
      } else {
#pragma unroll
        for (int j = 0; j < kPerItem; ++j) sq[j] = j < n ? (uint32_t)selfq[o + j] : 0u;
      }

      uint32_t ob[kPerItem], mb[kPerItem], nbad = 0u;
      Run seen_run(Sl), acted_run(Al);
#pragma unroll
      for (int j = 0; j < kPerItem; ++j) {
        ob[j] = tg[j];
        mb[j] = 0u;
        if (j < n && (int)tg[j] != ignore_index) {
          if (tg[j] >= (uint32_t)nc) {
            ++nbad;
          } else {
            seen_run.add((int)tg[j]);
            const bool issue = (int)sg[j] != none_id && sg[j] < (uint32_t)nc && sg[j] != tg[j];
            if (issue) {
              const bool act = (int)sq[j] <= Ml[tg[j]];
              mb[j] = act ? 255u : 128u;
              if (act) {
                ob[j] = mode == MDIL_AUDIT_RELABEL ? sg[j] : (uint32_t)drop_id;
                acted_run.add((int)(tg[j] * (uint32_t)nc + sg[j]));
              }
            }
          }
        }
      }
      seen_run.done();
      acted_run.done();
      if (nbad) atomicAdd(&bad_t, nbad);
      if (out) store_bytes(out, o, n, ob);
      if (mask) store_bytes(mask, o, n, mb);
    }

    const bool last = base + (long long)gridDim.x * kMapWG >= nitems;
    if (last || ++trips == kFlushEvery) {                          // uniform over the work-group
      trips = 0;
      __syncthreads();
      flush_counters<kMapWG>(Sl, nc, seen);
      flush_counters<kMapWG>(Al, nc * nc, acted);
      if (threadIdx.x == 0) {
        if (bad_t && bad_targets) __hip_atomic_fetch_add(bad_targets, (u64)bad_t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bad_t = 0u;
      }
      __syncthreads();
    }
  }
}

}  // namespace

API int mdil_audit_version(void) { return 100; }
API const char* mdil_audit_last_error(void) { return g_err; }

API int mdil_audit_head(const float* x, const float* w, const float* bias, int N, int H, int W, int nc,
                        const unsigned char* target, int ignore_index, const int* thr, int q_class, int none_id,
                        unsigned short* qmap, unsigned char* suggest, long long* count, long long* qsum,
                        long long* joint, long long* per_image, long long* bad_targets, long long* nonfinite,
                        void* stream) {
  if (!x || !w || !bias || N <= 0 || H <= 0 || W <= 0) {
    set_error("audit_head: bad argument (x %p w %p bias %p N %d H %d W %d)", (const void*)x, (const void*)w,
              (const void*)bias, N, H, W);
    return MDIL_AUDIT_ERR_INVALID;
  }
  if (!qmap && !suggest && !count && !qsum && !joint && !per_image && !bad_targets && !nonfinite) {
    set_error("audit_head: nothing to write (qmap, suggest and every counter are NULL)");
    return MDIL_AUDIT_ERR_INVALID;
  }
  if (!classes_ok(kFnHead, nc, MDIL_AUDIT_MIN_CLASSES, MDIL_AUDIT_MAX_CLASSES)) return MDIL_AUDIT_ERR_INVALID;
  if (!ignore_ok(kFnHead, ignore_index)) return MDIL_AUDIT_ERR_INVALID;
  if (none_id < 0 || none_id > 255) {
    set_error("audit_head: none_id=%d outside [0, 255]", none_id);
    return MDIL_AUDIT_ERR_INVALID;
  }
  if (!target && (count || qsum || joint || per_image || bad_targets)) {
    set_error("audit_head: count, qsum, joint, per_image and bad_targets need a target");
    return MDIL_AUDIT_ERR_INVALID;
  }
  if (!thr && (suggest || joint || per_image)) {
    set_error("audit_head: suggest, joint and per_image need thr (i32 [nc] on the device)");
    return MDIL_AUDIT_ERR_INVALID;
  }
  if (qmap && (q_class < 0 || q_class > nc || (q_class == nc && !target))) {
    set_error("audit_head: q_class=%d with nc=%d and target %p (a qmap needs a q_class in [0, nc]; nc, the given "
              "class, needs a target)", q_class, nc, (const void*)target);
    return MDIL_AUDIT_ERR_INVALID;
  }
  if (((uintptr_t)x & 15) || ((uintptr_t)w & 3) || ((uintptr_t)bias & 3) || ((uintptr_t)target & 1) ||
      ((uintptr_t)thr & 3) || ((uintptr_t)suggest & 1) || ((uintptr_t)qmap & 3) || ((uintptr_t)count & 7) ||
      ((uintptr_t)qsum & 7) || ((uintptr_t)joint & 7) || ((uintptr_t)per_image & 7) || ((uintptr_t)bad_targets & 7) ||
      ((uintptr_t)nonfinite & 7)) {
    set_error("audit_head: alignment (x 16 B; w, bias and thr 4 B; target and suggest 2 B; qmap 4 B; the counters 8 B)");
    return MDIL_AUDIT_ERR_INVALID;
  }
  if (!shape_ok(N, H, W, MDIL_AUDIT_MAX_PIXELS / 4)) {
    set_error("audit_head: too large (N %d, features %d x %d: at most 2^40 output pixels)", N, H, W);
    return MDIL_AUDIT_ERR_INVALID;
  }
  const long long npix = (long long)N * H * W;
  const int grid = bounded_grid(npix, kHeadWG, kHeadMaxBlocks);
  // q_class means something only with a qmap: without one the kernel selects no class
  hipLaunchKernelGGL(audit_head_kernel, dim3(grid), dim3(kHeadWG), 0, (hipStream_t)stream, x, w, bias, npix, W,
                     (long long)H * W, nc, target, ignore_index, thr, qmap ? q_class : 0, none_id, qmap, suggest,
                     reinterpret_cast<u64*>(count), reinterpret_cast<u64*>(qsum), reinterpret_cast<u64*>(joint),
                     reinterpret_cast<u64*>(per_image), reinterpret_cast<u64*>(bad_targets),
                     reinterpret_cast<u64*>(nonfinite));
  return launched(kFnHead) ? MDIL_AUDIT_OK : MDIL_AUDIT_ERR_LAUNCH;
}

API int mdil_audit_apply(const unsigned char* target, const unsigned char* suggest, const unsigned short* selfq,
                         long long npix, int nc, int ignore_index, int none_id, int mode, const int* max_q,
                         int drop_id, unsigned char* out, unsigned char* mask, long long* seen, long long* acted,
                         long long* bad_targets, void* stream) {
  if (!target || !suggest || !selfq || !max_q || npix <= 0) {
    set_error("audit_apply: bad argument (target %p suggest %p selfq %p max_q %p npix %lld)", (const void*)target,
              (const void*)suggest, (const void*)selfq, (const void*)max_q, npix);
    return MDIL_AUDIT_ERR_INVALID;
  }
  if (npix > MDIL_AUDIT_MAX_PIXELS) {
    set_error("audit_apply: too large (npix %lld: at most 2^40 pixels)", npix);
    return MDIL_AUDIT_ERR_INVALID;
  }
  if (!classes_ok(kFnApply, nc, MDIL_AUDIT_MIN_CLASSES, MDIL_AUDIT_MAX_CLASSES)) return MDIL_AUDIT_ERR_INVALID;
  if (!ignore_ok(kFnApply, ignore_index)) return MDIL_AUDIT_ERR_INVALID;
  if (none_id < 0 || none_id > 255 || drop_id < 0 || drop_id > 255) {
    set_error("audit_apply: none_id=%d or drop_id=%d outside [0, 255]", none_id, drop_id);
    return MDIL_AUDIT_ERR_INVALID;
  }
  if (mode != MDIL_AUDIT_PRUNE && mode != MDIL_AUDIT_RELABEL) {
    set_error("audit_apply: mode=%d (0 prune, 1 relabel)", mode);
    return MDIL_AUDIT_ERR_INVALID;
  }
  if (!out && !mask && !seen && !acted && !bad_targets) {
    set_error("audit_apply: nothing to write (out, mask and every counter are NULL)");
    return MDIL_AUDIT_ERR_INVALID;
  }
  if (((uintptr_t)target & 7) || ((uintptr_t)suggest & 7) || ((uintptr_t)selfq & 15) || ((uintptr_t)max_q & 3) ||
      ((uintptr_t)out & 7) || ((uintptr_t)mask & 7) || ((uintptr_t)seen & 7) || ((uintptr_t)acted & 7) ||
      ((uintptr_t)bad_targets & 7)) {
    set_error("audit_apply: alignment (selfq 16 B; target, suggest, out, mask and the counters 8 B; max_q 4 B)");
    return MDIL_AUDIT_ERR_INVALID;
  }
  const long long nitems = (npix + kPerItem - 1) / kPerItem;
  const int grid = bounded_grid(nitems, kMapWG, kMapMaxBlocks);
  hipLaunchKernelGGL(audit_apply_kernel, dim3(grid), dim3(kMapWG), 0, (hipStream_t)stream, target, suggest, selfq, npix,
                     nitems, nc, ignore_index, none_id, mode, max_q, drop_id, out, mask, reinterpret_cast<u64*>(seen),
                     reinterpret_cast<u64*>(acted), reinterpret_cast<u64*>(bad_targets));
  return launched(kFnApply) ? MDIL_AUDIT_OK : MDIL_AUDIT_ERR_LAUNCH;
}
