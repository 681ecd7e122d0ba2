// libmdil_density.so: open-set scores in feature space (gfx950).  Two kernels:
//
//   density_head   Decoder.output_conv + argmax (openset_head.hip's chain through map_common.h, so `label` is
//                  predict_head's bits) and, from the same 16 registers, the feature pixel's squared Mahalanobis
//                  distances to K whitened class means, the distance to the background Gaussian, the nearest mean's
//                  class, the 16-bit codes of both scores and their [kind][group][code] histograms.
//   density_rows   the same scores for feature rows of C = 16 NT channels, NT <= 8.
//
// Arithmetic (include/mdil_density.h): w = x - pivot; z = A w and z0 = A0 w as FMA chains over j ascending (what
// lies above the diagonal is zero and adds nothing); d_k = sum_i (z_i - m_k,i)^2 as differences (the expanded form cancels); the
// minimum by strict `<` with k ascending, a NaN winning; maha = dmin + 0.0f, rmaha = (dmin - d0) + 0.0f.
//
// density_head.  A lane owns one feature pixel.  z_i and z0_i are FMA chains on the VALU over row i of A and A0, read
// from LDS at wave-uniform addresses (whole rows: the zeros above the diagonal add nothing), and go straight into
// the K + 1 running sums, so no z is kept; the head's 4 x nc x 16 FMAs follow per parity.  The
// scores belong to the feature pixel, so the histogram gets ONE add per (kind, group) of weight 0..4 (how many of
// its four output pixels lie in that group), not four.
//
// density_rows.  A work-group takes 64 rows per trip, a wave 16 of them.  The rows are staged in LDS with the
// pivot subtracted (row stride C + 4 floats: the MFMA's A operand, lane l <- row l & 15, column 4 s + (l >> 4),
// hits 64 banks).  v_mfma_f32_16x16x4_f32 forms the 16 x 16 tiles of Z = W A^T and Z0 = W A0^T.  The model is staged
// in LDS once per work-group: of A and A0 only the 16 x 16 tiles on and below the diagonal, NT (NT + 1) / 2 each (36 KB
// each at C = 128, so both fit beside the rows, the means and the table: 133,508 B of the 163,840 a work-group may declare), every tile stored k-major,
// T[c][r] = A[16 ct + r][16 sb + c], so that the B operand of step s is the 64 consecutive floats at 64 (s & 3): lane l
// reads float l, no bank conflict.  One A-operand read serves up to 2 NT MFMAs.  (-DMDIL_DENSITY_ROWS_MODEL_IN_LDS=0
// builds the form that reads the B operand from global memory instead; tools/bench_density_variants.py times both.)  d0 is summed
// in the accumulator layout (four xor-shuffles).  Z goes back to LDS over the wave's own rows, and for the
// distances four lanes share a row, each a quarter of the channels held in registers against the means in LDS, the
// quarters added by two xor-shuffles: every lane of the four ends with the same bits.
//
// The histogram.  openset_head.hip's three levels, built for the input that is normal here, hundreds of occupied
// bins per kind:
//   1. the wave merges lanes of equal (kind, group, code) by ballots, but a round that gathers fewer than
//      kMinMerged lanes ends the merging: on spread codes the wave pays one round, not kMergeRounds;
//   2. the work-group's LDS table (map_common.h's cached_add_probed, flush_cache) is probed at two slots before an
//      add goes to global memory;
//   3. 64-bit global atomics, relaxed, agent scope.
// Integer sums throughout: the result does not depend on the order of arrival.
#include "../../include/mdil_density.h"
#include "map_common.h"

// The constants that tools/bench_density_variants.py varies, one per build; the defaults are what ships.
#ifndef MDIL_DENSITY_HEAD_WAVES
#define MDIL_DENSITY_HEAD_WAVES 3
#endif
#ifndef MDIL_DENSITY_HEAD_BLOCKS
#define MDIL_DENSITY_HEAD_BLOCKS 768
#endif
#ifdef MDIL_DENSITY_ROWS_BLOCKS
#define MDIL_DENSITY_ROWS_BLOCKS_WIDE MDIL_DENSITY_ROWS_BLOCKS
#else
#define MDIL_DENSITY_ROWS_BLOCKS 512
#define MDIL_DENSITY_ROWS_BLOCKS_WIDE 256
#endif
#ifndef MDIL_DENSITY_MERGE_ROUNDS
#define MDIL_DENSITY_MERGE_ROUNDS 8
#endif
#ifndef MDIL_DENSITY_MIN_MERGED
#define MDIL_DENSITY_MIN_MERGED 8
#endif
#ifndef MDIL_DENSITY_ROWS_MODEL_IN_LDS
#define MDIL_DENSITY_ROWS_MODEL_IN_LDS 1
#endif

namespace {

constexpr int kMaxC = MDIL_DENSITY_MAX_CLASSES;
constexpr int kMaxK = MDIL_DENSITY_MAX_MEANS;
constexpr int kKinds = MDIL_DENSITY_KINDS;
constexpr int kCodes = MDIL_DENSITY_CODES;
constexpr int kHeadWG = 256;
constexpr int kHeadMaxBlocks = MDIL_DENSITY_HEAD_BLOCKS;   // 768: beyond 196,608 feature pixels the loop strides
constexpr int kHeadSlots = 4096;                     // LDS table of (key, count): 32 KB
constexpr int kRowsWG = 256;
constexpr int kRowsPerTrip = 64;                     // 16 per wave
constexpr int kRowsMaxBlocks = MDIL_DENSITY_ROWS_BLOCKS;   // 512: beyond 32,768 rows the loop strides
// C >= 96 (NT >= 6): registers and LDS leave one work-group per CU, and one per CU is the bound: 256.  At 49,152 rows of
// 128 channels 256 / 512 / 1,024 work-groups took 84 / 88 / 92 us with both histograms, 50 / 58 / 66 us without.
constexpr int kRowsMaxBlocksWide = MDIL_DENSITY_ROWS_BLOCKS_WIDE;
constexpr int kLdsBytes = 163840;                    // what one work-group may declare on gfx950
constexpr int kMergeRounds = MDIL_DENSITY_MERGE_ROUNDS;
constexpr int kMinMerged = MDIL_DENSITY_MIN_MERGED;                        // a round that gathers fewer lanes ends the merging
constexpr char kFnHead[] = "density_head";
constexpr char kFnRows[] = "density_rows";

// table[slot] += wgt for every lane of the wave, wgt in [0, 7]; every lane calls it (the caller's loop is
// wave-uniform).  Lanes of one slot are gathered into one add while that pays.
template <int SLOTS>
__device__ __forceinline__ void wave_merged_add(u64* __restrict__ hist, uint32_t* tags, uint32_t* counts,
                                                uint32_t slot, uint32_t wgt) {
  const int lane = threadIdx.x & 63;
  bool active = wgt != 0u;
  u64 todo = __ballot(active);
  for (int round = 0; round < kMergeRounds && todo; ++round) {
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
    const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)slot, leader);
    const bool mine = active && slot == s0;
    const u64 same = __ballot(mine);
    const uint32_t total = (uint32_t)__popcll(__ballot(mine && (wgt & 1u))) +
                           2u * (uint32_t)__popcll(__ballot(mine && (wgt & 2u))) +
                           4u * (uint32_t)__popcll(__ballot(mine && (wgt & 4u)));
    if (lane == leader) cached_add_probed<SLOTS, 2>(hist, tags, counts, s0, total);
    active = active && !mine;
    todo &= ~same;
    if (__popcll(same) < kMinMerged) break;                        // uniform over the wave
  }
  if (active) cached_add_probed<SLOTS, 2>(hist, tags, counts, slot, wgt);
}

// min over k by strict `<`, k ascending; a NaN replaces any number and is never replaced
__device__ __forceinline__ void vote_min(int k, float d, float& best, int& bk) {
  const bool t = k == 0 || d < best || (d != d && best == best);
  best = t ? d : best;
  bk = t ? k : bk;
}

// 3 waves per SIMD: 768 work-groups are then resident at once (168 VGPRs, 20 of them spilled); at 2 the 768 ran as a
// full round and a half-empty one, and the kernel without a histogram took 195 us instead of 120 (6 x 256 x 512 x 16)
__global__ __launch_bounds__(kHeadWG, MDIL_DENSITY_HEAD_WAVES) void density_head_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, long long npix, int W,
    int nc, const float* __restrict__ model, const unsigned char* __restrict__ cls, int K,
    const unsigned char* __restrict__ target, const unsigned char* __restrict__ group_lut, int const_group, int kinds,
    int map_kind, unsigned char* __restrict__ label, unsigned char* __restrict__ nearest,
    unsigned short* __restrict__ code, u64* __restrict__ hist, u64* __restrict__ nonfinite, u64* __restrict__ agree) {
  __shared__ __attribute__((aligned(16))) float Wp[4][kMaxC][16];   // [a*2+b][c][ci]
  __shared__ float Bl[kMaxC];
  __shared__ __attribute__((aligned(16))) float Pv[16], Al[16][16], A0l[16][16], M0l[16], Mt[16][kMaxK];   // Mt[i][k] = m[k][i]
  __shared__ uint32_t Kl[kMaxK];                                     // class of mean k
  __shared__ uint32_t Gl[256];                                       // group of a target byte
  __shared__ uint32_t Tl[kHeadSlots], Cl[kHeadSlots];
  __shared__ uint32_t nf, ag[2];
  static_assert(MDIL_DENSITY_MAX_PIXELS / 4 / kHeadMaxBlocks * 4 <= 0x80000000LL, "a slot's count could wrap");
  stage_parity<kHeadWG>(w, bias, nc, Wp, Bl);
  for (int i = threadIdx.x; i < 16; i += kHeadWG) {
    Pv[i] = model[i];
    M0l[i] = model[16 + 512 + i];
  }
  for (int i = threadIdx.x; i < 256; i += kHeadWG) {
    (&Al[0][0])[i] = model[16 + i];
    (&A0l[0][0])[i] = model[16 + 256 + i];
  }
  for (int i = threadIdx.x; i < 16 * kMaxK; i += kHeadWG) {
    const int k = i & (kMaxK - 1), c = i / kMaxK;
    Mt[c][k] = k < K ? model[32 + 512 + k * 16 + c] : 0.f;
  }
  for (int i = threadIdx.x; i < K; i += kHeadWG) Kl[i] = (uint32_t)cls[i];
  if (hist) {
    for (int i = threadIdx.x; i < kHeadSlots; i += kHeadWG) {
      Tl[i] = kEmptySlot;
      Cl[i] = 0u;
    }
  }
  for (int i = threadIdx.x; i < 256; i += kHeadWG) Gl[i] = target ? (uint32_t)group_lut[i] : (uint32_t)const_group;
  if (threadIdx.x == 0) nf = ag[0] = ag[1] = 0u;
  __syncthreads();

  const bool scoring = nearest || code || hist || nonfinite || agree;
  uint32_t bad = 0u, known = 0u, same_class = 0u;
  // the trip count is the same for every lane of the work-group
  for (long long base = (long long)blockIdx.x * kHeadWG; base < npix; base += (long long)gridDim.x * kHeadWG) {
    const bool valid = base + threadIdx.x < npix;
    const long long p = valid ? base + threadIdx.x : npix - 1;     // a lane past the end: a clamped pixel, no writes
    f32x4 xv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xv[k] = *reinterpret_cast<const f32x4*>(x + p * 16 + k * 4);
    const long long r = p / W;                                     // n * H + h
    const long long o0 = (2 * r * 2 * W) + 2 * (p - r * W);        // pixel (2h, 2w); row below: + 2W
    uint32_t groups = 0u;                                          // byte a*2+b
    if (target) groups = quad_bytes(target, o0, W);

    uint32_t cd[kKinds] = {0u, 0u}, near = (uint32_t)MDIL_DENSITY_NO_CLASS;
    bool finite = true;
    if (scoring) {
      float wv[16], d[kMaxK];
#pragma unroll
      for (int i = 0; i < 16; ++i) wv[i] = __fsub_rn(xv[i >> 2][i & 3], Pv[i]);
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) d[k] = 0.f;
      float d0 = 0.f;
      // i stays a loop: it indexes LDS alone, and z_i, z0_i go straight into the K + 1 sums.  Row i is read whole;
      // the zeros above the diagonal leave the chain's bits alone.
#pragma unroll 1
      for (int i = 0; i < 16; ++i) {
        float a = 0.f, a0 = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 av = *reinterpret_cast<const f32x4*>(&Al[i][q * 4]);
          const f32x4 a0v = *reinterpret_cast<const f32x4*>(&A0l[i][q * 4]);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            a = __builtin_fmaf(av[e], wv[q * 4 + e], a);
            a0 = __builtin_fmaf(a0v[e], wv[q * 4 + e], a0);
          }
        }
        const float t0 = __fsub_rn(a0, M0l[i]);
        d0 = __builtin_fmaf(t0, t0, d0);
#pragma unroll
        for (int kq = 0; kq < kMaxK / 4; ++kq) {
          if (kq * 4 < K) {                                        // uniform; means past K are zeros and never voted on
            const f32x4 mv = *reinterpret_cast<const f32x4*>(&Mt[i][kq * 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float t = __fsub_rn(a, mv[e]);
              d[kq * 4 + e] = __builtin_fmaf(t, t, d[kq * 4 + e]);
            }
          }
        }
      }
      float dmin = 0.f;
      int bk = 0;
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) {
        if (k < K) {
          vote_min(k, d[k], dmin, bk);
          finite = finite && is_finite(d[k]);
        }
      }
      finite = finite && is_finite(d0);
      cd[0] = order_key16(__fadd_rn(dmin, 0.0f));
      cd[1] = order_key16(__fadd_rn(__fsub_rn(dmin, d0), 0.0f));
      near = finite ? Kl[bk] : (uint32_t)MDIL_DENSITY_NO_CLASS;
      bad += valid && !finite ? 4u : 0u;
    }

    if (label || agree) {
      uint32_t labels = 0u;
#pragma unroll 1
      for (int par = 0; par < 4; ++par) {
        float d[kMaxC];
        parity_logits<kMaxC>(xv, Wp, Bl, par, nc, d);                // predict_head.hip's chain, per parity
        float m = 0.f;
        int bi = 0;
#pragma unroll
        for (int c = 0; c < kMaxC; ++c)
          if (c < nc) vote(c, d[c], m, bi);
        labels |= (uint32_t)bi << (8 * par);
        const uint32_t g = target ? Gl[(groups >> (8 * par)) & 0xffu] : (uint32_t)const_group;
        known += valid && g == 0u ? 1u : 0u;
        same_class += valid && g == 0u && near == (uint32_t)bi ? 1u : 0u;
      }
      if (valid && label) {
        *reinterpret_cast<uint16_t*>(label + o0) = (uint16_t)(labels & 0xffffu);
        *reinterpret_cast<uint16_t*>(label + o0 + 2LL * W) = (uint16_t)(labels >> 16);
      }
    }

    if (hist) {
      uint32_t n_g[2] = {0u, 0u};
#pragma unroll
      for (int par = 0; par < 4; ++par) {
        const uint32_t g = target ? Gl[(groups >> (8 * par)) & 0xffu] : (uint32_t)const_group;
        n_g[0] += g == 0u ? 1u : 0u;
        n_g[1] += g == 1u ? 1u : 0u;
      }
      const bool counts = valid && finite;
#pragma unroll
      for (int k = 0; k < kKinds; ++k) {
        if (kinds >> k & 1) {                                      // uniform over the grid
#pragma unroll
          for (int g = 0; g < 2; ++g)
            wave_merged_add<kHeadSlots>(hist, Tl, Cl, (uint32_t)(k * 2 + g) * (uint32_t)kCodes + cd[k],
                                        counts ? n_g[g] : 0u);
        }
      }
    }

    if (valid && nearest) {
      const uint16_t two = (uint16_t)(near | near << 8);
      *reinterpret_cast<uint16_t*>(nearest + o0) = two;
      *reinterpret_cast<uint16_t*>(nearest + o0 + 2LL * W) = two;
    }
    if (valid && code) {
      uint32_t mine = map_kind == 1 ? cd[1] : cd[0];
      mine = finite ? mine : (uint32_t)MDIL_DENSITY_NONFINITE_CODE;
      mine |= mine << 16;
      *reinterpret_cast<uint32_t*>(code + o0) = mine;
      *reinterpret_cast<uint32_t*>(code + o0 + 2LL * W) = mine;
    }
  }

  if (bad) atomicAdd(&nf, bad);
  if (agree) {                                                     // uniform; below 2^26 per lane: 2^40 / 768 / 256
    known = wave_sum_u32(known);
    same_class = wave_sum_u32(same_class);
    if ((threadIdx.x & 63) == 0) {
      if (known) atomicAdd(&ag[0], known);
      if (same_class) atomicAdd(&ag[1], same_class);
    }
  }
  __syncthreads();                                                 // every lane of the work-group is here
  if (nonfinite && threadIdx.x == 0 && nf) atomicAdd(nonfinite, (u64)nf);
  if (agree && threadIdx.x < 2 && ag[threadIdx.x]) atomicAdd(agree + threadIdx.x, (u64)ag[threadIdx.x]);
  if (hist) flush_cache<kHeadWG, kHeadSlots>(hist, Tl, Cl);
}

// NT: 16-channel groups of a row.
template <int NT>
__global__ __launch_bounds__(kRowsWG) void density_rows_kernel(
    const float* __restrict__ x, long long rows, const float* __restrict__ model,
    const unsigned char* __restrict__ cls, int K, const unsigned char* __restrict__ group, int const_group, int kinds,
    int map_kind, unsigned char* __restrict__ nearest, unsigned short* __restrict__ code, u64* __restrict__ hist,
    u64* __restrict__ nonfinite) {
  constexpr int C = 16 * NT, S = C + 4, CQ = C / 4;
  constexpr int kSlots = NT <= 4 ? 4096 : 1024;                    // 32 KB where the rest is small; NT = 5 keeps two work-groups per CU
  constexpr int kTri = NT * (NT + 1) / 2;                          // 16 x 16 tiles on and below the diagonal
  __shared__ __attribute__((aligned(16))) float Ws[kRowsPerTrip * S];   // the rows minus the pivot, then Z
  __shared__ __attribute__((aligned(16))) float Ms[kMaxK * C];
  __shared__ __attribute__((aligned(16))) float Pv[C], M0s[C];
  __shared__ float D0s[kRowsPerTrip];
  __shared__ uint32_t Kl[kMaxK];
  __shared__ uint32_t Tl[kSlots], Cl[kSlots];
  __shared__ uint32_t nf;
  const float* __restrict__ Ag = model + C;
  const float* __restrict__ A0g = model + C + C * C;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
#if MDIL_DENSITY_ROWS_MODEL_IN_LDS
  __shared__ __attribute__((aligned(16))) float At[kTri * 256], A0t[kTri * 256];   // tile (ct, sb <= ct), k-major
  static_assert(sizeof(float) * (kRowsPerTrip * S + kMaxK * C + 2 * C + kRowsPerTrip + 2 * kTri * 256) +
                    4 * (kMaxK + 2 * kSlots + 1) <= kLdsBytes, "LDS of a work-group");
  for (int e = t; e < NT * NT * 256; e += kRowsWG) {               // consecutive lanes read consecutive floats of a row of A
    const int ct = e / (NT * 256), sb = (e >> 8) % NT, r = (e >> 4) & 15, c = e & 15;
    if (sb <= ct) {
      const int src = (16 * ct + r) * C + 16 * sb + c, dst = (ct * (ct + 1) / 2 + sb) * 256 + c * 16 + r;
      At[dst] = Ag[src];
      A0t[dst] = A0g[src];
    }
  }
#else
  static_assert(sizeof(float) * (kRowsPerTrip * S + kMaxK * C + 2 * C + kRowsPerTrip) + 4 * (kMaxK + 2 * kSlots + 1) <=
                    kLdsBytes, "LDS of a work-group");
#endif
  for (int i = t; i < C; i += kRowsWG) {
    Pv[i] = model[i];
    M0s[i] = model[C + 2 * C * C + i];
  }
  for (int i = t; i < K * C; i += kRowsWG) Ms[i] = model[2 * C + 2 * C * C + i];
  for (int i = t; i < K; i += kRowsWG) Kl[i] = (uint32_t)cls[i];
  if (hist) {
    for (int i = t; i < kSlots; i += kRowsWG) {
      Tl[i] = kEmptySlot;
      Cl[i] = 0u;
    }
  }
  if (t == 0) nf = 0u;

  uint32_t bad = 0u;
  // the trip count is the same for every lane of the work-group
  for (long long row0 = (long long)blockIdx.x * kRowsPerTrip; row0 < rows;
       row0 += (long long)gridDim.x * kRowsPerTrip) {
    __syncthreads();                                               // the tables; the trip before this one
    for (int e = t; e < kRowsPerTrip * (C / 4); e += kRowsWG) {
      const int r = e / (C / 4), c4 = (e - r * (C / 4)) * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (row0 + r < rows) {
        v = *reinterpret_cast<const f32x4*>(x + (row0 + r) * C + c4);
        v -= *reinterpret_cast<const f32x4*>(&Pv[c4]);
      }
      *reinterpret_cast<f32x4*>(&Ws[r * S + c4]) = v;
    }
    __syncthreads();

    // Z and Z0 of the wave's 16 rows: tile ct holds columns 16 ct .. 16 ct + 15; step s the channels 4 s .. 4 s + 3
    f32x4 acc[NT], acc0[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) acc[ct] = acc0[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wr = &Ws[(16 * wave + (lane & 15)) * S + (lane >> 4)];
#pragma unroll
    for (int s = 0; s < 4 * NT; ++s) {
      const float a = wr[4 * s];
#pragma unroll
      for (int ct = s / 4; ct < NT; ++ct) {                        // above the diagonal A is zero: not formed
#if MDIL_DENSITY_ROWS_MODEL_IN_LDS
        const int o = (ct * (ct + 1) / 2 + s / 4) * 256 + (s & 3) * 64 + lane;   // k = 4 (s & 3) + (l >> 4), r = l & 15
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, At[o], acc[ct], 0, 0, 0);
        acc0[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, A0t[o], acc0[ct], 0, 0, 0);
#else
        const int o = (16 * ct + (lane & 15)) * C + 4 * s + (lane >> 4);
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Ag[o], acc[ct], 0, 0, 0);
        acc0[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, A0g[o], acc0[ct], 0, 0, 0);
#endif
      }
    }
    // register i of lane l: row 4 (l >> 4) + i, column l & 15 of the tile
    float p0[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
      const float m0 = M0s[16 * ct + (lane & 15)];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float d = __fsub_rn(acc0[ct][i], m0);
        p0[i] = __builtin_fmaf(d, d, p0[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int m = 1; m <= 8; m <<= 1) p0[i] += __shfl_xor(p0[i], m, 64);
    }
    __syncthreads();                                               // every wave has read its rows of W
    if ((lane & 15) == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) D0s[16 * wave + 4 * (lane >> 4) + i] = p0[i];
    }
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
#pragma unroll
      for (int i = 0; i < 4; ++i) Ws[(16 * wave + 4 * (lane >> 4) + i) * S + 16 * ct + (lane & 15)] = acc[ct][i];
    }
    __syncthreads();

    // four lanes per row: lane l has row l & 15 of the wave's and the channels [q CQ, (q + 1) CQ), q = l >> 4
    const int rl = 16 * wave + (lane & 15), q = lane >> 4;
    const long long row = row0 + rl;
    const bool valid = row < rows;
    float zq[CQ];
#pragma unroll
    for (int i = 0; i < CQ; i += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(&Ws[rl * S + q * CQ + i]);
#pragma unroll
      for (int e = 0; e < 4; ++e) zq[i + e] = v[e];
    }
    const float d0 = D0s[rl];
    float dmin = 0.f;
    int bk = 0;
    bool finite = true;
    for (int k = 0; k < K; ++k) {
      float d = 0.f;
#pragma unroll
      for (int i = 0; i < CQ; i += 4) {
        const f32x4 mv = *reinterpret_cast<const f32x4*>(&Ms[k * C + q * CQ + i]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float dd = __fsub_rn(zq[i + e], mv[e]);
          d = __builtin_fmaf(dd, dd, d);
        }
      }
      d += __shfl_xor(d, 16, 64);
      d += __shfl_xor(d, 32, 64);                                  // the same bits in the four lanes of a row
      vote_min(k, d, dmin, bk);
      finite = finite && is_finite(d);
    }
    finite = finite && is_finite(d0);
    uint32_t cd[kKinds];
    cd[0] = order_key16(__fadd_rn(dmin, 0.0f));
    cd[1] = order_key16(__fadd_rn(__fsub_rn(dmin, d0), 0.0f));
    if (valid && q == 0) {
      bad += finite ? 0u : 1u;
      if (nearest) nearest[row] = (unsigned char)(finite ? Kl[bk] : (uint32_t)MDIL_DENSITY_NO_CLASS);
      if (code) {
        const uint32_t mine = map_kind == 1 ? cd[1] : cd[0];
        code[row] = (unsigned short)(finite ? mine : (uint32_t)MDIL_DENSITY_NONFINITE_CODE);
      }
    }
    if (hist) {                                                    // lanes q = 0 count kind 0, q = 1 kind 1
      uint32_t g = (uint32_t)const_group;
      if (group && valid) g = (uint32_t)group[row];
      const bool counts = valid && finite && q < kKinds && (kinds >> q & 1) && g < 2u;
      wave_merged_add<kSlots>(hist, Tl, Cl, ((uint32_t)((q & 1) * 2) + (g & 1u)) * (uint32_t)kCodes + cd[q & 1],
                              counts ? 1u : 0u);
    }
  }

  if (bad) atomicAdd(&nf, bad);
  __syncthreads();
  if (nonfinite && t == 0 && nf) atomicAdd(nonfinite, (u64)nf);
  if (hist) flush_cache<kRowsWG, kSlots>(hist, Tl, Cl);
}

// What both entry points check alike.
bool model_ok(const char* fn, const float* model, const unsigned char* cls, int K, int const_group, int kinds,
              int map_kind, const void* code, const void* groups, const void* lut) {
  if (!model || !cls || K < 1 || K > MDIL_DENSITY_MAX_MEANS) {
    set_error("%s: the model (model %p cls %p) needs 1 <= K <= %d means, got K=%d", fn, (const void*)model,
              (const void*)cls, MDIL_DENSITY_MAX_MEANS, K);
    return false;
  }
  if (kinds < 1 || kinds > 3) {
    set_error("%s: kinds=%d outside [1, 3] (a bit mask: 1 maha, 2 rmaha)", fn, kinds);
    return false;
  }
  if (map_kind < -1 || map_kind >= MDIL_DENSITY_KINDS || (code != nullptr) != (map_kind >= 0)) {
    set_error("%s: map_kind=%d with code %p (a code map needs a map_kind in [0, 1]; without one map_kind is -1)", fn,
              map_kind, code);
    return false;
  }
  if (const_group < 0 || const_group > 2) {
    set_error("%s: const_group=%d outside [0, 2]", fn, const_group);
    return false;
  }
  if (groups && !lut) {
    set_error("%s: a target needs its group_lut (u8 [256])", fn);
    return false;
  }
  return true;
}

}  // namespace

API int mdil_density_version(void) { return 100; }
API const char* mdil_density_last_error(void) { return g_err; }

API int mdil_density_head(const float* x, const float* w, const float* bias, int N, int H, int W, int nc,
                          const float* model, const unsigned char* cls, int K, const unsigned char* target,
                          const unsigned char* group_lut, int const_group, int kinds, int map_kind,
                          unsigned char* label, unsigned char* nearest, unsigned short* code, long long* hist,
                          long long* nonfinite, long long* agree, void* stream) {
  if (!x || !w || !bias || N <= 0 || H <= 0 || W <= 0) {
    set_error("density_head: bad argument (x %p w %p bias %p N %d H %d W %d)", (const void*)x, (const void*)w,
              (const void*)bias, N, H, W);
    return MDIL_DENSITY_ERR_INVALID;
  }
  if (!label && !nearest && !code && !hist && !nonfinite && !agree) {
    set_error("density_head: nothing to write (label, nearest, code, hist, nonfinite and agree are all NULL)");
    return MDIL_DENSITY_ERR_INVALID;
  }
  if (!classes_ok(kFnHead, nc, MDIL_DENSITY_MIN_CLASSES, MDIL_DENSITY_MAX_CLASSES)) return MDIL_DENSITY_ERR_INVALID;
  if (!model_ok(kFnHead, model, cls, K, const_group, kinds, map_kind, code, target, group_lut))
    return MDIL_DENSITY_ERR_INVALID;
  if (((uintptr_t)x & 15) || ((uintptr_t)w & 3) || ((uintptr_t)bias & 3) || ((uintptr_t)model & 3) ||
      ((uintptr_t)target & 1) || ((uintptr_t)label & 1) || ((uintptr_t)nearest & 1) || ((uintptr_t)code & 3) ||
      ((uintptr_t)hist & 7) || ((uintptr_t)nonfinite & 7) || ((uintptr_t)agree & 7)) {
    set_error("density_head: alignment (x 16 B; w, bias and model 4 B; target, label and nearest 2 B; code 4 B; hist, "
              "nonfinite and agree 8 B)");
    return MDIL_DENSITY_ERR_INVALID;
  }
  if (!shape_ok(N, H, W, MDIL_DENSITY_MAX_PIXELS / 4)) {
    set_error("density_head: too large (N %d, features %d x %d: at most 2^40 output pixels)", N, H, W);
    return MDIL_DENSITY_ERR_INVALID;
  }
  const long long npix = (long long)N * H * W;
  const int grid = bounded_grid(npix, kHeadWG, kHeadMaxBlocks);
  hipLaunchKernelGGL(density_head_kernel, dim3(grid), dim3(kHeadWG), 0, (hipStream_t)stream, x, w, bias, npix, W, nc,
                     model, cls, K, target, group_lut, const_group, kinds, map_kind, label, nearest, code,
                     reinterpret_cast<u64*>(hist), reinterpret_cast<u64*>(nonfinite), reinterpret_cast<u64*>(agree));
  return launched(kFnHead) ? MDIL_DENSITY_OK : MDIL_DENSITY_ERR_LAUNCH;
}

API int mdil_density_rows(const float* x, long long rows, int C, const float* model, const unsigned char* cls, int K,
                          const unsigned char* group, int const_group, int kinds, int map_kind,
                          unsigned char* nearest, unsigned short* code, long long* hist, long long* nonfinite,
                          void* stream) {
  if (!x || rows < 1 || rows > MDIL_DENSITY_MAX_ROWS) {
    set_error("density_rows: bad argument (x %p rows %lld: 1 to 2^24 rows)", (const void*)x, rows);
    return MDIL_DENSITY_ERR_INVALID;
  }
  if (C < 16 || C > MDIL_DENSITY_MAX_CHANNELS || C % 16) {
    set_error("density_rows: C=%d is not a multiple of 16 in [16, %d]", C, MDIL_DENSITY_MAX_CHANNELS);
    return MDIL_DENSITY_ERR_INVALID;
  }
  if (!nearest && !code && !hist && !nonfinite) {
    set_error("density_rows: nothing to write (nearest, code, hist and nonfinite are all NULL)");
    return MDIL_DENSITY_ERR_INVALID;
  }
  if (!model_ok(kFnRows, model, cls, K, const_group, kinds, map_kind, code, nullptr, nullptr))
    return MDIL_DENSITY_ERR_INVALID;
  if (((uintptr_t)x & 15) || ((uintptr_t)model & 3) || ((uintptr_t)code & 1) || ((uintptr_t)hist & 7) ||
      ((uintptr_t)nonfinite & 7)) {
    set_error("density_rows: alignment (x 16 B; model 4 B; code 2 B; hist and nonfinite 8 B)");
    return MDIL_DENSITY_ERR_INVALID;
  }
  const int grid = bounded_grid(rows, kRowsPerTrip, C >= 96 ? kRowsMaxBlocksWide : kRowsMaxBlocks);
  hipStream_t st = (hipStream_t)stream;
#define MDIL_DENSITY_CASE(NT)                                                                                       \
  case NT:                                                                                                          \
    hipLaunchKernelGGL((density_rows_kernel<NT>), dim3(grid), dim3(kRowsWG), 0, st, x, rows, model, cls, K, group,  \
                       const_group, kinds, map_kind, nearest, code, reinterpret_cast<u64*>(hist),                   \
                       reinterpret_cast<u64*>(nonfinite));                                                          \
    break;
  switch (C / 16) {
    MDIL_DENSITY_CASE(1) MDIL_DENSITY_CASE(2) MDIL_DENSITY_CASE(3) MDIL_DENSITY_CASE(4)
    MDIL_DENSITY_CASE(5) MDIL_DENSITY_CASE(6) MDIL_DENSITY_CASE(7) MDIL_DENSITY_CASE(8)
  }
#undef MDIL_DENSITY_CASE
  return launched(kFnRows) ? MDIL_DENSITY_OK : MDIL_DENSITY_ERR_LAUNCH;
}
