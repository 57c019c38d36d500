// flat_prescan.hip.h -- a BATCH of the brute-force scan (vers_flat_search[_dev], b >= 2, top_k <= 48) on the matrix cores over the flat
// handle's fp16 shadow, with the exact finish of the list scans.  Option "flat_prescan" = 1 (default 0: DESIGN.md section 6 says why).
//
// The scheme is prescan.hip.h's -- pre-select on an approximate val, certify, re-score exactly, re-scan what does not certify -- but the
// work is another: no lists, no probe plan, no quads; every query meets every row.  What there is to reuse is the QUERY BLOCK: up to 64
// queries sit in LDS while a segment of the corpus streams past once.
//   (1) flat_prescan_kernel<SETS, LO>: a block = (row segment, query block of 32 SETS queries).  The query block is staged once
//       (shadow_mma.hip.h's planes); hi alone (LO = false) where hi + lo does not fit the CU's 160 KB: 64 x 768 x 2 B = 98 KB.  The block's
//       waves deal the segment's 64-row tiles round-robin through the load ring of shadow_mma.hip.h (ShadowRing, every W-th tile).
//       Per tile and set: lo MFMA, hi MFMA per row piece (the small term first, as prescan_item_g), then |x|^2 as one more k-step
//       (v_mfma_f32_32x32x2_f32) -- the accumulation RescoreArgs::shadow = 1 (hi + lo) / 2 (hi only) is the audited error model of.
//         val = |x|^2 - 2 <x~, q>      (cosine distance: -<x~, q>)
//       CANDIDATES.  Per (query, wave) ONE sorted list of the kp = top_k + slack smallest (val, row) keys, one key per lane, in LDS
//       (the wave's own: no lock, no spin, no shared buffer).  Its last val is the query's threshold, shared with the query's other
//       waves and segments through one atomicMin word per query in HBM that travels back with the tile's last load.  The path from the
//       accumulators to the lists is the list offer of shadow_mma.hip.h, a (set, row half) at a time through the wave's 4 KiB LDS
//       slice.  Rows at or beyond n (the last tile's padding, row_ids = 0xFFFFFFFF) never enter a list; a non-finite val of a real
//       row flags its query (qflags) for the exact re-scan.
//       At the segment's end the waves' lists are folded per query (wave_merge_sorted64) into the slot (query, segment) of kp keys.
//   (2) ivf_rescore_kernel on slots [b][n_segs][kp] with P = 1 (the corpus is ONE list from row 0), then fallback_kernel: unchanged.
#pragma once
#include "prescan.hip.h"
#include "shadow_mma.hip.h"

#pragma clang fp contract(off)

namespace vers {

constexpr int64_t kFlatPrescanDefault = 0;
constexpr int kFlpWaves = 4;      // waves of a block at most (fewer where the lists would not fit: flat_prescan_plan)
constexpr int kFlpTrPitch = 33;   // floats per row of a wave's transpose slice (shadow_list_offer<32>: 32 queries + 1)
constexpr uint32_t kFlpLdsMax = 160u * 1024u;

struct FlatPreArgs {
  const uint16_t* rows_h;  // the fp16 shadow
  const float* xnorm;      // |x|^2 per storage row (0 for the last tile's padding rows)
  const float* qp;         // zero padded queries [b][ld]
  uint64_t* partials;      // [b][n_segs][kp]
  uint32_t* bounds32;      // [b] order bits of the smallest known kp-th val of the query (0xFFFFFFFF: none yet)
  uint32_t* qflags;        // [b] != 0: a non-finite val
  uint32_t ld, kp, metric, n_rows, b, n_segs, seg_tiles;
};

// how a call is cut: query blocks of nq slots (32 | 64), hi + lo or hi only, waves per block, segments of seg_tiles 64-row tiles
struct FlatPrePlan {
  uint32_t nq, lo, waves, seg_tiles, n_segs, n_qb;
  size_t lds;
  bool ok;
};
inline size_t flat_prescan_lds_bytes(uint32_t ld, uint32_t nq, uint32_t lo, uint32_t waves, uint32_t kp) {  // query block | transpose slices | lists
  return (size_t)ld * nq * 2u * (1u + lo) + (size_t)waves * 32u * kFlpTrPitch * sizeof(float) + (size_t)waves * nq * kp * sizeof(uint64_t);
}
// n rows, b queries, ld padded columns, n_cu compute units (seg_plan's inputs) and the list width.  Widest block first: 64 queries when the
// batch has more than 32; hi + lo where it fits with four waves, else hi only with four, three, two waves; then the same for 32 queries.
// Segments: one block per resident slot of the GPU when the batch is one query block (small b), fewer and longer ones as the query blocks
// multiply -- the shadow is then streamed once per query block --, at least one tile per wave.
inline FlatPrePlan flat_prescan_plan(uint64_t n, uint32_t b, uint32_t ld, int n_cu, uint32_t kp) {
  FlatPrePlan p{};
  for (uint32_t nq = b > 32u ? 64u : 32u; nq >= 32u && !p.ok; nq -= 32u) {
    const uint32_t tries[4][2] = {{1u, 4u}, {0u, 4u}, {0u, 3u}, {0u, 2u}};
    for (const auto& t : tries) {
      const size_t lds = flat_prescan_lds_bytes(ld, nq, t[0], t[1], kp);
      if (lds <= kFlpLdsMax) { p.nq = nq; p.lo = t[0]; p.waves = t[1]; p.lds = lds; p.ok = true; break; }
    }
  }
  if (!p.ok || n == 0) { p.ok = false; return p; }
  p.n_qb = (b + p.nq - 1u) / p.nq;
  const uint64_t n_tiles = (n + 63u) / 64u;
  const uint32_t per_cu = p.lds * 2u <= kFlpLdsMax ? 2u : 1u;
  const uint64_t want = std::max<uint64_t>(1u, ((uint64_t)n_cu * per_cu + p.n_qb - 1u) / p.n_qb);
  const uint64_t seg_tiles = std::max<uint64_t>(std::min<uint64_t>(p.waves, n_tiles), (n_tiles + want - 1u) / want);
  p.seg_tiles = (uint32_t)seg_tiles;
  p.n_segs = (uint32_t)((n_tiles + seg_tiles - 1u) / seg_tiles);
  if ((uint64_t)p.n_segs * p.n_qb >= 0x7FFFFFFFull) p.ok = false;
  return p;
}

struct FlatPreTables {  // the per-call tables of the scan and the finish, [b] words each (fail_list: [b + 1])
  uint32_t *pj_list, *pj_pref, *pj_nq, *qflags, *bounds32, *fail_list;
  uint32_t* fix;  // [0] list_off = 0 | [1] list_len = n | [2] failed certificates, [3] candidates re-scored since the last fold | u64 [2], [3]: their totals
};
constexpr uint32_t kFlpFixWords = 8;

// the launches (flat_prescan.hip)
int32_t launch_flat_pre_begin(const FlatPreTables& t, uint32_t b, uint32_t n_segs, uint32_t n, hipStream_t st);
int32_t launch_flat_prescan(const FlatPreArgs& a, const FlatPrePlan& p, hipStream_t st);

#ifdef VERS_FLAT_PRESCAN_KERNELS
// the call's tables (no memset: a plain kernel); thread 0 folds the previous calls' two counters into their 64-bit totals
static __global__ void flat_pre_begin_kernel(FlatPreTables t, uint32_t b, uint32_t n_segs, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < b) {
    t.pj_list[i] = 0u; t.pj_pref[i] = 0u; t.pj_nq[i] = n_segs; t.qflags[i] = 0u; t.bounds32[i] = 0xFFFFFFFFu;
  }
  if (i == 0) {
    t.fail_list[b] = 0u;
    t.fix[0] = 0u; t.fix[1] = n;
    unsigned long long* tot = reinterpret_cast<unsigned long long*>(t.fix + 4);
    tot[0] += t.fix[2]; tot[1] += t.fix[3];
    t.fix[2] = 0u; t.fix[3] = 0u;
  }
}

// shadow_list_offer's lists of a wave and a set of 32 queries: kp keys each in LDS, the corpus' real rows (lanes 0 .. 31 hold one each), keys (val, row)
struct FlatPreLists {
  static constexpr int kUnroll = 1;
  uint64_t* lists;
  uint32_t kp, n_rows;
  int lane;
  __device__ __forceinline__ bool row_ok(uint32_t row) const { return lane < 32 && row < n_rows; }
  __device__ __forceinline__ uint32_t key_lo(int, uint32_t row) const { return row; }
  __device__ __forceinline__ uint64_t load(int q) const { return (uint32_t)lane < kp ? lists[(size_t)q * kp + lane] : kKeyMax; }
  __device__ __forceinline__ void store(int q, uint64_t l) const { if ((uint32_t)lane < kp) lists[(size_t)q * kp + lane] = l; }
};

template <int SETS, bool LO>
__global__ __launch_bounds__(kWave * kFlpWaves) void flat_prescan_kernel(FlatPreArgs a) {
  constexpr int NQ = 32 * SETS;
  extern __shared__ __attribute__((aligned(16))) unsigned char flp_lds[];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t W = blockDim.x >> 6;
  const uint32_t n_cb = a.ld / 16u, kp = a.kp;
  const uint32_t q_entries = n_cb * 2u * NQ;  // f16x8 entries of the hi (and of the lo) part
  f16x8_t* const qh = reinterpret_cast<f16x8_t*>(flp_lds);
  float* const tr = reinterpret_cast<float*>(flp_lds + (size_t)q_entries * 16u * (LO ? 2u : 1u)) + (size_t)wid * 32u * kFlpTrPitch;
  uint64_t* const lists_all = reinterpret_cast<uint64_t*>(flp_lds + (size_t)q_entries * 16u * (LO ? 2u : 1u) + (size_t)W * 32u * kFlpTrPitch * sizeof(float));
  uint64_t* const lists = lists_all + (size_t)wid * NQ * kp;  // the wave's own: [NQ][kp]
  const uint32_t seg = blockIdx.x % a.n_segs, q0 = (blockIdx.x / a.n_segs) * NQ;
  const uint32_t nq_live = a.b - q0 < (uint32_t)NQ ? a.b - q0 : (uint32_t)NQ;
  const uint32_t n_tiles = (a.n_rows + kWave - 1) / kWave;
  const uint32_t t0 = seg * a.seg_tiles + (uint32_t)wid;
  const uint32_t t_end = (seg + 1u) * a.seg_tiles < n_tiles ? (seg + 1u) * a.seg_tiles : n_tiles;
  const uint32_t my_tiles = t0 < t_end ? (t_end - t0 + W - 1u) / W : 0u;
  ShadowRing ring{__builtin_amdgcn_make_buffer_rsrc((void*)a.rows_h, 0, (int)(n_tiles * a.ld * 128u), 0x00020000),  // (< 4 GiB: flat_shadow_derive)
                  a.xnorm, a.ld * 128u, a.ld / (16u * kShCbStep), t0, t_end, W};  // the wave's tiles t0, t0 + W, .. of the segment
  const uint32_t n_steps = my_tiles * ring.nst;
  const int n = lane & 31, hf = lane >> 5;

  // per-lane query constants: the lane's column of each set
  bool live[SETS];
  uint32_t slot[SETS];
  ShadowList sl[SETS];
#pragma unroll
  for (int s = 0; s < SETS; ++s) {
    live[s] = (uint32_t)(s * 32 + n) < nq_live;
    slot[s] = live[s] ? q0 + (uint32_t)(s * 32 + n) : q0;  // (dead columns: the unconditional loads read query q0's word)
    const uint32_t thr0 = live[s] ? __hip_atomic_load(a.bounds32 + slot[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;  // order bits; a stale word only prunes less
    sl[s] = ShadowList{thr0, thr0, ~0u, 0u};
  }

  // the ring is primed before the block stages, so that the first tiles fly meanwhile.  The shared thresholds travel with the steps; they
  // are consumed once per tile, with the step that completes it: on the other steps every lane reads ONE word
  uint32_t gthr[kShRing][SETS];
  auto extra = [&](int b, bool last) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < SETS; ++s) gthr[b][s] = __hip_atomic_load(a.bounds32 + (last ? slot[s] : q0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  if (n_steps > 0) ring.prime(lane, extra);

  // stage the query block; every wave clears its own lists
  const float scale = a.metric ? -1.0f : -2.0f;  // (exact scalings)
  shadow_stage_queries<NQ, LO>(qh, n_cb, [&](uint32_t c0, uint32_t qs, float (&y)[8]) __attribute__((always_inline)) {
    if (qs < nq_live) {
      const f32x4* src = reinterpret_cast<const f32x4*>(a.qp + (uint64_t)(q0 + qs) * a.ld + c0);
      const f32x4 v0 = src[0], v1 = src[1];
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] = scale * (j < 4 ? v0[j & 3] : v1[j & 3]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] = 0.0f;
    }
  });
  for (uint32_t i = (uint32_t)lane; i < (uint32_t)NQ * kp; i += kWave) lists[i] = kKeyMax;
  __syncthreads();

  f32x16_t acc[SETS][2];
#pragma unroll
  for (int s = 0; s < SETS; ++s)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[s][0][e] = acc[s][1][e] = 0.0f;

  const f16x8_t* const qhi = qh + (size_t)hf * NQ + n;
  const f16x8_t* const qlo = qhi + q_entries;
  auto mma = [&](uint32_t cc, const u32x4 (&r)[2 * kShCbStep]) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < kShCbStep; ++k) {
      const size_t e0 = (size_t)(cc * kShCbStep + k) * 2u * NQ;
#pragma unroll
      for (int s = 0; s < SETS; ++s) {
        const f16x8_t bh = qhi[e0 + 32 * s];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f16x8_t ar = __builtin_bit_cast(f16x8_t, r[2 * k + h]);
          if constexpr (LO) acc[s][h] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar, qlo[e0 + 32 * s], acc[s][h], 0, 0, 0);  // (small term first)
          acc[s][h] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar, bh, acc[s][h], 0, 0, 0);
        }
      }
    }
  };
  // end of tile t: the list offer of shadow_mma.hip.h, a set and a row half at a time, on the wave's LDS lists
  auto tile_done = [&](uint32_t t, float xnv, int b) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < SETS; ++s) shadow_tile_norm(acc[s], xnv, a.metric ? 0.0f : 1.0f, lane, live[s], gthr[b][s], sl[s]);
#pragma unroll
    for (int s = 0; s < SETS; ++s) {
      const uint32_t nq_set = nq_live > (uint32_t)(32 * s) ? (nq_live - 32u * s < 32u ? nq_live - 32u * s : 32u) : 0u;
      shadow_list_offer<32>(acc[s], t, lane, live[s], nq_set, kp, tr, a.bounds32 + slot[s], sl[s], FlatPreLists{lists + (size_t)(32 * s) * kp, kp, a.n_rows, lane});
    }
  };
  ring.run(n_steps, lane, extra, mma, tile_done);

  // the segment's end: the waves' lists of a query folded into its slot; wave w takes queries w, w + W, ...
  if (lane < 32) {
#pragma unroll
    for (int s = 0; s < SETS; ++s)
      if (live[s] && ((sl[s].bad >> n) & 1u)) a.qflags[slot[s]] = 1u;
  }
  __syncthreads();
  for (uint32_t qi = (uint32_t)wid; qi < nq_live; qi += W) {
    uint64_t list = kKeyMax;
    for (uint32_t w = 0; w < W; ++w) {
      const uint64_t other = (uint32_t)lane < kp ? lists_all[((size_t)w * NQ + qi) * kp + lane] : kKeyMax;
      wave_merge_sorted64(list, other, lane);
    }
    if ((uint32_t)lane < kp) a.partials[((uint64_t)(q0 + qi) * a.n_segs + seg) * kp + lane] = list;  // ascending, kKeyMax padded
  }
}
#endif  // VERS_FLAT_PRESCAN_KERNELS

}  // namespace vers
