// flat_prescan.hip.h -- a BATCH of the brute-force scan (vers_flat_search[_dev], b >= 2, top_k <= 48) on the matrix cores over the flat
// handle's fp16 shadow, with the exact finish of the list scans.  Option "flat_prescan" = 1 (default 0: DESIGN.md section 6 says why).
//
// The scheme is prescan.hip.h's -- pre-select on an approximate val, certify, re-score exactly, re-scan what does not certify -- but the
// work is another: no lists, no probe plan, no quads; every query meets every row.  What there is to reuse is the QUERY BLOCK: up to 64
// queries sit in LDS while a segment of the corpus streams past once.
//   (1) flat_prescan_kernel<SETS, LO>: a block = (row segment, query block of 32 SETS queries).  The query block is staged once as the B
//       operand of v_mfma_f32_32x32x16_f16 -- [hi | lo][column block of 16][octet][slot] x 16 bytes, the scaled query (-2 q, cosine: -q)
//       split into fp16 hi + lo; hi alone (LO = false) where hi + lo does not fit the CU's 160 KB: 64 x 768 x 2 B = 98 KB.  The block's
//       waves deal the segment's 64-row tiles round-robin.  A lane's row operand is ONE 16-byte non-temporal buffer load of the shadow
//       (rows_to_f16_kernel's layout) that goes into the MFMA as loaded; loads run kFlpRing steps ahead in registers, across tile ends.
//       Per tile and set: lo MFMA, hi MFMA per row piece (the small term first, as prescan_item_g), then |x|^2 as one more k-step
//       (v_mfma_f32_32x32x2_f32) -- the accumulation RescoreArgs::shadow = 1 (hi + lo) / 2 (hi only) is the audited error model of.
//         val = |x|^2 - 2 <x~, q>      (cosine distance: -<x~, q>)
//       CANDIDATES.  Per (query, wave) ONE sorted list of the kp = top_k + slack smallest (val, row) keys, one key per lane, in LDS
//       (the wave's own: no lock, no spin, no shared buffer).  Its last val is the query's threshold, shared with the query's other
//       waves and segments through one atomicMin word per query in HBM that travels back with the tile's last load.  A tile costs one
//       compare per accumulator register and one ballot; only when something passes (or is not finite) is the accumulator of that
//       (set, row half) transposed through the wave's 4 KiB LDS slice to row-per-lane and offered to the lists of its live queries
//       (wave_topk_update; a rank sort when the list is still empty).  Rows at or beyond n (the last tile's padding, row_ids =
//       0xFFFFFFFF) never enter a list; a non-finite val of a real row flags its query (qflags) for the exact re-scan.
//       At the segment's end the waves' lists are folded per query (wave_merge_sorted64) into the slot (query, segment) of kp keys.
//   (2) ivf_rescore_kernel on slots [b][n_segs][kp] with P = 1 (the corpus is ONE list from row 0), then fallback_kernel: unchanged.
#pragma once
#include "prescan.hip.h"

#pragma clang fp contract(off)

namespace vers {

constexpr int64_t kFlatPrescanDefault = 0;
constexpr int kFlpWaves = 4;      // waves of a block at most (fewer where the lists would not fit: flat_prescan_plan)
constexpr int kFlpCbStep = 2;     // column blocks of 16 per step of the load ring: 4 loads, 4 KiB per wave
constexpr int kFlpRing = 4;       // steps in flight: 16 KiB per wave
constexpr int kFlpTrPitch = 33;   // floats per row of a wave's transpose slice (32 queries + 1: conflict-free column reads)
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

// Accumulator layout (prescan.hip.h): lane l holds query column n = l & 31 of its set and rows 32 h + 8 (e >> 2) + 4 (l >> 5) + (e & 3) of the tile.
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
  const uint32_t nst = a.ld / (16u * kFlpCbStep), tile_bytes = a.ld * 128u;
  const uint32_t n_steps = my_tiles * nst;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.rows_h, 0, (int)(n_tiles * tile_bytes), 0x00020000);  // (< 4 GiB: flat_shadow_derive)
  const uint32_t lane_off = (uint32_t)lane * 16u;
  const int n = lane & 31, hf = lane >> 5;

  // per-lane query constants: the lane's column of each set
  bool live[SETS];
  uint32_t slot[SETS], thrb[SETS], pubb[SETS];
#pragma unroll
  for (int s = 0; s < SETS; ++s) {
    live[s] = (uint32_t)(s * 32 + n) < nq_live;
    slot[s] = live[s] ? q0 + (uint32_t)(s * 32 + n) : q0;  // (dead columns: the unconditional loads read query q0's word)
    thrb[s] = live[s] ? __hip_atomic_load(a.bounds32 + slot[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;  // order bits; a stale word only prunes less
    pubb[s] = thrb[s];
  }

  // the load ring: issued before the block stages, so that the first tiles fly meanwhile
  u32x4 buf[kFlpRing][2 * kFlpCbStep];
  float xn[kFlpRing];
  uint32_t gthr[kFlpRing][SETS];
  uint32_t ti = t0, ci = 0;  // (tile, step) the next issue fetches
  auto issue_next = [&](u32x4 (&r)[2 * kFlpCbStep], float& x, uint32_t (&g)[SETS]) __attribute__((always_inline)) {
    x = a.xnorm[(uint64_t)ti * kWave + (uint32_t)lane];
    // the shared thresholds are consumed once per tile, with the step that completes it; on the other steps every lane reads ONE word
#pragma unroll
    for (int s = 0; s < SETS; ++s) g[s] = __hip_atomic_load(a.bounds32 + (ci + 1 >= nst ? slot[s] : q0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t soff = ti * tile_bytes + ci * (kFlpCbStep * 2048u);
#pragma unroll
    for (int i = 0; i < 2 * kFlpCbStep; ++i) r[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane_off, soff + (uint32_t)i * 1024u, kPreAux);
    if (ci + 1 < nst) ++ci;
    else if (ti + W < t_end) { ci = 0; ti += W; }  // else: stay on the last step (a harmless re-read)
  };
  if (n_steps > 0) {
#pragma unroll
    for (int r = 0; r < kFlpRing - 1; ++r) issue_next(buf[r], xn[r], gthr[r]);
  }

  // stage the query block; every wave clears its own lists
  const float scale = a.metric ? -1.0f : -2.0f;  // (exact scalings)
  for (uint32_t i = threadIdx.x; i < q_entries; i += blockDim.x) {
    const uint32_t cb = i / (2u * NQ), oct = (i / NQ) & 1u, qs = i % NQ;
    f16x8_t hi, lo;
    if (qs < nq_live) {
      const f32x4* src = reinterpret_cast<const f32x4*>(a.qp + (uint64_t)(q0 + qs) * a.ld + cb * 16u + oct * 8u);
      const f32x4 v0 = src[0], v1 = src[1];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float y = scale * (j < 4 ? v0[j & 3] : v1[j & 3]);
        hi[j] = (_Float16)y;
        lo[j] = (_Float16)(y - (float)hi[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) hi[j] = lo[j] = (_Float16)0.0f;
    }
    qh[i] = hi;
    if (LO) qh[q_entries + i] = lo;
  }
  for (uint32_t i = (uint32_t)lane; i < (uint32_t)NQ * kp; i += kWave) lists[i] = kKeyMax;
  __syncthreads();

  uint64_t empty = ~0ull;            // wave-uniform: queries of the block whose list (this wave's) holds nothing yet
  uint32_t badmask[SETS];            // wave-uniform: queries with a non-finite val of a real row
  f32x16_t acc[SETS][2];
#pragma unroll
  for (int s = 0; s < SETS; ++s) {
    badmask[s] = 0u;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[s][0][e] = acc[s][1][e] = 0.0f;
  }

  // end of tile t: |x|^2 through the matrix core, the thresholds, the two-stage path to the lists
  auto tile_done = [&](uint32_t t, float xnv, const uint32_t (&g)[SETS]) __attribute__((always_inline)) {
    const float nrm = a.metric ? 0.0f : 1.0f;
#pragma unroll
    for (int s = 0; s < SETS; ++s) {
      acc[s][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(xnv, hf == 0 ? nrm : 0.0f, acc[s][0], 0, 0, 0);
      acc[s][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(xnv, hf == 1 ? nrm : 0.0f, acc[s][1], 0, 0, 0);
      if (live[s] && g[s] < thrb[s]) thrb[s] = g[s];
      if (g[s] < pubb[s]) pubb[s] = g[s];
    }
#pragma unroll
    for (int s = 0; s < SETS; ++s) {
      const float thrf = thrb[s] == 0xFFFFFFFFu ? __builtin_inff() : __uint_as_float(order_bits_to_f32_bits(thrb[s]));
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        bool any = false;
#pragma unroll
        for (int e = 0; e < 16; ++e) any |= (acc[s][h][e] <= thrf) || !(__builtin_fabsf(acc[s][h][e]) < __builtin_inff());
        if (__ballot(any && live[s]) != 0ull) {  // (wave-uniform) rare after the first tiles
          __builtin_amdgcn_wave_barrier();  // the slice's readers of the previous round are done
#pragma unroll
          for (int e = 0; e < 16; ++e) tr[(8 * (e >> 2) + 4 * hf + (e & 3)) * kFlpTrPitch + n] = acc[s][h][e];
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          const uint32_t row = t * kWave + 32u * (uint32_t)h + (uint32_t)lane;  // lanes 0 .. 31: a row of the half each
          const bool real = lane < 32 && row < a.n_rows;
          const uint32_t nq_set = nq_live > (uint32_t)(32 * s) ? (nq_live - 32u * s < 32u ? nq_live - 32u * s : 32u) : 0u;
          for (uint32_t c = 0; c < nq_set; ++c) {  // wave-uniform
            const float val = tr[(lane & 31) * kFlpTrPitch + c];
            const bool fin = __builtin_fabsf(val) < __builtin_inff();
            if (__ballot(real && !fin) != 0ull) badmask[s] |= 1u << c;
            const uint32_t tb = (uint32_t)__builtin_amdgcn_readlane((int)thrb[s], (int)c);
            const uint32_t vb = f32_to_order_bits(val);
            const bool pass = real && fin && vb <= tb;
            const uint64_t pm = __ballot(pass);
            if (pm != 0ull) {
              const uint32_t qi = 32u * s + c;
              uint64_t* const lq = lists + (size_t)qi * kp;
              const uint64_t cand = pass ? (((uint64_t)vb << 32) | row) : kKeyMax;
              uint64_t list;
              if (((empty >> qi) & 1ull) && __popcll(pm) > 8) {  // an empty list and many survivors: one sort instead of an ordered insert each
                list = cand;
                wave_rank_sort64<true>(list, lane);
              } else {
                list = (uint32_t)lane < kp ? lq[lane] : kKeyMax;
                wave_topk_update(list, kp, cand, kKeyMax);
              }
              if ((uint32_t)lane < kp) lq[lane] = list;
              empty &= ~(1ull << qi);
              const uint32_t nb = (uint32_t)(readlane64(list, (int)kp - 1) >> 32);  // 0xFFFFFFFF: the list is not full
              if (n == (int)c && nb < thrb[s]) thrb[s] = nb;
            }
          }
          // a list's kp-th val improved on what the query's other waves and segments know: tell them
          if (lane < 32 && live[s] && thrb[s] < pubb[s]) {
            atomicMin(a.bounds32 + slot[s], thrb[s]);
            pubb[s] = thrb[s];
          }
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[s][h][e] = 0.0f;
      }
    }
  };

  if (n_steps > 0) {
    const f16x8_t* const qhi = qh + (size_t)hf * NQ + n;
    const f16x8_t* const qlo = qhi + q_entries;
    uint32_t cc = 0, ct = t0;  // step and tile being consumed
    for (uint32_t s0 = 0; s0 < n_steps; s0 += kFlpRing) {
#pragma unroll
      for (int r = 0; r < kFlpRing; ++r) {
        constexpr int kR = kFlpRing;
        issue_next(buf[(r + kR - 1) % kR], xn[(r + kR - 1) % kR], gthr[(r + kR - 1) % kR]);
        if (s0 + r < n_steps) {  // wave-uniform
#pragma unroll
          for (int k = 0; k < kFlpCbStep; ++k) {
            const size_t e0 = (size_t)(cc * kFlpCbStep + k) * 2u * NQ;
#pragma unroll
            for (int s = 0; s < SETS; ++s) {
              const f16x8_t bh = qhi[e0 + 32 * s];
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                const f16x8_t ar = __builtin_bit_cast(f16x8_t, buf[r][2 * k + h]);
                if constexpr (LO) acc[s][h] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar, qlo[e0 + 32 * s], acc[s][h], 0, 0, 0);  // (small term first)
                acc[s][h] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar, bh, acc[s][h], 0, 0, 0);
              }
            }
          }
          if (++cc == nst) {
            cc = 0;
            tile_done(ct, xn[r], gthr[r]);
            ct += W;
          }
        }
      }
    }
  }

  // the segment's end: the waves' lists of a query folded into its slot; wave w takes queries w, w + W, ...
  if (lane < 32) {
#pragma unroll
    for (int s = 0; s < SETS; ++s)
      if (live[s] && ((badmask[s] >> n) & 1u)) a.qflags[slot[s]] = 1u;
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
