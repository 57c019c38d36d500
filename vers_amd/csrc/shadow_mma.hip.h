// shadow_mma.hip.h -- the pieces the matrix-core scans of the fp16 shadow are built from: range_prefilter_kernel (range_prescan.hip.h),
// filter_prescan_kernel (filter_prescan.hip.h) and flat_prescan_kernel (flat_prescan.hip.h).  Internal: device code only, nothing exported.
// (prescan_kernel_g, the headline list scan, is NOT built from these: its ring is TileLoader's and its candidates go through the shared buffer.)
//   THE LOAD RING (ShadowRing).  A wave streams 64-row tiles of the shadow (rows_to_f16_kernel's layout: a lane's 16-byte piece is already
//   the A operand of v_mfma_f32_32x32x16_f16).  A step = kShCbStep column blocks of 16 = 4 non-temporal 16-byte buffer loads per lane; the
//   loads run kShRing steps ahead in registers, across tile ends, every one unconditional: steps past the end re-read the last (scan_item
//   says why).  |x|^2 of the lane's row travels with the step, and so may words of the caller's (`extra`: the shared thresholds, read with
//   the step that completes a tile), so nothing is loaded outside the ring.  The walk takes every stride-th tile (the range filter: every
//   tile of the item; the flat scan: every W-th of the segment); what a step feeds (`mma`) and what ends a tile (`done`) are the caller's
//   closures -- __attribute__((always_inline)), item_loop.hip.h says why.  prime() and run() are separate calls: the flat kernel stages its
//   query block between them.  The filtered kernel walks the live bits of 64-tile windows and keeps this ring WRITTEN OUT: it spills 109
//   (QG 8) / 142 (QG 16) scalar registers as it is, and built from a ring struct with a live-bit walk it spilled 140 / 187, grew from
//   176 to 207 VGPRs and from 0 / 272 to 144 / 416 bytes of scratch a lane (profiles/r28_summary.txt).
//   THE QUERY BLOCK (shadow_split8, shadow_stage_queries).  The scaled query (-2 q, cosine: -q; exact scalings) as fp16 hi + lo, the B
//   operand in LDS: [hi | lo][column block of 16][octet][slot] x 16 bytes; entry (cb, octet, slot) holds columns 16 cb + 8 octet .. + 7 of
//   query `slot`.  (The range pre-filter keeps hi and lo side by side in ONE operand and stages in place, through shadow_split8.)
//   THE LIST OFFER (shadow_tile_norm, shadow_list_offer).  At a tile's end |x|^2 enters as one more k-step (v_mfma_f32_32x32x2_f32) into the
//   same accumulators -- the accumulation RescoreArgs::shadow is the audited error model of (pre_bound, prescan.hip.h) -- and the threshold
//   word that came with the step is taken in.  From the accumulators (lane l: query column l & 31, rows 32 h + 8 (e >> 2) + 4 (l >> 5) + (e & 3)) the path is
//   two-stage: a compare per register against the lane's own threshold and ONE ballot (after the first tiles nothing passes); only when
//   something passes or is not finite are the vals transposed through the wave's private LDS slice to row-per-lane and offered, per live
//   query, to its list of the kp smallest (val, row) keys, one key per lane (wave_topk_update; a rank sort into an empty list when many
//   pass).  The list's kp-th val is the query's threshold; an improvement on the shared word is published (atomicMin; stale = prunes less).
//   THE EXACT ROW CHAIN (tile_row_chain): the reference's ordered chain of one row of an f32 tile against a query, a row per lane.
#pragma once
#include "prescan.hip.h"

#pragma clang fp contract(off)

namespace vers {

constexpr int kShCbStep = 2;  // column blocks of 16 per step of the load ring: 4 loads, 4 KiB per wave
constexpr int kShRing = 4;    // steps in flight: 16 KiB per wave, across tile ends

// ---- the load ring ----------------------------------------------------------------------------------------------------------------------
// Tiles t0, t0 + stride, .. below t_end; tile t: its pieces at t * tile_bytes behind rsrc, |x|^2 of its rows at xnorm + 64 t; nst steps a tile.
// The caller's words are its own arrays: extra(slot, last step of its tile) loads them, done(tile, |x|^2, slot) reads them; mma(step, loads).
struct ShadowRing {
  __amdgpu_buffer_rsrc_t rsrc;
  const float* xnorm;
  uint32_t tile_bytes, nst, t0, t_end, stride;
  uint32_t ti = t0, ci = 0;  // (tile, step) the next issue fetches
  u32x4 buf[kShRing][2 * kShCbStep];  // (a ring is brace-initialised up to `stride`: these two start as zeros nobody reads -- issue()
  float xn[kShRing];                  // fills a slot before run() consumes it -- and the compiler drops the stores: r28_summary.txt, no scratch)

  template <class Extra>
  __device__ __forceinline__ void issue(int b, int lane, Extra&& extra) {
    xn[b] = xnorm[ti * kWave + (uint32_t)lane];  // 32-bit ON PURPOSE: rsrc bounds the stream below 4 GiB, so t_end * 64 rows fit; a caller beyond that needs another ring
    extra(b, ci + 1 >= nst);
    const uint32_t soff = ti * tile_bytes + ci * (kShCbStep * 2048u);
#pragma unroll
    for (int i = 0; i < 2 * kShCbStep; ++i) buf[b][i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (uint32_t)lane * 16u, soff + (uint32_t)i * 1024u, kPreAux);
    if (ci + 1 < nst) ++ci;
    else if (ti + stride < t_end) { ci = 0; ti += stride; }  // else: stay on the last step (a harmless re-read)
  }
  template <class Extra>
  __device__ __forceinline__ void prime(int lane, Extra&& extra) {  // kShRing - 1 steps ahead; the walk has a tile
#pragma unroll
    for (int b = 0; b < kShRing - 1; ++b) issue(b, lane, extra);
  }
  template <class Extra, class Mma, class Done>
  __device__ __forceinline__ void run(uint32_t n_steps, int lane, Extra&& extra, Mma&& mma, Done&& done) {  // n_steps = the walk's tiles x nst
    uint32_t tc = t0, cc = 0;  // (tile, step) being consumed
    for (uint32_t s0 = 0; s0 < n_steps; s0 += kShRing) {
#pragma unroll
      for (int b = 0; b < kShRing; ++b) {
        issue((b + kShRing - 1) % kShRing, lane, extra);
        if (s0 + b < n_steps) {  // wave-uniform
          mma(cc, buf[b]);
          if (++cc == nst) {
            cc = 0;
            done(tc, xn[b], b);
            tc += stride;
          }
        }
      }
    }
  }
};

// ---- the query block --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void shadow_split8(const float (&y)[8], f16x8_t& hi, f16x8_t& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    hi[j] = (_Float16)y[j];
    lo[j] = (_Float16)(y[j] - (float)hi[j]);
  }
}
// the block's threads stage NS slots: get(first column, slot, y) gives the 8 scaled elements of an entry (zeros for a slot without a query)
template <int NS, bool LO, class Get>
__device__ __forceinline__ void shadow_stage_queries(f16x8_t* qh, uint32_t n_cb, Get&& get) {
  const uint32_t entries = n_cb * 2u * NS;  // of the hi (and of the lo) part
  for (uint32_t i = threadIdx.x; i < entries; i += blockDim.x) {
    float y[8];
    get((i / (2u * NS)) * 16u + ((i / NS) & 1u) * 8u, i % NS, y);
    f16x8_t hi, lo;
    shadow_split8(y, hi, lo);
    qh[i] = hi;
    if (LO) qh[entries + i] = lo;
  }
}

// ---- the list offer ---------------------------------------------------------------------------------------------------------------------
struct ShadowList {       // of one set of query columns
  uint32_t thrb, pubb;    // per lane, of its column's query: order bits of the threshold | the smallest value seen in or sent to the shared word
  uint32_t empty, bad;    // wave-uniform, a bit per query: the list holds nothing yet | a non-finite val of a row that counts
};
// end of a tile, first part: |x|^2 (xs) of the lane's row into both row halves, the word g that travelled with the step into the thresholds
__device__ __forceinline__ void shadow_tile_norm(f32x16_t* acc, float xs, float nrm, int lane, bool live, uint32_t g, ShadowList& L) {
  acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(xs, lane < 32 ? nrm : 0.0f, acc[0], 0, 0, 0);
  acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(xs, lane < 32 ? 0.0f : nrm, acc[1], 0, 0, 0);
  if (live && g < L.thrb) L.thrb = g;
  if (g < L.pubb) L.pubb = g;
}
// end of tile t, second part.  COLS = 16: the operand's columns 16 .. 31 repeat 0 .. 15 and are ignored, both row halves go through the slice
// at once (64 rows x 17 floats); COLS = 32: a row half at a time (32 rows x 33 floats; lanes 0 .. 31 hold a row each).  live: the lane's column
// holds one of the nq live queries; word: that query's shared threshold.  Lists: row_ok(row), key_lo(query, row), load(query), store(query,
// list), kUnroll (lists in registers want constant indices: the query loop is unrolled that far; 1: a plain loop).  Clears the accumulators.
template <int COLS, class Lists>
__device__ __forceinline__ void shadow_list_offer(f32x16_t* acc, uint32_t t, int lane, bool live, uint32_t nq, uint32_t kp, float* tr, uint32_t* word,
                                                  ShadowList& L, Lists&& ls) {
  using LT = std::remove_reference_t<Lists>;
  constexpr int H = 32 / COLS, PITCH = COLS + 1;  // row halves per round | floats per row of the slice (+ 1: conflict-free column reads)
  const int n = lane & (COLS - 1), hf = lane >> 5;
  const bool incol = (lane & 31) < COLS;
  const float thrf = L.thrb == 0xFFFFFFFFu ? __builtin_inff() : __uint_as_float(order_bits_to_f32_bits(L.thrb));
#pragma unroll
  for (int h0 = 0; h0 < 2; h0 += H) {
    bool any = false;
#pragma unroll
    for (int i = 0; i < 16 * H; ++i) any |= (acc[h0 + i / 16][i % 16] <= thrf) || !(__builtin_fabsf(acc[h0 + i / 16][i % 16]) < __builtin_inff());
    if (__ballot(any && live && incol) != 0ull) {  // (wave-uniform) rare after the first tiles
      __builtin_amdgcn_wave_barrier();  // the slice's readers of the previous round are done
      if (incol) {
#pragma unroll
        for (int i = 0; i < 16 * H; ++i) tr[(32 * (i / 16) + 8 * ((i % 16) >> 2) + 4 * hf + (i & 3)) * PITCH + n] = acc[h0 + i / 16][i % 16];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const uint32_t row = t * kWave + 32u * (uint32_t)h0 + (uint32_t)lane;
      const bool ok = ls.row_ok(row);
      const int c_end = LT::kUnroll > 1 ? LT::kUnroll : (int)nq;
#pragma unroll LT::kUnroll
      for (int c = 0; c < c_end; ++c) {
        if (c < (int)nq) {  // wave-uniform
          const float val = tr[(lane & (32 * H - 1)) * PITCH + c];
          const bool fin = __builtin_fabsf(val) < __builtin_inff();
          if (__ballot(ok && !fin) != 0ull) L.bad |= 1u << c;
          const uint32_t tb = (uint32_t)__builtin_amdgcn_readlane((int)L.thrb, c);
          const uint32_t vb = f32_to_order_bits(val);
          const bool pass = ok && fin && vb <= tb;
          const uint64_t pm = __ballot(pass);
          if (pm != 0ull) {
            const uint64_t cand = pass ? (((uint64_t)vb << 32) | ls.key_lo(c, row)) : kKeyMax;
            uint64_t list;
            if (((L.empty >> c) & 1u) && __popcll(pm) > 8) {  // an empty list and many survivors: one sort instead of an ordered insert each
              list = cand;
              wave_rank_sort64<true>(list, lane);
            } else {
              list = ls.load(c);
              wave_topk_update(list, kp, cand, kKeyMax);
            }
            ls.store(c, list);
            L.empty &= ~(1u << c);
            const uint32_t nb = (uint32_t)(readlane64(list, (int)kp - 1) >> 32);  // 0xFFFFFFFF: the list is not full
            if (n == c && nb < L.thrb) L.thrb = nb;
          }
        }
      }
      // a list's kp-th val improved on what the shared word holds: tell the query's other lists
      if (lane < COLS && live && L.thrb < L.pubb) {
        atomicMin(word, L.thrb);
        L.pubb = L.thrb;
      }
    }
#pragma unroll
    for (int i = 0; i < 16 * H; ++i) acc[h0 + i / 16][i % 16] = 0.0f;
  }
}

// ---- the exact row chain ----------------------------------------------------------------------------------------------------------------
// the reference's ordered chain (scan.hip.h's arithmetic) of the lane's row of an f32 tile against q4p[0 .. ld / 4); xp: the row's first 4-column group, the groups lie 64 f32x4 apart
template <int METRIC>
__device__ __forceinline__ float tile_row_chain(const f32x4* xp, const f32x4* q4p, uint32_t ld) {
  float acc = 0.0f;
#pragma unroll 8
  for (uint32_t j = 0; j < ld / 4; ++j) {
    const f32x4 x4 = xp[(uint64_t)j * 64];
    const f32x4 q4 = q4p[j];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (METRIC == 0) {
        const float t = __fsub_rn(x4[u], q4[u]);
        acc = __fadd_rn(acc, __fmul_rn(t, t));
      } else {
        acc = __fadd_rn(acc, __fmul_rn(x4[u], q4[u]));
      }
    }
  }
  return METRIC == 0 ? acc : __fsub_rn(1.0f, acc);
}

}  // namespace vers
