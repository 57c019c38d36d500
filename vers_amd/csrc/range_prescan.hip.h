// range_prescan.hip.h -- the probed range search behind a matrix-core pre-filter on the fp16 shadow, with an exact finish.
//
// A range search's threshold is fixed before the scan starts: the query's radius does not move, no candidate list can overflow, so a
// filter over the shadow needs neither a threshold exchange nor a certificate that can fail.  Two passes replace the ordered-chain count
// pass of range.hip.h for a batch of two or more queries on a handle that holds a shadow, under option "range_prescan" = 1 (default 0):
//   (1) range_prefilter_kernel -- the items and the quad hand-out of range_scan_kernel (IvfSrc<QG>, QG 8 / 16).  Per (row, query)
//         val = |x|^2 - 2 <x~, q>   (cosine distance: -<x~, q>)
//       from v_mfma_f32_32x32x16_f16 over the shadow's row pieces and the block's query block in LDS: the B operand's columns 0..15 hold
//       the fp16 hi parts of the <= 16 scaled queries, columns 16..31 their lo parts, so ONE matrix instruction per row piece yields both
//       partial sums; they and |x|^2 are added on the VALU at the end of a tile.  A row with `val > cut[q]` is RULED OUT; every other row
//       of the segment is a candidate: one bit of the 64-bit word of (query, tile) in mask[mbase[pair] + tile of the list].  cand[slot] =
//       the candidates of the (pair, segment) slot.  One writer per word and per slot: plain stores, no atomics.
//   (2) range_exact_kernel<METRIC, FILL> -- waves stride over the slots; a wave takes the non-empty ones singly, walks the slot's mask
//       words in tile order (windows of 64 tiles) and deals the set bits out 64 per step, a candidate per lane: the reference's ordered
//       chain on the f32 tile (scan.hip.h's arithmetic, contraction off), `dist <= r` a plain f32 comparison.  FILL = false counts the
//       hits of the slot (counts[slot]; the NaN status bit as the chain pass sets it); FILL = true stores them at base[slot] + hits of
//       the slot's earlier candidates + hits in lower lanes: tile order, row order inside a tile -- the positions and the bytes of
//       range_item<.., FILL = true>.
// The candidates are a SUPERSET of the answer (range_cut, below), the finish is the reference's arithmetic: limits, ids and distance bits
// equal the chain path's.
//
// range_cut: the guarantee is  `val > cut` TRUE  =>  D_ref(row, q) > radius.
//   squared L2.  pre_bound(qn, xmax2, R2, d_pad, 0, 1) gives D_ref >= (val + offset) - of(val), of(val) = common + chain_k max(0, T),
//   T = val + offset + common.  For T > 0: D_ref >= T (1 - chain_k) - 2 common, which exceeds r when T > (r + 2 common) / (1 - chain_k).
//   For r + 2 common < 0 the division would move the threshold the wrong way for T <= 0 (there D_ref >= T - 2 common): the threshold on T
//   is then r + 2 common itself -- T above it gives T - 2 common > r for T <= 0 and T (1 - chain_k) - 2 common > -2 common > r for T > 0.
//       cut = [ (r + 2 c) / (1 - chain_k)  or  r + 2 c ] - offset - c,      c = common + extra
//   cosine distance.  D_ref >= val + 1 - global:  cut = r - 1 + global + extra.
//   extra: pre_bound's model sends hi, lo and |x|^2 through ONE matrix-core accumulator; here the hi and the lo sums are two accumulators
//   of d products each (no more roundings than the model's 2 d in one) and the VALU adds them and then |x|^2: two more roundings, of a sum
//   bounded by 2 |x~||q| <= S and of one bounded by 2 S, S = |q|^2 + max |x|^2 (+ 1): 3 u S, charged as 8 u S.  The cut grows with c, so
//   a row ruled out under c is ruled out under pre_bound's own `common` a fortiori (tests/cpp/range_cut_demo.cpp checks exactly that).
//   Evaluated in f64 (its own roundings: the 1e-12 term), rounded UP to f32.  A non-finite |q|^2, max |x|^2, R^2 or radius -- and a
//   query whose scaled elements overflow fp16 -- gives cut = +inf: `val > cut` is false for every val, every row stays a candidate.  A
//   NaN val makes the comparison false too: nothing is ruled out by a comparison a NaN can make true.
#pragma once
#include "ivf_src.hip.h"
#include "prescan.hip.h"
#include "range.hip.h"
#include "shadow_mma.hip.h"

#pragma clang fp contract(off)

namespace vers {

// ---- range_cut: host + device ---------------------------------------------------------------------------------------------------------
__host__ __device__ inline float range_round_up(double x) {  // the smallest f32 >= x, either sign (NaN / inf pass through)
  if (x >= 0.0) return prune_round_up(x);
  float f = (float)x;
  if ((double)f < x) f = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, f) - 1u);  // (negative: one step towards zero)
  return f;
}
__host__ __device__ inline float range_cut(double qn, double xmax2, double R2, float radius, uint32_t d_pad, int metric) {
  const double inf = __builtin_inf(), r = (double)radius;
  if (!(__builtin_fabs(qn) < inf) || !(__builtin_fabs(xmax2) < inf) || !(__builtin_fabs(R2) < inf) || !(__builtin_fabs(r) < inf)) return __builtin_inff();
  const PreBound pb = pre_bound(qn, xmax2, R2, d_pad, metric, 1);
  const double S = pb.offset + xmax2 + (metric ? 1.0 : 0.0);
  const double extra = 8.0 * 5.9604644775390625e-08 * S;
  double cut;
  if (metric) {
    cut = r - 1.0 + pb.global + extra;
  } else {
    const double c = pb.common + extra, num = r + 2.0 * c;
    cut = (num >= 0.0 ? num / (1.0 - pb.chain_k) : num) - pb.offset - c;
  }
  cut += 1e-12 * (__builtin_fabs(r) + S + pb.global + 1.0);
  const float f = range_round_up(cut);
  return f == f ? f : __builtin_inff();
}
// ---- the kernels' parameters ----------------------------------------------------------------------------------------------------------

struct RangePreParams {
  uint32_t ld;
  const uint16_t* rows_h;          // the fp16 shadow (rows_to_f16_kernel's layout)
  const float* xnorm;              // |x|^2 per storage row
  const float* cut;                // [b] range_cut per query
  const uint64_t* mbase;           // [b * P] first mask word of a pair: exclusive scan of the tiles of the pairs' lists
  uint64_t* mask;
  uint32_t* cand;                  // [slots] candidates per (pair, segment) slot (zeroed by the driver)
  uint32_t* next_quad;
  unsigned long long* wave_slots;  // [launched waves][2]: (query, row) pairs tested | candidates
};
struct RangeExactParams {
  const float* rows;
  uint32_t ld, ldq;
  const float* qp;                 // staged queries [b][ldq]
  const uint32_t *pj_list, *pj_pref, *list_off, *list_len;
  uint32_t P, S_max, seg_rows, seg_target;
  uint64_t n_slots;
  const uint64_t *mbase, *mask;
  const uint32_t* cand;
  unsigned long long* wave_slots;  // [launched waves]: exact hits (count pass)
};
// option "range_prescan": 0 -- measured: the filter leaves hardly more than the hits, but the finish's lane-per-candidate
// chains cost more than the chain passes they replace as soon as a query has ~100 results; count + fill won only at ~10 per query.
constexpr int64_t kRangePrescanDefault = 0;
inline size_t range_prefilter_lds_bytes(uint32_t ld) { return (size_t)(ld / 16u) * 1024u + 16u; }  // query block (hi | lo columns) + hand-out word
inline size_t range_exact_lds_bytes(uint32_t ld) { return (size_t)kWavesPerBlock * ((size_t)ld * sizeof(float) + kWave * (sizeof(uint32_t) + sizeof(uint64_t))); }
inline uint32_t range_prefilter_grid(int n_cu, uint32_t ld, uint32_t items) {  // 2 blocks per CU (176 .. 186 registers a wave: 32 KiB of loads in flight per SIMD), 1 where two query blocks exceed LDS
  const uint32_t by_lds = (uint32_t)((160u * 1024u) / range_prefilter_lds_bytes(ld));
  const uint32_t per_cu = by_lds < 1u ? 1u : (by_lds > 2u ? 2u : by_lds);
  const uint32_t quads = (items + 3u) / 4u;
  return std::max<uint32_t>(1u, std::min<uint32_t>(quads, (uint32_t)n_cu * per_cu));
}
inline uint32_t range_exact_grid(int n_cu, uint64_t n_slots) {
  const uint64_t blocks = (n_slots + (uint64_t)kWave * kWavesPerBlock - 1) / ((uint64_t)kWave * kWavesPerBlock);
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)n_cu * 4));
}

// the launches (range_prescan.hip: the translation unit that holds the kernels below)
int32_t launch_range_cut(const float* qp, uint32_t ldq, uint32_t ld, uint32_t b, const uint32_t* misc, const float* radius, int metric, float* cut, hipStream_t st);
int32_t launch_range_pair_tiles(const uint32_t* pj_list, const uint32_t* list_len, uint64_t n_pairs, uint32_t* tiles, hipStream_t st);
int32_t launch_range_prefilter(int metric, const IvfSrc<8>& src, const RangePreParams& p, uint32_t blocks, hipStream_t st);
int32_t launch_range_prefilter(int metric, const IvfSrc<16>& src, const RangePreParams& p, uint32_t blocks, hipStream_t st);
int32_t launch_range_exact(int metric, bool fill, const RangeExactParams& e, const RangeParams& p, uint32_t blocks, hipStream_t st);
int32_t launch_range_stats_fold(const unsigned long long* pre_slots, uint32_t pre_waves, const unsigned long long* exact_slots, uint32_t exact_waves,
                                unsigned long long* total, hipStream_t st);

#ifdef VERS_RANGE_PRESCAN_KERNELS
// ---- cut[q] per call: a wave per query (prune_table_kernel's shape) -------------------------------------------------------------------
static __global__ __launch_bounds__(256) void range_cut_kernel(const float* qp, uint32_t ldq, uint32_t ld, uint32_t b, const uint32_t* misc, const float* radius,
                                                               int metric, float* cut) {
  const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (q >= b) return;  // (whole waves)
  const float* qrow = qp + (uint64_t)q * ldq;
  const float scale = metric ? -1.0f : -2.0f;
  float qn = 0.0f;
  bool ok = true;
  for (uint32_t s = 0; s < ld / 64u; ++s) {
    const float v = qrow[s * 64u + (uint32_t)lane];
    qn = __fadd_rn(qn, __fmul_rn(v, v));
    ok &= __builtin_fabsf((float)(_Float16)(scale * v)) < __builtin_inff();  // the staged hi part is finite (a NaN fails too)
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) qn += __shfl_xor(qn, off, kWave);
  const bool all_ok = __ballot(!ok) == 0;
  if (lane == 0)
    cut[q] = all_ok ? range_cut((double)qn, (double)__uint_as_float(misc[0]), (double)__uint_as_float(misc[2]), radius[q], ld, metric) : __builtin_inff();
}

// tiles[i] = 64-row tiles of the list of pair i (0: the pair is not scanned here); one zero entry behind: the scan's last entry is the total
static __global__ void range_pair_tiles_kernel(const uint32_t* pj_list, const uint32_t* list_len, uint64_t n_pairs, uint32_t* tiles) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n_pairs) return;
  const uint32_t L = i < n_pairs ? pj_list[i] : kNoList;
  tiles[i] = L == kNoList ? 0u : (list_len[L] + (uint32_t)kWave - 1u) / (uint32_t)kWave;
}

// ---- (1) the pre-filter -----------------------------------------------------------------------------------------------------------------
// One work item: a wave walks the 64-row tiles of its row segment through the load ring of shadow_mma.hip.h.  Per column block one
// ds_read_b128 of the B operand and two MFMAs into the two 16-register accumulators of the tile's row halves, so every LDS operand feeds both.
// Accumulator layout (prescan.hip.h): lane l holds query column n = l & 31 and rows 32 h + 8 (e >> 2) + 4 (l >> 5) + (e & 3) of the tile.
template <int QG, int METRIC, class Src>
__device__ __forceinline__ void range_prefilter_item(const Src& src, const RangePreParams& p, uint32_t it, const ItemView<QG>& v, int lane, const f16x8_t* qh,
                                                     unsigned long long& tested, unsigned long long& cands) {
  const uint32_t n_tiles = (v.nrows + kWave - 1) / kWave;
  const int qi = lane & 15, hf = lane >> 5;
  const bool qlive = qi < (int)v.nq;
  float cutv = __builtin_inff();
  uint64_t mword0 = 0, slot = 0;
  if (qlive) {
    const uint32_t pair = src.pair_of(it, qi);
    cutv = p.cut[pair / src.P];
    mword0 = p.mbase[pair] + (v.row0 >> 6);
    slot = src.range_slot(it, qi);
  }
  const uint32_t srow0 = src.storage_row(it);
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)(p.rows_h + (uint64_t)srow0 * p.ld), 0, (int)(n_tiles * kWave * p.ld * 2u), 0x00020000);
  ShadowRing ring{rsrc, p.xnorm + srow0, p.ld * 128u, p.ld / (16u * kShCbStep), 0u, n_tiles, 1u};  // every tile of the item
  auto extra = [](int, bool) __attribute__((always_inline)) {};  // (the radius does not move: no word travels with a step)
  ring.prime(lane, extra);
  f32x16_t acc[2];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[0][e] = acc[1][e] = 0.0f;
  uint32_t ccount = 0;  // lanes 0 .. 15: the query's candidates in the item so far

  // end of a tile: hi + lo (the lanes of column n and n + 16), + |x|^2, the comparison, the (query, tile) word
  auto tile_done = [&](uint32_t t, float xnv, int) __attribute__((always_inline)) {
    uint32_t w[2] = {0u, 0u};  // candidate bits of the lane's rows of each half: bit = row within the half
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int rr = 8 * (e >> 2) + (e & 3);  // the row within the half for lanes 0 .. 31; lanes 32 .. 63: + 4
        const float a = acc[h][e];
        float val = a + __uint_as_float(lane_xor_u32<16>(__float_as_uint(a), lane));
        if (METRIC == 0) {
          const float xa = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(xnv), 32 * h + rr));
          const float xb = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(xnv), 32 * h + rr + 4));
          val = val + (hf ? xb : xa);
        }
        const uint32_t row = t * kWave + 32u * h + (uint32_t)rr + 4u * (uint32_t)hf;
        const bool c = row < v.nrows && !(val > cutv);
        w[h] |= c ? 1u << (rr + 4 * hf) : 0u;
        acc[h][e] = 0.0f;
      }
    }
    w[0] |= lane_xor_u32<32>(w[0], lane);  // lanes l and l + 32 hold complementary rows
    w[1] |= lane_xor_u32<32>(w[1], lane);
    const uint64_t word = ((uint64_t)w[1] << 32) | w[0];
    if (lane < 16 && qlive) {
      p.mask[mword0 + t] = word;
      ccount += (uint32_t)__popcll(word);
    }
  };

  auto mma = [&](uint32_t cc, const u32x4 (&r)[2 * kShCbStep]) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < kShCbStep; ++k) {
      const f16x8_t bq = qh[(size_t)(cc * kShCbStep + k) * kWave + lane];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, r[2 * k]), bq, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, r[2 * k + 1]), bq, acc[1], 0, 0, 0);
    }
  };
  ring.run(n_tiles * ring.nst, lane, extra, mma, tile_done);
  if (lane < 16 && qlive) p.cand[slot] = ccount;  // (one item per slot: a plain store)
  tested += (unsigned long long)v.nrows * v.nq;
  cands += wave_sum_u32(lane < 16 && qlive ? ccount : 0u);
}

template <int QG, int METRIC, class Src>
__global__ __launch_bounds__(kWave * kWavesPerBlock) void range_prefilter_kernel(Src src, RangePreParams p) {
  static_assert(QG == 8 || QG == 16, "the query block holds 16 hi and 16 lo columns");
  static_assert(kWavesPerBlock == 4, "items are padded to quads");
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  extern __shared__ __attribute__((aligned(16))) unsigned char rp_lds[];
  // the query block as the B operand of v_mfma_f32_32x32x16_f16: [column block of 16][lane] x 16 bytes; lane (octet, n) holds columns
  // 16 cb + 8 octet .. + 7 of operand column n -- n < 16: the hi part of query n, n >= 16: the lo part of query n - 16 (QG 8: zero columns)
  f16x8_t* const qh = reinterpret_cast<f16x8_t*>(rp_lds);
  const uint32_t n_cb = p.ld / 16u;
  uint32_t* const nq_lds = reinterpret_cast<uint32_t*>(rp_lds + (size_t)n_cb * 1024u);
  const uint32_t n_quads = src.n_items() / 4;
  const float scale = METRIC ? -1.0f : -2.0f;  // (as the top-k scan stages its queries: exact scalings)
  unsigned long long tested = 0, cands = 0;  // wave-uniform
  for (uint32_t b0 = blockIdx.x;; b0 += gridDim.x) {
    uint32_t bi = b0;
    if (p.next_quad != nullptr) {
      if (threadIdx.x == 0) *nq_lds = atomicAdd(p.next_quad, 1u);
      __syncthreads();
      bi = *nq_lds;  // every wave reads it before the next write: two barriers follow below
    }
    if (bi >= n_quads) break;  // block-uniform
    const uint32_t it = bi * 4 + wid;
    ItemView<QG> v;
    src.get(it, v);  // v.qb / v.nq are the same for the four items of the quad
    __syncthreads();  // the previous quad's readers are done with the LDS block
    for (uint32_t i = threadIdx.x; i < n_cb * kWave; i += kWave * kWavesPerBlock) {
      const uint32_t cb = i >> 6, n = i & 31u, oct = (i >> 5) & 1u, q = n & 15u;
      float y[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] = q < (uint32_t)QG ? scale * v.qb[(size_t)(cb * 16u + oct * 8u + (uint32_t)j) * QG + q] : 0.0f;
      f16x8_t hi, lo;
      shadow_split8(y, hi, lo);
      qh[i] = n < 16u ? hi : lo;
    }
    __syncthreads();
    if (v.nrows == 0) continue;  // padding item (wave-uniform; barriers are outside)
    range_prefilter_item<QG, METRIC>(src, p, it, v, lane, qh, tested, cands);
  }
  if (lane == 0) {  // the wave's own slot (filter_stats_fold_kernel's scheme)
    unsigned long long* ws = p.wave_slots + (size_t)(blockIdx.x * kWavesPerBlock + wid) * 2;
    ws[0] = tested;
    ws[1] = cands;
  }
}

// ---- (2) the exact finish ---------------------------------------------------------------------------------------------------------------
// position of the k-th (0-based) set bit of m; k < popcount(m)
__device__ __forceinline__ uint32_t nth_set_bit64(uint64_t m, uint32_t k) {
  uint32_t w = (uint32_t)m, pos = 0;
  const uint32_t c0 = (uint32_t)__popc(w);
  if (k >= c0) { k -= c0; w = (uint32_t)(m >> 32); pos = 32; }
#pragma unroll
  for (int sh = 16; sh >= 1; sh >>= 1) {
    const uint32_t c = (uint32_t)__popc(w & ((1u << sh) - 1u));
    if (k >= c) { k -= c; w >>= sh; pos += sh; }
  }
  return pos;
}

template <int METRIC, bool FILL>
__global__ __launch_bounds__(kWave * kWavesPerBlock) void range_exact_kernel(RangeExactParams a, RangeParams p) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  extern __shared__ __attribute__((aligned(16))) unsigned char rx_lds[];
  // per wave, private: the query (wave-uniform operand of the chains) | the window's inclusive bit counts | its mask words
  float* const ql = reinterpret_cast<float*>(rx_lds) + (size_t)wid * a.ld;
  uint64_t* const wds = reinterpret_cast<uint64_t*>(rx_lds + (size_t)kWavesPerBlock * a.ld * sizeof(float)) + wid * kWave;
  uint32_t* const pre = reinterpret_cast<uint32_t*>(rx_lds + (size_t)kWavesPerBlock * (a.ld * sizeof(float) + kWave * sizeof(uint64_t))) + wid * kWave;
  const uint32_t n_waves = gridDim.x * kWavesPerBlock, wave = blockIdx.x * kWavesPerBlock + wid;
  const uint32_t* const sel = FILL ? p.counts : a.cand;  // FILL: the slots with a hit; count: the slots with a candidate
  uint32_t q_staged = 0xFFFFFFFFu;
  bool nan_seen = false;
  unsigned long long hits_all = 0;
  for (uint64_t s0 = (uint64_t)wave * kWave; s0 < a.n_slots; s0 += (uint64_t)n_waves * kWave) {
    const uint64_t sl = s0 + (uint64_t)lane;
    uint64_t live = __ballot(sl < a.n_slots && sel[sl] != 0u);
    while (live) {  // one non-empty slot at a time (everything below is wave-uniform up to the candidates)
      const uint64_t slot = s0 + (uint64_t)(__ffsll((unsigned long long)live) - 1);
      live &= live - 1;
      const uint32_t pair = (uint32_t)(slot / a.S_max), seg = (uint32_t)(slot % a.S_max), q = pair / a.P;
      const uint32_t L = a.pj_list[pair];
      if (L == kNoList) continue;
      const uint32_t len = a.list_len[L];
      const uint32_t sr = list_seg_rows(len, a.seg_rows, a.seg_target);
      const uint32_t r0 = seg * sr;
      if (r0 >= len) continue;
      const uint32_t nrows = len - r0 < sr ? len - r0 : sr;
      const uint32_t n_tiles = (nrows + kWave - 1) / kWave;
      const uint64_t* const mw = a.mask + a.mbase[pair] + (r0 >> 6);
      const uint32_t srow0 = a.list_off[L] + r0;
      const uint32_t seq0 = a.pj_pref[pair] + r0;
      const float rad = p.radius[q];
      const uint64_t base = FILL ? p.base[slot] : 0ull;
      if (q != q_staged) {
        __builtin_amdgcn_wave_barrier();
        for (uint32_t i = (uint32_t)lane; i < a.ld; i += kWave) ql[i] = a.qp[(uint64_t)q * a.ldq + i];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        q_staged = q;
      }
      const f32x4* const q4p = reinterpret_cast<const f32x4*>(ql);
      uint32_t hits = 0;
      for (uint32_t t0 = 0; t0 < n_tiles; t0 += kWave) {
        const uint64_t word = t0 + (uint32_t)lane < n_tiles ? mw[t0 + (uint32_t)lane] : 0ull;
        const uint32_t incl = wave_incl_u32((uint32_t)__popcll(word));
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
        __builtin_amdgcn_wave_barrier();
        wds[lane] = word;
        pre[lane] = incl;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (uint32_t c0 = 0; c0 < total; c0 += kWave) {  // 64 candidates per step, in walk order, one per lane
          const bool have = c0 + (uint32_t)lane < total;
          const uint32_t c = have ? c0 + (uint32_t)lane : total - 1u;
          uint32_t wi = 0;  // the first word whose inclusive count exceeds c
#pragma unroll
          for (uint32_t step = 32; step >= 1; step >>= 1)
            if (pre[wi + step - 1u] <= c) wi += step;
          const uint32_t bit = nth_set_bit64(wds[wi], c - (wi ? pre[wi - 1u] : 0u));
          const uint32_t row = (t0 + wi) * kWave + bit;  // within the segment
          const uint32_t srow = srow0 + row;
          const float dist = tile_row_chain<METRIC>(reinterpret_cast<const f32x4*>(a.rows + (uint64_t)(srow >> 6) * 64ull * a.ld) + (srow & 63u), q4p, a.ld);
          const bool hit = have && dist <= rad;
          const uint64_t m = __ballot(hit);
          if constexpr (!FILL) {
            nan_seen |= have && (dist != dist);
          } else if (hit) {
            const uint64_t pos = base + hits + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            p.out_ids[pos] = (uint64_t)p.row_ids[srow];
            if (p.out_keys != nullptr) p.out_keys[pos] = make_key(dist, seq0 + row);
            else p.out_dist[pos] = dist;
          }
          hits += (uint32_t)__popcll(m);
        }
      }
      if constexpr (!FILL) {
        if (lane == 0) p.counts[slot] = hits;  // (one wave per slot: a plain store)
        hits_all += hits;
      }
    }
  }
  if constexpr (!FILL) {
    if (__ballot(nan_seen) != 0 && lane == 0) atomicOr(p.status, 1u);
    if (lane == 0) a.wave_slots[wave] = hits_all;
  }
}

// behind the count pass, one block: the waves' slots into the handle's running totals -- calls | pairs tested | candidates | exact hits
static __global__ __launch_bounds__(256) void range_stats_fold_kernel(const unsigned long long* pre_slots, uint32_t pre_waves, const unsigned long long* exact_slots,
                                                                      uint32_t exact_waves, unsigned long long* total) {
  __shared__ unsigned long long sh[3][256];
  unsigned long long s[3] = {0ull, 0ull, 0ull};
  for (uint32_t i = threadIdx.x; i < pre_waves; i += 256) { s[0] += pre_slots[(size_t)i * 2]; s[1] += pre_slots[(size_t)i * 2 + 1]; }
  for (uint32_t i = threadIdx.x; i < exact_waves; i += 256) s[2] += exact_slots[i];
#pragma unroll
  for (int c = 0; c < 3; ++c) sh[c][threadIdx.x] = s[c];
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w)
#pragma unroll
      for (int c = 0; c < 3; ++c) sh[c][threadIdx.x] += sh[c][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x < 3) atomicAdd(total + 1 + threadIdx.x, sh[threadIdx.x][0]);
  else if (threadIdx.x == 3) atomicAdd(total, 1ull);
}
#endif  // VERS_RANGE_PRESCAN_KERNELS

}  // namespace vers
