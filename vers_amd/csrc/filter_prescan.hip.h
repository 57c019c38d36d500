// filter_prescan.hip.h -- the probed filtered top-k search behind a matrix-core scan of the ALLOWED rows on the fp16 shadow, with the exact
// finish of the unfiltered search.  Option "filter_prescan" = 1 (default 0); one bitmap per call, QG 8 / 16, one pass (ivf_search.hip says when).
//
// A filter is a virtual removal, and ivf_rescore_kernel's certificate holds for ANY subset of the probed rows: the maxima it charges (max |x|^2,
// the shadow's measured residual) are taken over a superset.  So the scan below may leave out whatever the bitmap leaves out and the finish
// runs unchanged:
//   (1) filter_prescan_kernel<QG, METRIC, Src> -- filter_scan_kernel's items and quad hand-out (four waves, one LDS query block per quad,
//       the next_quad counter) and filter_item's walk over the LIVE tiles of an item (windows of 64 mask words, the ballot, an item without a
//       live tile returns before its first load).  Per live tile and (row, query)
//         val = |x|^2 - 2 <x~, q>   (cosine distance: -<x~, q>)
//       ACCUMULATED EXACTLY AS prescan_kernel_g<true, .., LO = true> DOES: per 16-byte row piece of the shadow (one non-temporal buffer load,
//       rows_to_f16_kernel's layout) the lo MFMA, then the hi MFMA, then at the tile's end |x|^2 as one more k-step
//       (v_mfma_f32_32x32x2_f32), all into ONE accumulator per row half.  RescoreArgs::shadow = 1 is therefore the audited error model as
//       it stands (pre_bound, prescan.hip.h): nothing is added to it.  The one difference is outside the model: |x|^2 of a DISALLOWED row
//       enters the k-step as 0 (its NaN would otherwise poison the allowed row 32 further through the 0 * NaN cross term).
//       The query block (shadow_mma.hip.h's planes) has 16 slots per octet (QG 8: eight of them zero); the MFMA's columns 16 .. 31 repeat
//       0 .. 15 and are ignored.  The load ring is shadow_mma.hip.h's, written out over the live tiles of a window.
//       A row is a candidate when its bit in the tile's mask word is set and val's order bits do not exceed the query's threshold: the
//       smallest known kp-th val of the merge group (bounds32: relaxed agent-scope load per tile, atomicMin when a list's kp-th improves; a
//       stale value only prunes less).  Keys are (order bits of val, seq_base + row): the unfiltered walk's sequence numbers.
//       SURVIVORS -> LISTS.  A wave keeps the kp smallest keys of each of its <= 16 queries in registers, one key per lane (filter_item2's
//       lists), and writes them at the item's end: exact per item, no lock, no shared buffer, no spin.  The two-stage path from the
//       accumulators to the lists is the list offer of shadow_mma.hip.h, through a private 4 KiB LDS slice.  The prescan's
//       append-and-compact buffer was the alternative: it serves eight waves that share a list across a quad; here a list belongs to one wave
//       and one short item, so its lock, its `done` counter and its overflow rounds would buy nothing, and per-item lists keep the slot
//       format and the certificate's "cut rows lie at or above the list's last val" argument per slot.
//       A non-finite val of an ALLOWED row sets the merge group's qflags word; a disallowed row's val is never looked at.
//   (2) ivf_rescore_kernel<kRescoreWaves>, launched unchanged on slots of kp keys per (pair, segment) and pj_nq = segments per pair.
//   (3) filter_fallback_kernel -- the queries the finish queued in fail_list, re-scanned over their probed lists' allowed rows with the
//       reference's ordered chain (tile_row_chain, shared with range_exact_kernel) and the chain path's keys: a block per queued query, a wave per live tile,
//       one list per wave, folded by wave 0.  Returns before its first store when nothing is queued.
#pragma once
#include "filter.hip.h"
#include "ivf_src.hip.h"
#include "prescan.hip.h"
#include "shadow_mma.hip.h"

#pragma clang fp contract(off)

namespace vers {

// option "filter_prescan": 0 -- measured
constexpr int64_t kFilterPrescanDefault = 0;
constexpr int kFpTrPitch = 17;  // floats per row of a wave's transpose slice (shadow_list_offer<16>: 16 queries + 1)
constexpr int kFpFbWaves = 4;
// slots of vers_ivf_filter_prescan_stats (u64 each) and, behind them, the finish's u32 count of failed certificates
constexpr int kFpCalls = 0, kFpFallback = 1, kFpStats = 2;

struct FilterPreParams {
  uint32_t ld, kp;
  const uint16_t* rows_h;          // the fp16 shadow
  const float* xnorm;              // |x|^2 per storage row
  const uint64_t* tile_mask;       // filter_tile_mask_kernel's words
  uint32_t* bounds32;              // per merge group: order bits of the smallest known kp-th val (0xFFFFFFFF: none yet)
  uint32_t* qflags;                // per merge group: != 0 -> a non-finite val of an allowed row
  uint32_t* next_quad;
  unsigned long long* wave_slots;  // [launched waves][4]: planned | loaded | skipped (filter_stats_fold_kernel)
};
struct FilterFbParams {
  const float* rows; uint32_t ld, ldq; const float* qp;
  const uint32_t *pj_list, *pj_pref, *list_off, *list_len, *row_ids;
  uint32_t P, top_k, b;
  const uint64_t* tile_mask;
  const uint32_t* fail_list;       // [b] queued queries, [b] their count
  uint32_t* status;
  uint64_t* out_ids; float* out_dist; uint32_t* out_count;
  unsigned long long* total;       // [kFpStats]
};
// query block (hi | lo) | the four waves' transpose slices | hand-out word
inline size_t filter_prescan_lds_bytes(uint32_t ld) { return (size_t)(ld / 16u) * 1024u + (size_t)kWavesPerBlock * kWave * kFpTrPitch * sizeof(float) + 16u; }
inline uint32_t filter_prescan_grid(int n_cu, uint32_t ld, uint32_t items, uint32_t cap_blocks) {  // 2 blocks per CU (<= 256 registers a wave), 1 where two query blocks exceed LDS
  const uint32_t by_lds = (uint32_t)((160u * 1024u) / filter_prescan_lds_bytes(ld));
  const uint32_t per_cu = by_lds < 1u ? 1u : (by_lds > 2u ? 2u : by_lds);
  return std::max<uint32_t>(1u, std::min<uint32_t>(std::min<uint32_t>((items + 3u) / 4u, (uint32_t)n_cu * per_cu), cap_blocks));
}

// the launches (filter_prescan.hip: the translation unit that holds the kernels below)
int32_t launch_filter_pre_begin(const uint32_t* pj_list, const uint32_t* list_len, uint64_t n_pairs, uint32_t seg_rows, uint32_t* pj_nq, unsigned long long* total, hipStream_t st);
int32_t launch_filter_prescan(int metric, const IvfSrc<8>& src, const FilterPreParams& p, uint32_t blocks, hipStream_t st);
int32_t launch_filter_prescan(int metric, const IvfSrc<16>& src, const FilterPreParams& p, uint32_t blocks, hipStream_t st);
int32_t launch_filter_fallback(int metric, const FilterFbParams& a, uint32_t blocks, hipStream_t st);

#ifdef VERS_FILTER_PRESCAN_KERNELS
// pj_nq[i] = the (pair, segment) slots of pair i: the segments of its list (0: not scanned here); thread 0 counts the call
static __global__ void filter_pre_begin_kernel(const uint32_t* pj_list, const uint32_t* list_len, uint64_t n_pairs, uint32_t seg_rows, uint32_t* pj_nq, unsigned long long* total) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) atomicAdd(total + kFpCalls, 1ull);
  if (i >= n_pairs) return;
  const uint32_t L = pj_list[i];
  pj_nq[i] = L == kNoList ? 0u : (list_len[L] + seg_rows - 1u) / seg_rows;
}

// ---- (1) the scan ---------------------------------------------------------------------------------------------------------------------
// shadow_list_offer's lists of a wave: a register per query (filter_item2's), the rows the tile's mask word allows, the walk's sequence numbers
template <int QG>
struct FilterPreLists {
  static constexpr int kUnroll = QG;
  uint64_t (&list)[QG];
  uint64_t mw;
  uint32_t nrows, vseq;  // vseq: lane q holds query q's sequence number of the item's first row
  int lane;
  __device__ __forceinline__ bool row_ok(uint32_t row) const { return ((mw >> lane) & 1ull) && row < nrows; }
  __device__ __forceinline__ uint32_t key_lo(int q, uint32_t row) const { return (uint32_t)__builtin_amdgcn_readlane((int)vseq, q) + row; }
  __device__ __forceinline__ uint64_t load(int q) const { return list[q]; }
  __device__ __forceinline__ void store(int q, uint64_t l) const { list[q] = l; }  // (q: a constant once unrolled)
};

template <int QG, int METRIC, class Src>
__device__ __forceinline__ void filter_prescan_item(const Src& src, const FilterPreParams& p, uint32_t it, const ItemView<QG>& v, int lane, const f16x8_t* qh,
                                                    float* tr, FilterCounts& fc) {
  const uint32_t n_tiles = (v.nrows + kWave - 1) / kWave;
  const uint32_t srow0 = src.storage_row(it);
  const uint64_t* words = p.tile_mask + (srow0 >> 6);
  uint64_t word = (uint32_t)lane < n_tiles ? words[lane] : 0ull;  // window 0's words: lane t holds tile t's
  uint64_t live = __ballot(word != 0ull);
  if (n_tiles <= (uint32_t)kWave && live == 0ull) {  // nothing allowed in the item: not a byte of it is loaded, its slots stay kKeyMax (wave-uniform)
    fc.planned += n_tiles;
    fc.skipped += 1u;
    return;
  }
  const int qi = lane & 15, hf = lane >> 5;
  const bool qlive = qi < (int)v.nq;
  // per-query constants, lane qi (and its three repeats) = query qi
  uint32_t vslot = 0, vseq = 0;
  uint64_t vout = 0;
  if (qlive) {
    const uint32_t pair = src.pair_of(it, qi);
    vslot = src.slot_of_pair(pair);
    vseq = src.pj_pref[pair] + v.row0;
    vout = (uint64_t)(src.partials + ((uint64_t)pair * src.S_max + src.items[it].seg) * src.k_keep);
  }
  const uint32_t slot0 = (uint32_t)__builtin_amdgcn_readlane((int)vslot, 0);  // (query 0 is live: the unconditional loads of dead lanes read its word)
  if (!qlive) vslot = slot0;
  const uint32_t thr0 = qlive ? __hip_atomic_load(p.bounds32 + vslot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;  // order bits; stale = prunes less
  ShadowList sl{thr0, thr0, 0xFFFFu, 0u};
  const uint32_t kp = p.kp;
  uint64_t list[QG];
#pragma unroll
  for (int q = 0; q < QG; ++q) list[q] = kKeyMax;

  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)(p.rows_h + (uint64_t)srow0 * p.ld), 0, (int)(n_tiles * kWave * p.ld * 2u), 0x00020000);
  const uint32_t lane_off = (uint32_t)lane * 16u, tile_bytes = p.ld * 128u;
  const float* xn_item = p.xnorm + srow0;
  const uint32_t nst = p.ld / (16u * kShCbStep);  // steps per tile (ld is a multiple of 64)
  const f16x8_t* const qhi = qh + (size_t)hf * 16 + qi;
  const f16x8_t* const qlo = qhi + (size_t)(p.ld / 16u) * 32;
  // shadow_mma.hip.h's ring, written out over the live bits of a window, the MFMA step in the loop: as closures of a shared ring they
  // cost this kernel scalar registers it does not have (said there)
  u32x4 buf[kShRing][2 * kShCbStep];
  float xn[kShRing];
  uint32_t gthr[kShRing];  // the merge group's shared threshold as it came with each step
  f32x16_t acc[2];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[0][e] = acc[1][e] = 0.0f;
  uint32_t loaded = 0;

  // end of tile t (of the item): the list offer of shadow_mma.hip.h on the wave's register lists
  auto tile_done = [&](uint32_t t, float xnv, uint32_t g) __attribute__((always_inline)) {
    const uint64_t mw = readlane64(word, (int)(t & 63u));
    const float xs = ((mw >> lane) & 1ull) ? xnv : 0.0f;  // (a disallowed row's |x|^2 is not looked at either)
    shadow_tile_norm(acc, xs, METRIC ? 0.0f : 1.0f, lane, qlive, g, sl);
    shadow_list_offer<16>(acc, t, lane, qlive, v.nq, kp, tr, p.bounds32 + vslot, sl, FilterPreLists<QG>{list, mw, v.nrows, vseq, lane});
  };

  for (uint32_t w0 = 0;; w0 += kWave) {
    if (live != 0ull) {
      const uint32_t n_live = (uint32_t)__popcll(live);
      loaded += n_live;
      const uint32_t n_steps = n_live * nst;
      uint64_t li = live, lc = live;  // live tiles not yet issued / not yet consumed, the current one included
      uint32_t ti = w0 + (uint32_t)__ffsll((unsigned long long)li) - 1u, ci = 0;  // (tile, step) the next issue fetches
      auto issue_next = [&](u32x4 (&r)[2 * kShCbStep], float& x, uint32_t& g) __attribute__((always_inline)) {
        x = xn_item[ti * kWave + (uint32_t)lane];
        // the shared threshold is consumed once per tile, with the step that completes it; on the others every lane reads ONE word (prescan_item_g)
        g = __hip_atomic_load(p.bounds32 + (ci + 1 >= nst ? vslot : slot0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t soff = ti * tile_bytes + ci * (kShCbStep * 2048u);
#pragma unroll
        for (int i = 0; i < 2 * kShCbStep; ++i) r[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane_off, soff + (uint32_t)i * 1024u, kPreAux);
        if (ci + 1 < nst) ++ci;
        else if (li & (li - 1)) { li &= li - 1; ci = 0; ti = w0 + (uint32_t)__ffsll((unsigned long long)li) - 1u; }  // else: stay on the last step (a harmless re-read)
      };
#pragma unroll
      for (int b = 0; b < kShRing - 1; ++b) issue_next(buf[b], xn[b], gthr[b]);
      uint32_t cc = 0;  // step being consumed
      for (uint32_t s0 = 0; s0 < n_steps; s0 += kShRing) {
#pragma unroll
        for (int b = 0; b < kShRing; ++b) {
          issue_next(buf[(b + kShRing - 1) % kShRing], xn[(b + kShRing - 1) % kShRing], gthr[(b + kShRing - 1) % kShRing]);
          if (s0 + b < n_steps) {  // uniform
#pragma unroll
            for (int k = 0; k < kShCbStep; ++k) {
              const f16x8_t bh = qhi[(size_t)(cc * kShCbStep + k) * 32];
              const f16x8_t bl = qlo[(size_t)(cc * kShCbStep + k) * 32];
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                const f16x8_t ar = __builtin_bit_cast(f16x8_t, buf[b][2 * k + h]);
                acc[h] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar, bl, acc[h], 0, 0, 0);  // (small term first: prescan_item_g's order)
                acc[h] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar, bh, acc[h], 0, 0, 0);
              }
            }
            if (++cc == nst) {
              cc = 0;
              tile_done(w0 + (uint32_t)__ffsll((unsigned long long)lc) - 1u, xn[b], gthr[b]);
              lc &= lc - 1;
            }
          }
        }
      }
    }
    if (w0 + kWave >= n_tiles) break;
    // the next window's words, between windows: the ring has drained
    word = w0 + kWave + (uint32_t)lane < n_tiles ? words[w0 + kWave + lane] : 0ull;
    live = __ballot(word != 0ull);
  }
  fc.planned += n_tiles;
  fc.loaded += loaded;
  if (loaded == 0) {  // (an item of several windows without a live tile: slots stay kKeyMax)
    fc.skipped += 1u;
    return;
  }
#pragma unroll
  for (int q = 0; q < QG; ++q)
    if (q < (int)v.nq && lane < (int)kp) reinterpret_cast<uint64_t*>(readlane64(vout, q))[lane] = list[q];  // ascending, kKeyMax padded
  if (lane < 16 && qlive && ((sl.bad >> lane) & 1u)) p.qflags[vslot] = 1u;
}

template <int QG, int METRIC, class Src>
__global__ __launch_bounds__(kWave * kWavesPerBlock) void filter_prescan_kernel(Src src, FilterPreParams p) {
  static_assert(QG == 8 || QG == 16, "the query block holds 16 slots per octet");
  static_assert(kWavesPerBlock == 4, "items are padded to quads");
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  extern __shared__ __attribute__((aligned(16))) unsigned char fp_lds[];
  // the query block as the B operand of v_mfma_f32_32x32x16_f16: [hi | lo][column block of 16][octet][16 slots] x 16 bytes; entry (cb, octet,
  // slot) holds columns 16 cb + 8 octet .. + 7 of query `slot`
  f16x8_t* const qh = reinterpret_cast<f16x8_t*>(fp_lds);
  const uint32_t n_cb = p.ld / 16u;
  float* const tr = reinterpret_cast<float*>(fp_lds + (size_t)n_cb * 1024u) + (size_t)wid * kWave * kFpTrPitch;
  uint32_t* const nq_lds = reinterpret_cast<uint32_t*>(fp_lds + (size_t)n_cb * 1024u + (size_t)kWavesPerBlock * kWave * kFpTrPitch * sizeof(float));
  const uint32_t n_quads = src.n_items() / 4;
  const float scale = METRIC ? -1.0f : -2.0f;  // (as the prescan stages its queries: exact scalings)
  FilterCounts fc;
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
    shadow_stage_queries<16, true>(qh, n_cb, [&](uint32_t c0, uint32_t q, float (&y)[8]) __attribute__((always_inline)) {
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] = q < (uint32_t)QG ? scale * v.qb[(size_t)(c0 + (uint32_t)j) * QG + q] : 0.0f;
    });
    __syncthreads();
    if (v.nrows == 0) continue;  // padding item (wave-uniform; barriers are outside)
    filter_prescan_item<QG, METRIC>(src, p, it, v, lane, qh, tr, fc);
  }
  if (lane < 3 && fc.planned != 0u)  // the wave's counters into its own slot (filter_scan_kernel's scheme)
    p.wave_slots[((size_t)blockIdx.x * kWavesPerBlock + wid) * 4 + lane] += (unsigned long long)(lane == kFltTilesPlanned ? fc.planned : lane == kFltTilesLoaded ? fc.loaded : fc.skipped);
}

// ---- (3) the filtered fallback ----------------------------------------------------------------------------------------------------------
template <int METRIC>
__global__ __launch_bounds__(kWave * kFpFbWaves) void filter_fallback_kernel(FilterFbParams a) {
  const uint32_t n_fail = a.fail_list[a.b];
  if (n_fail == 0) return;  // (before the first store)
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  extern __shared__ __attribute__((aligned(16))) unsigned char fb_lds[];
  float* const ql = reinterpret_cast<float*>(fb_lds);  // the query | the waves' lists
  uint64_t (*const sh)[kWave] = reinterpret_cast<uint64_t(*)[kWave]>(fb_lds + (size_t)a.ld * sizeof(float));
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(a.total + kFpFallback, (unsigned long long)n_fail);
  bool nan_seen = false;
  for (uint32_t i = blockIdx.x; i < n_fail; i += gridDim.x) {
    const uint32_t q = a.fail_list[i];
    __syncthreads();  // the previous query's readers are done
    for (uint32_t c = threadIdx.x; c < a.ld; c += blockDim.x) ql[c] = a.qp[(uint64_t)q * a.ldq + c];
    __syncthreads();
    const f32x4* const q4p = reinterpret_cast<const f32x4*>(ql);
    const uint32_t* const pl = a.pj_list + (uint64_t)q * a.P;
    const uint32_t* const pp = a.pj_pref + (uint64_t)q * a.P;
    uint64_t list = kKeyMax;
    for (uint32_t j = 0; j < a.P; ++j) {
      const uint32_t L = pl[j];
      if (L == kNoList) continue;
      const uint32_t len = a.list_len[L], srow0 = a.list_off[L], seq0 = pp[j];
      const uint32_t n_tiles = (len + kWave - 1) / kWave;
      for (uint32_t t = (uint32_t)wid; t < n_tiles; t += kFpFbWaves) {  // (wave-uniform)
        const uint64_t mw = a.tile_mask[(srow0 >> 6) + t];
        if (mw == 0ull) continue;
        const uint32_t row = t * kWave + (uint32_t)lane;
        const bool allowed = ((mw >> lane) & 1ull) && row < len;
        const float dist = tile_row_chain<METRIC>(reinterpret_cast<const f32x4*>(a.rows + (uint64_t)((srow0 >> 6) + t) * 64ull * a.ld) + lane, q4p, a.ld);
        nan_seen |= allowed && (dist != dist);
        wave_topk_update(list, a.top_k, allowed ? make_key(dist, seq0 + row) : kKeyMax, kKeyMax);
      }
    }
    sh[wid][lane] = (uint32_t)lane < a.top_k ? list : kKeyMax;
    __syncthreads();
    if (wid == 0) {
      for (int w = 1; w < kFpFbWaves; ++w) wave_topk_update(list, a.top_k, sh[w][lane], kKeyMax);
      const bool have = (uint32_t)lane < a.top_k && list != kKeyMax;
      uint32_t srow = 0;
      if (have) {  // the last scanned probe that starts at or before the sequence number (pj_pref ascends with the probe rank)
        const uint32_t seq = (uint32_t)list;
        for (uint32_t j = 0; j < a.P; ++j)
          if (pl[j] != kNoList && pp[j] <= seq) srow = a.list_off[pl[j]] + (seq - pp[j]);
        const uint64_t o = (uint64_t)q * a.top_k + (uint32_t)lane;
        a.out_ids[o] = a.row_ids[srow];
        a.out_dist[o] = __uint_as_float(order_bits_to_f32_bits((uint32_t)(list >> 32)));
      }
      const uint64_t hm = __ballot(have);
      if (lane == 0) a.out_count[q] = (uint32_t)__popcll(hm);
    }
  }
  if (__ballot(nan_seen) != 0 && lane == 0) atomicOr(a.status, 1u);
}
#endif  // VERS_FILTER_PRESCAN_KERNELS

}  // namespace vers
