// filter.hip.h -- filtered top-k search: the top_k nearest among the vec ids a bitmap allows, one bitmap per call or one per query.
//
// In the reference's terms an EXTENSION: `ids[c].retain(|v| A.contains(v))` for the duration of one call -- a VIRTUAL vers_ivf_remove_batch of
// every id outside A, the index itself untouched.  The result is, bit for bit, what the unfiltered call of the same mode returns on an index
// from which those ids were removed.  A filter per query has no semantics of its own: row q of such a call is, bit for bit, row q of the
// per-call filtered search made with bitmap filter_of[q].
//
// The device has no vec id -> storage row map and gets none.  One pass over row_ids instead (the walk of removal's marking pass,
// remove_scan_rows_kernel), by the mask kernel of the layout (filter_walk.hip.h says what the two layouts are and why):
//   filter_tile_mask_kernel   the caller's bitmap over VEC IDS becomes one u64 per 64-row STORAGE TILE
//   filter_multi_mask_kernel  the caller's bitmaps become row_sets and tile_sets
// and filter_scan_kernel<QG, METRIC, Src, Mask>: scan_kernel's walk (scan.hip.h: the same items, quads sharing one LDS query block, the
// register prefetch ring over (tile, chunk) steps, the ordered f32 chain, wave_topk_fill / _update, `bounds`, `lower`) over the LIVE tiles of
// each item only (filter_walk.hip.h).  An item without a live tile leaves its slots at kKeyMax (the fill the plan / the driver gave them).
// Sequence numbers stay those of the unfiltered walk (seq_base + row; vec ids for SegSrc), so ivf_merge_kernel and seg_merge_kernel finish
// the call as they are: they count the keys they find and map a sequence number to a vec id whatever was skipped.  A NaN distance counts
// for valid (row, query) pairs only.
#pragma once
#include "filter_walk.hip.h"
#include "item_loop.hip.h"

#pragma clang fp contract(off)

namespace vers {

constexpr int kFltMaskThreads = 1024;  // (few, fat blocks: the allowed-row count is one atomic per block on one word, 13 ns each)
// One wave per storage tile, one ballot per tile.  Ids at or beyond n_bits are not allowed; bits of the bitmap's last word at or beyond
// n_bits are never read as allowed for the same reason.  Ids that were removed own no storage row (0xFFFFFFFF marks slack and freed rows).
static __global__ __launch_bounds__(kFltMaskThreads) void filter_tile_mask_kernel(const uint32_t* row_ids, uint64_t cap_rows, const uint64_t* bits, uint64_t n_bits,
                                                                      uint64_t* tile_mask, unsigned long long* stats) {
  const int lane = threadIdx.x & 63;
  const uint64_t n_tiles = (cap_rows + kWave - 1) / kWave;
  const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x / kWave);
  uint32_t allowed = 0;
  for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x >> 6); t < n_tiles; t += n_waves) {
    const uint64_t r = t * kWave + lane;
    const uint32_t id = r < cap_rows ? row_ids[r] : 0xFFFFFFFFu;
    const bool ok = id != 0xFFFFFFFFu && (uint64_t)id < n_bits && ((bits[id >> 6] >> (id & 63)) & 1ull);
    const uint64_t m = __ballot(ok);
    if (lane == 0) tile_mask[t] = m;
    allowed += (uint32_t)__popcll(m);
  }
  // one atomic per block: every wave adding its own count to the one word was 0.1 ms at a million rows (measured), 2048 blocks 31 us
  __shared__ uint32_t s_allowed;
  if (threadIdx.x == 0) s_allowed = 0u;
  __syncthreads();
  if (lane == 0 && allowed) atomicAdd(&s_allowed, allowed);
  __syncthreads();
  if (threadIdx.x == 0 && s_allowed) atomicAdd(stats + kFltRowsAllowed, (unsigned long long)s_allowed);
}

// One wave per storage tile.  `filters`: n_filters bitmaps, bitmap f at filters + f * stride_words; n_bits serves them all, with
// filter_tile_mask_kernel's meaning.  row_sets is written for every row of every tile (rows at or beyond cap_rows: 0).  The allowed (bitmap,
// row) pairs are counted by filter_tile_mask_kernel's scheme: one atomic per block.
static __global__ __launch_bounds__(kFltMaskThreads) void filter_multi_mask_kernel(const uint32_t* row_ids, uint64_t cap_rows, const uint64_t* filters,
                                                                                   uint64_t stride_words, uint32_t n_filters, uint64_t n_bits, uint64_t* row_sets,
                                                                                   uint64_t* tile_sets, unsigned long long* stats) {
  const int lane = threadIdx.x & 63;
  const uint64_t n_tiles = (cap_rows + kWave - 1) / kWave;
  const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x / kWave);
  uint32_t allowed = 0;
  for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x >> 6); t < n_tiles; t += n_waves) {
    const uint64_t r = t * kWave + lane;
    const uint32_t id = r < cap_rows ? row_ids[r] : 0xFFFFFFFFu;
    const bool in = id != 0xFFFFFFFFu && (uint64_t)id < n_bits;
    const uint64_t* w = filters + (in ? (id >> 6) : 0u);
    uint64_t rs = 0ull, ts = 0ull;
    for (uint32_t f = 0; f < n_filters; ++f) {
      const bool ok = in && ((w[(uint64_t)f * stride_words] >> (id & 63)) & 1ull);
      if (ok) rs |= 1ull << f;
      if (__ballot(ok) != 0ull) ts |= 1ull << f;
    }
    row_sets[r] = rs;
    if (lane == 0) tile_sets[t] = ts;
    allowed += (uint32_t)__popcll(rs);
  }
  for (int s = 32; s >= 1; s >>= 1) allowed += __shfl_xor(allowed, s);
  __shared__ uint32_t s_allowed;
  if (threadIdx.x == 0) s_allowed = 0u;
  __syncthreads();
  if (lane == 0 && allowed) atomicAdd(&s_allowed, allowed);
  __syncthreads();
  if (threadIdx.x == 0 && s_allowed) atomicAdd(stats + kFltRowsAllowed, (unsigned long long)s_allowed);
}

// Behind the call's last launch, one block: the waves' slots summed into the call's counters, and those into the handle's running totals.
constexpr int kFltFoldThreads = 256;
static __global__ __launch_bounds__(kFltFoldThreads) void filter_stats_fold_kernel(const unsigned long long* wave_slots, uint32_t n_waves, unsigned long long* last,
                                                                                   unsigned long long* total) {
  __shared__ unsigned long long sh[3][kFltFoldThreads];
  unsigned long long a[3] = {0ull, 0ull, 0ull};
  for (uint32_t i = threadIdx.x; i < n_waves; i += kFltFoldThreads)
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] += wave_slots[(size_t)i * 4 + c];
#pragma unroll
  for (int c = 0; c < 3; ++c) sh[c][threadIdx.x] = a[c];
  __syncthreads();
  for (int s = kFltFoldThreads / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s)
#pragma unroll
      for (int c = 0; c < 3; ++c) sh[c][threadIdx.x] += sh[c][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x < 3) {
    last[threadIdx.x] = sh[threadIdx.x][0];
    atomicAdd(total + threadIdx.x, sh[threadIdx.x][0]);
  } else if (threadIdx.x == kFltRowsAllowed) {
    atomicAdd(total + kFltRowsAllowed, last[kFltRowsAllowed]);  // (the mask kernel's count)
  }
}

// End of tile t of an item (on = false: the B half of an odd last pair, nothing to fold): its valid rows into the per-query lists, `acc`
// cleared for the next tile.  bound_of(qi): query qi's pruning bound, wave-uniform.  first: no tile of the item folded yet, the lists are empty.
template <int QG, int NP, int METRIC, class Src, class Mask, class BoundOf>
__device__ __forceinline__ void filter_topk_fold(const Src& src, const ScanParams& p, const Mask& m, uint32_t it, const ItemView<QG>& v, int lane,
                                                 f32x2 (&acc)[(QG + 1) / 2], uint32_t t, bool on, typename Mask::Aux aux, uint64_t (&list)[QG], BoundOf&& bound_of,
                                                 uint32_t vseq, uint64_t vlower, bool& first, bool& nan_seen) {
  const uint32_t row = t * kWave + lane;
  const typename Mask::Row r = m.row(on && row < v.nrows, t, lane, aux);
  uint32_t sid = 0;
  if constexpr (Src::kSeqIds) {
    // The sequence number is the vec id: loaded only for tiles in which some valid row can still enter a list (its distance bits at or
    // below the list's k-th) -- behind the wave-uniform ballot, so that most tiles issue no memory operation between two steps.
    bool ask = false;
#pragma unroll
    for (int qi = 0; qi < QG; ++qi)
      if (qi < 2 * NP && qi < (int)v.nq) {
        const float a = acc[qi >> 1][qi & 1];
        const float dist = METRIC == 0 ? a : __fsub_rn(1.0f, a);
        ask |= m.valid(r, qi) && f32_to_order_bits(dist) <= (uint32_t)(readlane64(list[qi], (int)p.k - 1) >> 32);
      }
    if (__ballot(ask) != 0) sid = m.any_query(r) ? src.seq_ids(it)[row] : 0u;
  }
#pragma unroll
  for (int qi = 0; qi < QG; ++qi) {
    if (on && qi < 2 * NP && qi < (int)v.nq) {
      const bool valid = m.valid(r, qi);  // (a valid row holds a vector: its id is not 0xFFFFFFFF)
      const float a = acc[qi >> 1][qi & 1];
      const float dist = METRIC == 0 ? a : __fsub_rn(1.0f, a);
      nan_seen |= valid && (dist != dist);
      const uint32_t seq = Src::kSeqIds ? sid : (uint32_t)__builtin_amdgcn_readlane((int)vseq, qi) + row;
      uint64_t cand = valid ? make_key(dist, seq) : kKeyMax;
      if (p.lower != nullptr && cand <= readlane64(vlower, qi)) cand = kKeyMax;  // ranked in an earlier pass
      const uint64_t bnd = bound_of(qi);
      if (first && p.k <= 16 && bnd == kKeyMax) wave_topk_fill(list[qi], p.k, cand, lane);
      else wave_topk_update(list[qi], p.k, cand, bnd);
    }
    acc[qi >> 1][qi & 1] = 0.0f;
  }
  first = false;
}

// One work item of a single query (the kernel instantiates QG == 1, NP == 1; the batched items are filter_item2's): scan_item with the tile
// walk restricted to the item's live tiles, one tile per step.
template <int QG, int NP, int METRIC, class Mask, class Src>
__device__ __forceinline__ void filter_item(const Src& src, const ScanParams& p, const typename Mask::Params& f, uint32_t it, const ItemView<QG>& v, int lane,
                                            bool& nan_seen, FilterCounts& fc) {
  const uint32_t n_tiles = (v.nrows + kWave - 1) / kWave;
  Mask m;
  m.template setup<QG>(f, src, it, src.storage_row(it), v.nq, n_tiles, lane);
  const uint64_t live = m.window(0, n_tiles, lane);
  if (n_tiles <= (uint32_t)kWave && live == 0ull) {  // nothing allowed in the item: not a byte of it is loaded, its slots stay kKeyMax (wave-uniform)
    fc.item(n_tiles, 0u);
    return;
  }
  uint64_t list[QG], bound[QG];
#pragma unroll
  for (int qi = 0; qi < QG; ++qi) {
    list[qi] = kKeyMax;
    bound[qi] = kKeyMax;
    if (p.bounds != nullptr && qi < 2 * NP && qi < (int)v.nq)  // relaxed agent-scope read: a stale value only prunes less
      bound[qi] = uniform64(__hip_atomic_load(p.bounds + src.bound_slot(it, qi), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  }
  uint64_t vlower = 0;  // lane qi: query qi's exclusive lower bound (0 = none: no key is 0)
  if (p.lower != nullptr && lane < QG && lane < (int)v.nq) vlower = p.lower[src.bound_slot(it, lane)];
  TileLoader L;
  L.init(v.rows, (uint64_t)n_tiles * kWave * p.ld * 4u, p.ld, lane);
  f32x2 acc[(QG + 1) / 2];
#pragma unroll
  for (int p2 = 0; p2 < (QG + 1) / 2; ++p2) acc[p2] = f32x2{0.0f, 0.0f};
  // per-query item constants once, lane qi = query qi, read back with v_readlane (scan_item)
  uint32_t vseq = 0;
  uint64_t vout = 0;
  if (lane < QG && lane < (int)v.nq) {
    vseq = Src::kSeqIds ? 0u : src.seq_base(it, lane);
    vout = (uint64_t)src.out(it, lane);
  }
  bool first = true;
  // The fold is filter_topk_fold's, written out in place with the wave-uniform bound[] read directly: through the shared function the
  // single-query kernels' instruction stream left the one they had (profiles/r26_summary.txt, section 0), and a single query is the
  // latency case -- 9 to 12 us a call.
  const uint32_t loaded = walk_live_tiles<QG, NP, METRIC, Src>(m, L, v.qb, n_tiles, p.n_chunks, live, lane, acc, [&](uint32_t t, typename Mask::Aux aux) __attribute__((always_inline)) {
    const uint32_t row = t * kWave + lane;
    const typename Mask::Row r = m.row(row < v.nrows, t, lane, aux);
    uint32_t sid = 0;
    if constexpr (Src::kSeqIds) {  // the vec id, only where a valid row can still enter a list (filter_topk_fold)
      bool ask = false;
#pragma unroll
      for (int qi = 0; qi < QG; ++qi)
        if (qi < 2 * NP && qi < (int)v.nq) {
          const float a = acc[qi >> 1][qi & 1];
          const float dist = METRIC == 0 ? a : __fsub_rn(1.0f, a);
          ask |= m.valid(r, qi) && f32_to_order_bits(dist) <= (uint32_t)(readlane64(list[qi], (int)p.k - 1) >> 32);
        }
      if (__ballot(ask) != 0) sid = m.any_query(r) ? src.seq_ids(it)[row] : 0u;
    }
#pragma unroll
    for (int qi = 0; qi < QG; ++qi) {
      if (qi < 2 * NP && qi < (int)v.nq) {
        const bool valid = m.valid(r, qi);
        const float a = acc[qi >> 1][qi & 1];
        const float dist = METRIC == 0 ? a : __fsub_rn(1.0f, a);
        nan_seen |= valid && (dist != dist);
        const uint32_t seq = Src::kSeqIds ? sid : (uint32_t)__builtin_amdgcn_readlane((int)vseq, qi) + row;
        uint64_t cand = valid ? make_key(dist, seq) : kKeyMax;
        if (p.lower != nullptr && cand <= readlane64(vlower, qi)) cand = kKeyMax;  // ranked in an earlier pass
        if (first && p.k <= 16 && bound[qi] == kKeyMax) wave_topk_fill(list[qi], p.k, cand, lane);
        else wave_topk_update(list[qi], p.k, cand, bound[qi]);
      }
      acc[qi >> 1][qi & 1] = 0.0f;
    }
    first = false;
  });
  if (!fc.item(n_tiles, loaded)) return;  // (an item of several windows without a live tile: slots stay kKeyMax)
#pragma unroll
  for (int qi = 0; qi < QG; ++qi) {
    if (qi < 2 * NP && qi < (int)v.nq) {
      if (lane < (int)p.k) reinterpret_cast<uint64_t*>(readlane64(vout, qi))[lane] = list[qi];
      if (p.bounds != nullptr) {  // publish this item's k-th key (if it has k) as a bound for later items
        const uint64_t kth = readlane64(list[qi], (int)p.k - 1);
        if (kth < bound[qi] && lane == 0) atomicMin((unsigned long long*)(p.bounds + src.bound_slot(it, qi)), (unsigned long long)kth);
      }
    }
  }
}

// One batched work item (QG > 1): scan_item2 with the tile walk restricted to the item's live tiles, two of them per step.  Same contract as
// filter_item.
template <int QG, int NP, int METRIC, class Mask, class Src>
__device__ __forceinline__ void filter_item2(const Src& src, const ScanParams& p, const typename Mask::Params& f, uint32_t it, const ItemView<QG>& v, int lane,
                                             bool& nan_seen, FilterCounts& fc) {
  const uint32_t n_tiles = (v.nrows + kWave - 1) / kWave;
  Mask m;
  m.template setup<QG>(f, src, it, src.storage_row(it), v.nq, n_tiles, lane);
  const uint64_t live = m.window(0, n_tiles, lane);
  if (n_tiles <= (uint32_t)kWave && live == 0ull) {  // nothing allowed in the item: not a byte of it is loaded, its slots stay kKeyMax (wave-uniform)
    fc.item(n_tiles, 0u);
    return;
  }
  uint64_t list[QG];
#pragma unroll
  for (int qi = 0; qi < QG; ++qi) list[qi] = kKeyMax;
  TileLoader L;
  L.init(v.rows, (uint64_t)n_tiles * kWave * p.ld * 4u, p.ld, lane);
  f32x2 accA[QG / 2], accB[QG / 2];
#pragma unroll
  for (int p2 = 0; p2 < QG / 2; ++p2) accA[p2] = accB[p2] = f32x2{0.0f, 0.0f};
  uint32_t vseq = 0;
  uint64_t vout = 0;
  uint64_t vbound = kKeyMax;  // shared pruning bound of query `lane`'s merge group (wave_topk_update)
  uint64_t vlower = 0;        // exclusive lower bound of query `lane` (multi-pass results, ScanParams::lower)
  uint64_t* bslot = nullptr;
  if (lane < QG && lane < (int)v.nq) {  // per-query constants once, lane qi = query qi (scan_item)
    vseq = Src::kSeqIds ? 0u : src.seq_base(it, lane);
    vout = (uint64_t)src.out(it, lane);
    if (p.lower != nullptr) vlower = p.lower[src.bound_slot(it, lane)];
    if (p.bounds != nullptr) {
      bslot = p.bounds + src.bound_slot(it, lane);
      vbound = __hip_atomic_load(bslot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // stale = prunes less, never wrong
    }
  }
  bool first = true;
  const uint32_t loaded = walk_live_pairs<QG, NP, METRIC, Src>(m, L, v.qb, n_tiles, p.n_chunks, live, lane, accA, accB,
                                                               [&](f32x2 (&acc)[QG / 2], uint32_t t, bool on, typename Mask::Aux aux) __attribute__((always_inline)) {
    filter_topk_fold<QG, NP, METRIC>(src, p, m, it, v, lane, acc, t, on, aux, list,
                                     [&](int qi) __attribute__((always_inline)) { return p.bounds != nullptr ? readlane64(vbound, qi) : kKeyMax; }, vseq, vlower, first, nan_seen);
  });
  if (!fc.item(n_tiles, loaded)) return;  // (an item of several windows without a live tile: slots stay kKeyMax)
  uint64_t kth = kKeyMax;  // lane qi collects query qi's k-th key
#pragma unroll
  for (int qi = 0; qi < QG; ++qi)
    if (qi < 2 * NP && qi < (int)v.nq) {
      if (lane < (int)p.k) reinterpret_cast<uint64_t*>(readlane64(vout, qi))[lane] = list[qi];
      const uint64_t kq = readlane64(list[qi], (int)p.k - 1);
      if (lane == qi) kth = kq;
    }
  // publish a full list's k-th key as a bound for the items of the same merge group that start later
  if (bslot != nullptr && kth < vbound) atomicMin((unsigned long long*)bslot, (unsigned long long)kth);
}

// Live query pairs of a batched top-k item: dead pairs are not computed, single-pair granularity (wave-uniform dispatch, as scan_kernel's)
template <int QG, int METRIC, class Mask, class Src>
__device__ __forceinline__ void filter_item2_by_pairs(const Src& src, const ScanParams& p, const typename Mask::Params& f, uint32_t it, const ItemView<QG>& v,
                                                      int lane, bool& nan_seen, FilterCounts& fc) {
  const uint32_t np = (v.nq + 1) >> 1;
  if constexpr (QG == 8) {
    switch (np) {
      case 1: filter_item2<8, 1, METRIC, Mask>(src, p, f, it, v, lane, nan_seen, fc); break;
      case 2: filter_item2<8, 2, METRIC, Mask>(src, p, f, it, v, lane, nan_seen, fc); break;
      case 3: filter_item2<8, 3, METRIC, Mask>(src, p, f, it, v, lane, nan_seen, fc); break;
      default: filter_item2<8, 4, METRIC, Mask>(src, p, f, it, v, lane, nan_seen, fc); break;
    }
  } else {
    switch (np) {
      case 1: filter_item2<16, 1, METRIC, Mask>(src, p, f, it, v, lane, nan_seen, fc); break;
      case 2: filter_item2<16, 2, METRIC, Mask>(src, p, f, it, v, lane, nan_seen, fc); break;
      case 3: filter_item2<16, 3, METRIC, Mask>(src, p, f, it, v, lane, nan_seen, fc); break;
      case 4: filter_item2<16, 4, METRIC, Mask>(src, p, f, it, v, lane, nan_seen, fc); break;
      case 5: filter_item2<16, 5, METRIC, Mask>(src, p, f, it, v, lane, nan_seen, fc); break;
      case 6: filter_item2<16, 6, METRIC, Mask>(src, p, f, it, v, lane, nan_seen, fc); break;
      case 7: filter_item2<16, 7, METRIC, Mask>(src, p, f, it, v, lane, nan_seen, fc); break;
      default: filter_item2<16, 8, METRIC, Mask>(src, p, f, it, v, lane, nan_seen, fc); break;
    }
  }
}

// QG == 1: filter_item; QG > 1: filter_item2.  The host launches no more waves than there are counter slots.
template <int QG, int METRIC, class Src, class Mask>
__global__ __launch_bounds__(kWave * kWavesPerBlock) void filter_scan_kernel(Src src, ScanParams p, typename Mask::Params f) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  bool nan_seen = false;
  FilterCounts fc;
  for_each_item<QG>(src, p.ld, p.next_quad, wid, [&](uint32_t it, const ItemView<QG>& v) __attribute__((always_inline)) {
    if constexpr (QG == 1) filter_item<1, 1, METRIC, Mask>(src, p, f, it, v, lane, nan_seen, fc);
    else filter_item2_by_pairs<QG, METRIC, Mask>(src, p, f, it, v, lane, nan_seen, fc);
  });
  if (__ballot(nan_seen) != 0 && lane == 0) atomicOr(p.status, 1u);
  FilterCounts::store(fc, f.wave_slots, wid, lane);
}

}  // namespace vers
