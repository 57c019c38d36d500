// filter_range.hip.h -- filtered range search: every ALLOWED row within a radius, the allowed set a bitmap of vec ids per call or per query.
//
// The composition of range.hip.h and filter.hip.h: a VIRTUAL vers_ivf_remove_batch of every id outside the bitmap for the duration of one
// range call.  The result is, bit for bit, what the unfiltered range call of the same mode returns on an index from which those ids were
// removed.  A filter per query has no semantics of its own: query q's CSR segment of such a call is, bit for bit, query q's segment of the
// per-call filtered range search made with bitmap filter_of[q].
//
// The mask kernel of the layout (filter.hip.h) runs once per call and before the count pass; filter_range_scan_kernel<QG, METRIC, FILL, Src,
// Mask> is range_scan_kernel's count / fill walk (range.hip.h: the same items, the same slots, the same prefix between the passes, quads
// sharing one LDS query block, `next_quad`) over the LIVE tiles of each item only (filter_walk.hip.h), one live tile per step.  A tile that
// no query of the item is allowed a row of is never loaded, in either pass; an item without a live tile returns before its first load, in
// both passes, and its count slots keep the driver's zero.
//
// ONE predicate for both passes, or the positions drift:   row < v.nrows  &&  the mask allows (row, query)  &&  dist <= r.
// Both passes read the same words: the call holds the index shared and the masks are built once.  A set bit implies that the row holds a
// vector (the mask kernels never set one for 0xFFFFFFFF), so the count pass loads no row id at all -- not for kRangeRowsStored either --
// and the fill pass loads one only behind the wave-uniform "some lane hit" ballot, to obtain the id.  A NaN distance is an error for a valid
// (row, query) pair only, and in the count pass only; a row no query may see is not scanned.  Keys, ids and positions are range_item's:
// base[slot] + hits of the item's earlier live tiles + hits in lower lanes; no atomics on the output.
//
// vers_ivf_filter_stats: planned / loaded tile visits and items skipped are counted in the COUNT pass only (FilterCounts, filter_walk.hip.h)
// -- what the fill pass skips for lack of hits is range search's own saving, not the filter's.
//
// What the walk asks of a source: range.hip.h's contract (range_query, range_slot, storage_row, kRangeRows).
#pragma once
#include "filter.hip.h"
#include "range.hip.h"

#pragma clang fp contract(off)

namespace vers {

// One work item, NP live query pairs (QG == 1: NP == 1; QG > 1: NP even, as range_item's).
template <int QG, int NP, int METRIC, bool FILL, class Mask, class Src>
__device__ __forceinline__ void filter_range_item(const Src& src, const RangeParams& p, const typename Mask::Params& f, uint32_t it, const ItemView<QG>& v,
                                                  int lane, bool& nan_seen, FilterCounts& fc) {
  constexpr bool kKeyId = Src::kRangeRows != kRangeRowsListed;  // the sort key's low word is the vec id itself
  const bool liveq = lane < QG && lane < (int)v.nq;
  const uint32_t n_tiles = (v.nrows + kWave - 1) / kWave;
  const uint32_t srow0 = src.storage_row(it);
  uint32_t vrad = 0, vseq = 0, vhits = 0;  // lane qi = query qi; vhits: the query's hits in the item's live tiles so far
  uint64_t vslot = 0, vbase = 0;
  if (liveq) vslot = src.range_slot(it, lane);
  if constexpr (FILL) {
    const uint32_t had = liveq ? p.counts[vslot] : 0u;
    if (__ballot(had != 0u) == 0) return;  // no query of the item counted a hit: not a byte of it is loaded (range_item's rule, wave-uniform)
  }
  Mask m;
  m.template setup<QG>(f, src, it, srow0, v.nq, n_tiles, lane);
  const uint64_t live = m.window(0, n_tiles, lane);
  if (n_tiles <= (uint32_t)kWave && live == 0ull) {  // nothing allowed in the item: not a byte of it is loaded, its count slots stay zero (wave-uniform)
    if constexpr (!FILL) fc.item(n_tiles, 0u);
    return;
  }
  if (liveq) {
    vrad = __float_as_uint(p.radius[src.range_query(it, lane)]);
    if constexpr (FILL) {
      vbase = p.base[vslot];
      if (!kKeyId) vseq = src.seq_base(it, lane);
    }
  }
  TileLoader L;
  L.init(v.rows, (uint64_t)n_tiles * kWave * p.ld * 4u, p.ld, lane);
  f32x2 acc[(QG + 1) / 2];
#pragma unroll
  for (int p2 = 0; p2 < (QG + 1) / 2; ++p2) acc[p2] = f32x2{0.0f, 0.0f};

  // end of live tile t (of the item): lane r holds row r's exact distance for each live query
  const uint32_t loaded = walk_live_tiles<QG, NP, METRIC, Src>(m, L, v.qb, n_tiles, p.n_chunks, live, lane, acc, [&](uint32_t t, typename Mask::Aux aux) __attribute__((always_inline)) {
    const uint32_t row = t * kWave + lane;
    const typename Mask::Row r = m.row(row < v.nrows, t, lane, aux);  // THE predicate's first two terms are m.valid(r, qi), for both passes
    if constexpr (!FILL) {
#pragma unroll
      for (int qi = 0; qi < QG; ++qi) {
        if (qi < 2 * NP && qi < (int)v.nq) {
          const bool valid = m.valid(r, qi);
          const float a = acc[qi >> 1][qi & 1];
          const float dist = METRIC == 0 ? a : __fsub_rn(1.0f, a);
          nan_seen |= valid && (dist != dist);
          const float rad = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)vrad, qi));
          const uint32_t n = (uint32_t)__popcll(__ballot(valid && dist <= rad));
          if (lane == qi) vhits += n;
        }
        acc[qi >> 1][qi & 1] = 0.0f;
      }
    } else {
      bool any = false;
#pragma unroll
      for (int qi = 0; qi < QG; ++qi)
        if (qi < 2 * NP && qi < (int)v.nq) {
          const float a = acc[qi >> 1][qi & 1];
          const float dist = METRIC == 0 ? a : __fsub_rn(1.0f, a);
          any |= m.valid(r, qi) && dist <= __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)vrad, qi));
        }
      if (__ballot(any) != 0) {  // (wave-uniform; a tile without a hit issues no memory operation)
        uint32_t id32 = srow0 + row;  // (kRangeRowsFlat: the row number is the vec id)
        if constexpr (Src::kRangeRows != kRangeRowsFlat) id32 = m.any_query(r) ? p.row_ids[srow0 + row] : 0xFFFFFFFFu;
        const uint64_t id = id32;
#pragma unroll
        for (int qi = 0; qi < QG; ++qi)
          if (qi < 2 * NP && qi < (int)v.nq) {
            const float a = acc[qi >> 1][qi & 1];
            const float dist = METRIC == 0 ? a : __fsub_rn(1.0f, a);
            const bool hit = m.valid(r, qi) && dist <= __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)vrad, qi));
            const uint64_t hm = __ballot(hit);
            if (hm) {
              const uint64_t pos = readlane64(vbase, qi) + (uint32_t)__builtin_amdgcn_readlane((int)vhits, qi) + (uint32_t)__popcll(hm & ((1ull << lane) - 1ull));
              if (hit) {
                if (!kKeyId || p.out_keys == nullptr) p.out_ids[pos] = id;
                if (p.out_keys != nullptr) p.out_keys[pos] = make_key(dist, kKeyId ? id32 : (uint32_t)__builtin_amdgcn_readlane((int)vseq, qi) + row);
                else p.out_dist[pos] = dist;
              }
              if (lane == qi) vhits += (uint32_t)__popcll(hm);
            }
          }
      }
#pragma unroll
      for (int p2 = 0; p2 < (QG + 1) / 2; ++p2) acc[p2] = f32x2{0.0f, 0.0f};
    }
  });
  if constexpr (!FILL) {
    if (!fc.item(n_tiles, loaded)) return;  // (an item of several windows without a live tile: its count slots stay zero)
    if (liveq) p.counts[vslot] = vhits;    // (one item per slot: a plain store)
  }
}

// FILL = false: the count pass; FILL = true: the fill pass.  The count pass alone feeds the wave's filter counters and the status word.
template <int QG, int METRIC, bool FILL, class Src, class Mask>
__global__ __launch_bounds__(kWave * kWavesPerBlock) void filter_range_scan_kernel(Src src, RangeParams p, typename Mask::Params f) {
  static_assert(QG == 1 || QG == 8 || Src::kRangeRows == kRangeRowsListed, "segment sources group 8 queries");
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  bool nan_seen = false;
  FilterCounts fc;
  for_each_item<QG>(src, p.ld, p.next_quad, wid, [&](uint32_t it, const ItemView<QG>& v) __attribute__((always_inline)) {
    if constexpr (QG == 1) filter_range_item<1, 1, METRIC, FILL, Mask>(src, p, f, it, v, lane, nan_seen, fc);
    else with_pairs_by_two<QG>(v.nq, [&](auto np) __attribute__((always_inline)) { filter_range_item<QG, decltype(np)::value, METRIC, FILL, Mask>(src, p, f, it, v, lane, nan_seen, fc); });
  });
  if constexpr (!FILL) {
    if (__ballot(nan_seen) != 0 && lane == 0) atomicOr(p.status, 1u);
    FilterCounts::store(fc, f.wave_slots, wid, lane);
  }
}

}  // namespace vers
