// filter_range_multi.hip.h -- filtered range search with a filter PER QUERY: up to kFltMaxFilters bitmaps per call, query q uses bitmap
// filter_of[q].
//
// Semantics: none of its own.  Query q's CSR segment of a multi call is, bit for bit, query q's segment of the per-call filtered range search
// (filter_range.hip.h) made with bitmap filter_of[q]: the same virtual removal, query by query.
//
// filter_range.hip.h with the mask turned around, the way filter_multi.hip.h turned filter.hip.h's around: filter_multi_mask_kernel builds a
// word per ROW with a bit per BITMAP (row_sets) and a word per tile (tile_sets), once per call and before the count pass;
// filter_range_multi_scan_kernel is filter_range_scan_kernel's count / fill walk (the same items, the same slots, the same prefix between the
// passes, quads sharing one LDS query block, `next_quad`) over the tiles that are LIVE for the item: before the streaming loop lane qi loads
// filter_of of the item's query qi (an index at or beyond n_filters selects the empty filter and never reaches the masks), the OR of the live
// queries' bits is the item's filter set S, wave-uniform; lane t loads tile_sets of tile t and a tile is live when its word meets S.  The ring
// visits the set bits, one live tile per step, window by window of 64 tiles; the next window's words are loaded between windows.  A tile that
// no query of the item is allowed a row of is never loaded, in either pass; an item without a live tile returns before its first load, in both
// passes, and its count slots keep the driver's zero.  Every step of the ring also loads the lane's row_sets word of the step's tile (8 bytes,
// unconditional, issued with the step's row loads and counted with them: a load outside the ring would drain it at every tile boundary).
//
// ONE predicate for both passes, or the positions drift:   row < v.nrows  &&  bit filter_of[qi] of the lane's row_sets word  &&  dist <= r.
// Both passes read the same words: the call holds the index shared and the masks are built once.  A set bit implies that the row holds a
// vector, so the count pass loads no row id at all and the fill pass loads one only behind the wave-uniform "some lane hit" ballot.  A NaN
// distance is an error for a (query, row) pair that is valid for that query only, and in the count pass only.  Keys, ids and positions are
// filter_range_item's: base[slot] + hits of the item's earlier live tiles + hits in lower lanes; no atomics on the output.
//
// vers_ivf_filter_stats: planned / loaded tile visits and items skipped are counted in the COUNT pass only (FilterCounts, filter.hip.h).
//
// What the walk asks of a source: range.hip.h's contract (range_query, range_slot, storage_row, kRangeRows).
#pragma once
#include "filter_multi.hip.h"
#include "range.hip.h"

#pragma clang fp contract(off)

namespace vers {

// One work item, NP live query pairs (QG == 1: NP == 1; QG > 1: NP even, as range_item's).
template <int QG, int NP, int METRIC, bool FILL, class Src>
__device__ __forceinline__ void filter_range_multi_item(const Src& src, const RangeParams& p, const FilterMultiParams& f, uint32_t it, const ItemView<QG>& v,
                                                        int lane, bool& nan_seen, FilterCounts& fc) {
  constexpr bool kKeyId = Src::kRangeRows != kRangeRowsListed;  // the sort key's low word is the vec id itself
  const bool liveq = lane < QG && lane < (int)v.nq;
  const uint32_t n_tiles = (v.nrows + kWave - 1) / kWave;
  const uint32_t srow0 = src.storage_row(it);
  const uint64_t* words = f.tile_sets + (srow0 >> 6);
  uint32_t vrad = 0, vseq = 0, vhits = 0;  // lane qi = query qi; vhits: the query's hits in the item's live tiles so far
  uint64_t vslot = 0, vbase = 0;
  if (liveq) vslot = src.range_slot(it, lane);
  if constexpr (FILL) {
    const uint32_t had = liveq ? p.counts[vslot] : 0u;
    if (__ballot(had != 0u) == 0) return;  // no query of the item counted a hit: not a byte of it is loaded (range_item's rule, wave-uniform)
  }
  uint32_t vf;  // lane qi: query qi's bitmap (kFltNoFilter: none)
  const uint64_t S = item_filter_set<QG>(src, f, it, v.nq, lane, vf);
  // window 0's words: lane t holds tile t's (no load inside the streaming loop but the ring's own)
  uint64_t word = (uint32_t)lane < n_tiles ? words[lane] : 0ull;
  uint64_t live = __ballot((word & S) != 0ull);
  if (n_tiles <= (uint32_t)kWave && live == 0ull) {  // nothing allowed to any query of the item: not a byte of it is loaded, its count slots stay zero (wave-uniform)
    if constexpr (!FILL) {
      fc.planned += n_tiles;
      fc.skipped += 1u;
    }
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
  RowSetLoader R;
  R.init(f.row_sets + srow0, n_tiles, lane);
  f32x2 acc[(QG + 1) / 2];
#pragma unroll
  for (int p2 = 0; p2 < (QG + 1) / 2; ++p2) acc[p2] = f32x2{0.0f, 0.0f};
  uint32_t loaded = 0;

  // end of live tile t (of the item), rw: the lane's row_sets word of it; lane r holds row r's exact distance for each live query
  auto tile_done = [&](uint32_t t, u32x2 rw) {
    const uint32_t row = t * kWave + lane;
    const uint64_t rs = row < v.nrows ? row_set_word(rw) : 0ull;  // THE predicate's first term, for both passes
    // THE predicate's second term: (row, qi) is valid when bit filter_of[qi] of the lane's word is set (such a row holds a vector)
    auto valid_for = [&](int qi) -> bool {
      const uint32_t fq = (uint32_t)__builtin_amdgcn_readlane((int)vf, qi);
      return fq != kFltNoFilter && ((rs >> (fq & 63u)) & 1ull);
    };
    if constexpr (!FILL) {
#pragma unroll
      for (int qi = 0; qi < QG; ++qi) {
        if (qi < 2 * NP && qi < (int)v.nq) {
          const bool valid = valid_for(qi);
          const float a = acc[qi >> 1][qi & 1];
          const float dist = METRIC == 0 ? a : __fsub_rn(1.0f, a);
          nan_seen |= valid && (dist != dist);
          const float r = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)vrad, qi));
          const uint32_t n = (uint32_t)__popcll(__ballot(valid && dist <= r));
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
          any |= valid_for(qi) && dist <= __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)vrad, qi));
        }
      if (__ballot(any) != 0) {  // (wave-uniform; a tile without a hit issues no memory operation)
        uint32_t id32 = srow0 + row;  // (kRangeRowsFlat: the row number is the vec id)
        if constexpr (Src::kRangeRows != kRangeRowsFlat) id32 = (rs & S) != 0ull ? p.row_ids[srow0 + row] : 0xFFFFFFFFu;
        const uint64_t id = id32;
#pragma unroll
        for (int qi = 0; qi < QG; ++qi)
          if (qi < 2 * NP && qi < (int)v.nq) {
            const float a = acc[qi >> 1][qi & 1];
            const float dist = METRIC == 0 ? a : __fsub_rn(1.0f, a);
            const bool hit = valid_for(qi) && dist <= __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)vrad, qi));
            const uint64_t m = __ballot(hit);
            if (m) {
              const uint64_t pos = readlane64(vbase, qi) + (uint32_t)__builtin_amdgcn_readlane((int)vhits, qi) + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
              if (hit) {
                if (!kKeyId || p.out_keys == nullptr) p.out_ids[pos] = id;
                if (p.out_keys != nullptr) p.out_keys[pos] = make_key(dist, kKeyId ? id32 : (uint32_t)__builtin_amdgcn_readlane((int)vseq, qi) + row);
                else p.out_dist[pos] = dist;
              }
              if (lane == qi) vhits += (uint32_t)__popcll(m);
            }
          }
      }
#pragma unroll
      for (int p2 = 0; p2 < (QG + 1) / 2; ++p2) acc[p2] = f32x2{0.0f, 0.0f};
    }
  };

  // filter_multi_item's register ring over the (live tile, chunk) steps of one window of 64 tiles; every load unconditional (steps past the
  // end re-read the last chunk)
  constexpr int kBufs = QG == 1 ? 4 : 2;
  u32x4 buf[kBufs][kLoads];
  u32x2 rsw[kBufs];
  for (uint32_t w0 = 0;; w0 += kWave) {
    if (live != 0ull) {
      const uint32_t n_live = (uint32_t)__popcll(live);
      loaded += n_live;
      const uint32_t n_steps = n_live * p.n_chunks;
      uint64_t li = live, lc = live;  // live tiles not yet issued / not yet consumed, the current one included
      uint32_t ti = w0 + (uint32_t)__ffsll((unsigned long long)li) - 1u, ci = 0;  // (tile, chunk) the next issue fetches
      auto issue_next = [&](u32x4 (&r)[kLoads], u32x2& rw) {
        rw = R.issue(ti);
        L.template issue<tile_aux<Src::kStreamOnce>()>(r, ti, ci);
        if (ci + 1 < p.n_chunks) ++ci;
        else if (li & (li - 1)) { li &= li - 1; ci = 0; ti = w0 + (uint32_t)__ffsll((unsigned long long)li) - 1u; }  // else: stay on the last chunk
      };
#pragma unroll
      for (int b = 0; b < kBufs - 1; ++b) issue_next(buf[b], rsw[b]);
      uint32_t cc = 0;  // chunk being consumed
      for (uint32_t s0 = 0; s0 < n_steps; s0 += kBufs) {
#pragma unroll
        for (int b = 0; b < kBufs; ++b) {
          issue_next(buf[(b + kBufs - 1) % kBufs], rsw[(b + kBufs - 1) % kBufs]);
          if (s0 + b < n_steps) {  // uniform; no vector-memory op inside (FILL: behind tile_done's ballot)
            tile_chunk_compute<QG, NP, METRIC>(acc, buf[b], v.qb, cc);
            if (++cc == p.n_chunks) {
              cc = 0;
              tile_done(w0 + (uint32_t)__ffsll((unsigned long long)lc) - 1u, rsw[b]);
              lc &= lc - 1;
            }
          }
        }
      }
    }
    if (w0 + kWave >= n_tiles) break;
    // the next window's words, between windows: the ring has drained
    word = w0 + kWave + (uint32_t)lane < n_tiles ? words[w0 + kWave + lane] : 0ull;
    live = __ballot((word & S) != 0ull);
  }
  if constexpr (!FILL) {
    fc.planned += n_tiles;
    fc.loaded += loaded;
    if (loaded == 0) {  // (an item of several windows without a live tile: its count slots stay zero)
      fc.skipped += 1u;
      return;
    }
    if (liveq) p.counts[vslot] = vhits;  // (one item per slot: a plain store)
  }
}

// FILL = false: the count pass; FILL = true: the fill pass.  filter_range_scan_kernel's grid, hand-out and counters over the per-query items.
template <int QG, int METRIC, bool FILL, class Src>
__global__ __launch_bounds__(kWave * kWavesPerBlock) void filter_range_multi_scan_kernel(Src src, RangeParams p, FilterMultiParams f) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t n_items = src.n_items();
  bool nan_seen = false;
  FilterCounts fc;
  if constexpr (QG == 1) {
    const uint32_t n_waves = gridDim.x * kWavesPerBlock;
    for (uint32_t it = blockIdx.x * kWavesPerBlock + wid; it < n_items; it += n_waves) {
      ItemView<QG> v;
      src.get(it, v);
      if (v.nrows == 0) continue;
      filter_range_multi_item<1, 1, METRIC, FILL>(src, p, f, it, v, lane, nan_seen, fc);
    }
  } else {
    static_assert(QG == 8 || QG == 16, "query groups are 1, 8 or 16 wide");
    static_assert(QG == 8 || Src::kRangeRows == kRangeRowsListed, "segment sources group 8 queries");
    static_assert(kWavesPerBlock == 4, "items are padded to quads");
    extern __shared__ __attribute__((aligned(16))) float qlds[];
    const uint32_t n_quads = n_items / 4;
    const uint32_t n4 = p.ld * (QG / 4);  // float4s of one query block
    uint32_t* nq_lds = reinterpret_cast<uint32_t*>(qlds + (size_t)p.ld * QG);  // one word behind the query block
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
      const f32x4* g = reinterpret_cast<const f32x4*>(v.qb);
      for (uint32_t i = threadIdx.x; i < n4; i += kWave * kWavesPerBlock) reinterpret_cast<f32x4*>(qlds)[i] = g[i];
      __syncthreads();
      v.qb = qlds;
      if (v.nrows == 0) continue;  // padding item (wave-uniform; barriers are outside)
      const uint32_t np = ((v.nq + 3) >> 2) << 1;  // live query pairs, in steps of two
      if constexpr (QG == 8) {
        if (np <= 2) filter_range_multi_item<8, 2, METRIC, FILL>(src, p, f, it, v, lane, nan_seen, fc);
        else filter_range_multi_item<8, 4, METRIC, FILL>(src, p, f, it, v, lane, nan_seen, fc);
      } else {
        switch (np) {
          case 2: filter_range_multi_item<16, 2, METRIC, FILL>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 4: filter_range_multi_item<16, 4, METRIC, FILL>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 6: filter_range_multi_item<16, 6, METRIC, FILL>(src, p, f, it, v, lane, nan_seen, fc); break;
          default: filter_range_multi_item<16, 8, METRIC, FILL>(src, p, f, it, v, lane, nan_seen, fc); break;
        }
      }
    }
  }
  if constexpr (!FILL) {
    if (__ballot(nan_seen) != 0 && lane == 0) atomicOr(p.status, 1u);
    if (lane < 3 && fc.planned != 0u)  // the wave's counters into its own slot, once per call: the count pass alone feeds them
      f.wave_slots[((size_t)blockIdx.x * kWavesPerBlock + wid) * 4 + lane] += (unsigned long long)(lane == kFltTilesPlanned ? fc.planned : lane == kFltTilesLoaded ? fc.loaded : fc.skipped);
  }
}

}  // namespace vers
