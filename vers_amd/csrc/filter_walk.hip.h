// filter_walk.hip.h -- what the filtered list scans (filter.hip.h: top-k; filter_range.hip.h: range) share: the masks a call's bitmaps become,
// behind one policy type per layout, and the walk over an item's LIVE tiles, once per ring shape.
//
// A filtered item is scan_kernel's item (scan.hip.h) with the tile walk restricted to the tiles that hold an allowed row.  Lane t loads the
// mask word of tile t of the item; the ballot of "the word matters" is a wave-uniform 64-bit set and the step walk visits its set bits: a tile
// none of whose 64 rows is allowed is never loaded, an item without a live tile returns before its first load.  Items of more than 64 tiles
// go window by window; the next window's words are loaded between windows, when the ring has drained anyway.
//
// Two layouts answer "which rows may query qi of this item see":
//   MaskPerCall   ONE bitmap for the batch.  tile_mask: a u64 per 64-row storage tile, bit r = row 64 t + r holds an allowed vector.  A tile is
//                 live when its word is not 0; the words of a window stay in the lanes that loaded them and a tile's word comes back with
//                 v_readlane, so the ring carries nothing.
//   MaskPerQuery  a bitmap PER QUERY, query q uses bitmap filter_of[q] of up to kFltMaxFilters.  A mask word per (query of the group, tile)
//                 would cost 2 QG registers in a kernel that sits at 238 of 256 at QG = 16, so the mask is turned around -- a
//                 word per ROW, a bit per BITMAP -- and a wave carries one word per lane whatever QG is:
//                   row_sets[r]   bit f: storage row r holds a vector that bitmap f allows
//                   tile_sets[t]  bit f: some row of storage tile t is allowed by bitmap f
//                 Lane qi holds filter_of of the item's query qi (an index at or beyond n_filters selects the empty filter and never reaches
//                 the masks); the OR of the live queries' bits is the item's filter set S, wave-uniform, and a tile is live when its
//                 tile_sets word meets S.  Every step of the ring also loads the lane's row_sets word of the step's tile: 8 bytes,
//                 unconditional, issued with the step's row loads and counted with them -- a load outside the ring would drain it at every
//                 tile boundary (scan.hip.h).  A tile that is live for one query of a group only is loaded for the group; the other queries
//                 take no row from it.
// Both are rebuilt by every call (filter.hip.h's mask kernels) unless the call is a prepared one: no staleness protocol against add / remove /
// compact.  A set bit implies that the row holds a vector: the mask kernels never set one for a slack or freed row.
//
// What a policy answers, and nothing outside it knows how:
//   Params                         the struct the host fills and the kernel takes
//   setup<QG>(f, src, it, srow0, nq, n_tiles, lane)   the item's state, before its first window
//   window(w0, n_tiles, lane)      loads lane t's word of tile w0 + t; returns the live set of the window (wave-uniform)
//   Aux / issue(tile)              what rides the ring with a step's row loads: an empty type and no instruction for MaskPerCall
//   Row / row(in_range, t, lane, aux)   the lane's row of tile t at the end of the tile, in_range: the row exists (and the tile is folded)
//   valid(row, qi)                 THE predicate's mask term for one (row, query) pair: the fold asks nothing else about the filter
//   any_query(row)                 does some query of the item allow the row -- the lanes that load a row id behind a wave-uniform ballot
//
// What the walk asks of a source beyond scan_kernel's contract: storage_row(it); MaskPerQuery: range_query(it, qi), the batch's query behind
// slot qi of the item (both range.hip.h).
#pragma once
#include "scan.hip.h"

#pragma clang fp contract(off)

namespace vers {

// slots of vers_ivf_filter_stats
constexpr int kFltTilesPlanned = 0, kFltTilesLoaded = 1, kFltItemsSkipped = 2, kFltRowsAllowed = 3, kFltStats = 4;

constexpr uint32_t kFltMaxFilters = 64;        // (VERS_FILTER_MAX: a bit per bitmap in one u64)
constexpr uint32_t kFltNoFilter = 0xFFFFFFFFu;  // a query whose filter_of entry is out of range: the empty filter

typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

struct FilterParams {
  const uint64_t* tile_mask;       // [cap_rows / 64]: bit r of word t = storage row 64 t + r holds an allowed vector
  unsigned long long* stats;       // [kFltStats] of the call (zeroed by the driver)
  unsigned long long* wave_slots;  // [launched waves][4]: every wave's planned | loaded | skipped over the call's passes (zeroed by the driver)
};

struct FilterMultiParams {
  const uint64_t* row_sets;        // [n_tiles * 64]: bit f of word r = storage row r holds a vector bitmap f allows
  const uint64_t* tile_sets;       // [n_tiles]: bit f of word t = some row of storage tile t is allowed by bitmap f
  const uint32_t* filter_of;       // [b]: the bitmap of each query of the batch
  uint32_t n_filters;
  unsigned long long* stats;       // [kFltStats] of the call (FilterParams)
  unsigned long long* wave_slots;  // [launched waves][4] (FilterParams)
};

// A wave's share of the counters (wave-uniform): summed over its items in registers and added to the wave's OWN slot when it has run out of
// items, with plain stores; filter_stats_fold_kernel sums the slots behind the call's last launch.  Atomics on three shared words serialise
// in the L2 at 13 ns each: one per item was 40 us of a 130 us launch, and even one per wave -- the waves of a short launch finish together
// -- was 16 us of 93 (N = 1M, 64 queries) and 2 us of a single query's 12 (measured).
struct FilterCounts {
  uint32_t planned = 0, loaded = 0, skipped = 0;
  // one item of n_tiles tiles, n_loaded of them live; false: none was, the item is skipped and its slots keep the driver's fill
  __device__ __forceinline__ bool item(uint32_t n_tiles, uint32_t n_loaded) {
    planned += n_tiles;
    loaded += n_loaded;
    if (n_loaded == 0) skipped += 1u;
    return n_loaded != 0;
  }
  // the wave's counters into its own slot, once per launch (a call's passes run one after the other on the stream, and the host launches no
  // more waves than there are slots)
  // (fc by value: read through `this`, the choice of the counter became a switch where the kernels had two selects)
  static __device__ __forceinline__ void store(const FilterCounts fc, unsigned long long* wave_slots, int wid, int lane) {
    if (lane < 3 && fc.planned != 0u)
      wave_slots[((size_t)blockIdx.x * kWavesPerBlock + wid) * 4 + lane] += (unsigned long long)(lane == kFltTilesPlanned ? fc.planned : lane == kFltTilesLoaded ? fc.loaded : fc.skipped);
  }
};

struct MaskPerCall {
  using Params = FilterParams;
  struct Aux {};
  using Row = bool;
  const uint64_t* words;  // tile_mask of the item's first tile
  uint64_t word;          // lane t: the word of tile t of the current window

  template <int QG, class Src>
  __device__ __forceinline__ void setup(const Params& f, const Src&, uint32_t, uint32_t srow0, uint32_t, uint32_t, int) {
    words = f.tile_mask + (srow0 >> 6);
  }
  __device__ __forceinline__ uint64_t window(uint32_t w0, uint32_t n_tiles, int lane) {
    word = w0 + (uint32_t)lane < n_tiles ? words[w0 + lane] : 0ull;
    return __ballot(word != 0ull);
  }
  __device__ __forceinline__ Aux issue(uint32_t) const { return {}; }
  __device__ __forceinline__ Row row(bool in_range, uint32_t t, int lane, Aux) const { return in_range && ((readlane64(word, (int)(t & 63u)) >> lane) & 1ull); }
  __device__ __forceinline__ bool valid(Row r, int) const { return r; }
  __device__ __forceinline__ bool any_query(Row r) const { return r; }
};

struct MaskPerQuery {
  using Params = FilterMultiParams;
  using Aux = u32x2;     // the lane's row_sets word of a step's tile
  using Row = uint64_t;  // ... widened; 0 for a row that does not exist
  const uint64_t* words;  // tile_sets of the item's first tile
  uint64_t S;             // the item's filter set (wave-uniform)
  uint32_t vf;            // lane qi: query qi's bitmap (kFltNoFilter: none)
  // the row_sets words of the item: lane l of tile t reads word 64 t + l, through a buffer resource of its own (a step past the item's
  // rows reads 0, never memory)
  __amdgpu_buffer_rsrc_t rsrc;
  uint32_t lane_off;  // lane * 8 bytes

  template <int QG, class Src>
  __device__ __forceinline__ void setup(const Params& f, const Src& src, uint32_t it, uint32_t srow0, uint32_t nq, uint32_t n_tiles, int lane) {
    words = f.tile_sets + (srow0 >> 6);
    vf = kFltNoFilter;
    if (lane < QG && lane < (int)nq) {
      const uint32_t x = f.filter_of[src.range_query(it, lane)];
      vf = x < f.n_filters ? x : kFltNoFilter;
    }
    S = 0ull;
#pragma unroll
    for (int qi = 0; qi < QG; ++qi) {
      const uint32_t fq = (uint32_t)__builtin_amdgcn_readlane((int)vf, qi);
      if (fq != kFltNoFilter) S |= 1ull << (fq & 63u);
    }
    rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(f.row_sets + srow0), 0, (int)(n_tiles * (kWave * 8u)), 0x00020000);
    lane_off = (uint32_t)lane * 8u;
  }
  __device__ __forceinline__ uint64_t window(uint32_t w0, uint32_t n_tiles, int lane) const {
    const uint64_t word = w0 + (uint32_t)lane < n_tiles ? words[w0 + lane] : 0ull;
    return __ballot((word & S) != 0ull);
  }
  __device__ __forceinline__ Aux issue(uint32_t tile) const { return __builtin_amdgcn_raw_buffer_load_b64(rsrc, lane_off, tile * (kWave * 8u), 0); }
  __device__ __forceinline__ Row row(bool in_range, uint32_t, int, Aux w) const { return in_range ? ((uint64_t)w.y << 32) | (uint64_t)w.x : 0ull; }
  __device__ __forceinline__ bool valid(Row r, int qi) const {
    const uint32_t fq = (uint32_t)__builtin_amdgcn_readlane((int)vf, qi);
    return fq != kFltNoFilter && ((r >> (fq & 63u)) & 1ull);
  }
  __device__ __forceinline__ bool any_query(Row r) const { return (r & S) != 0ull; }
};

// The walk over the live tiles of an item, one tile per step: scan_item's register ring (4-deep for a single query, 2-deep otherwise) over
// the (live tile, chunk) steps of one window of 64 tiles after the other.  live: window 0's set (the caller has asked for it already, to leave
// an item without a live tile before any set-up).  tile_done(t, aux) at the end of tile t of the item, `acc` holding its rows' sums.  Every
// load of the ring is unconditional (steps past the end re-read the last chunk), and inside a step there is no vector-memory operation but
// what tile_done puts behind a wave-uniform ballot.  Returns the live tiles it loaded.
template <int QG, int NP, int METRIC, class Src, class Mask, class Done>
__device__ __forceinline__ uint32_t walk_live_tiles(Mask& m, const TileLoader& L, const float* qb, uint32_t n_tiles, uint32_t n_chunks, uint64_t live, int lane,
                                                    f32x2 (&acc)[(QG + 1) / 2], Done&& tile_done) {
  constexpr int kBufs = QG == 1 ? 4 : 2;
  u32x4 buf[kBufs][kLoads];
  typename Mask::Aux aux[kBufs];
  uint32_t loaded = 0;
  for (uint32_t w0 = 0;; w0 += kWave) {
    if (live != 0ull) {
      const uint32_t n_live = (uint32_t)__popcll(live);
      loaded += n_live;
      const uint32_t n_steps = n_live * n_chunks;
      uint64_t li = live, lc = live;  // live tiles not yet issued / not yet consumed, the current one included
      uint32_t ti = w0 + (uint32_t)__ffsll((unsigned long long)li) - 1u, ci = 0;  // (tile, chunk) the next issue fetches
      auto issue_next = [&](u32x4 (&r)[kLoads], typename Mask::Aux& a) __attribute__((always_inline)) {
        a = m.issue(ti);
        L.template issue<tile_aux<Src::kStreamOnce>()>(r, ti, ci);
        if (ci + 1 < n_chunks) ++ci;
        else if (li & (li - 1)) { li &= li - 1; ci = 0; ti = w0 + (uint32_t)__ffsll((unsigned long long)li) - 1u; }  // else: stay on the last chunk
      };
#pragma unroll
      for (int b = 0; b < kBufs - 1; ++b) issue_next(buf[b], aux[b]);
      uint32_t cc = 0;  // chunk being consumed
      for (uint32_t s0 = 0; s0 < n_steps; s0 += kBufs) {
#pragma unroll
        for (int b = 0; b < kBufs; ++b) {
          issue_next(buf[(b + kBufs - 1) % kBufs], aux[(b + kBufs - 1) % kBufs]);
          if (s0 + b < n_steps) {  // uniform
            tile_chunk_compute<QG, NP, METRIC>(acc, buf[b], qb, cc);
            if (++cc == n_chunks) {
              cc = 0;
              tile_done(w0 + (uint32_t)__ffsll((unsigned long long)lc) - 1u, aux[b]);
              lc &= lc - 1;
            }
          }
        }
      }
    }
    if (w0 + kWave >= n_tiles) break;
    live = m.window(w0 + kWave, n_tiles, lane);  // the next window's words, between windows: the ring has drained
  }
  return loaded;
}

// The same walk, two LIVE tiles per step through scan_item2's 2-deep ring: every query operand read from LDS feeds two row tiles (the LDS
// return bus bounds the batched math, scan.hip.h).  fold(acc, t, on, aux) for each tile of a pair; an odd last pair re-reads its first tile as
// B and folds it with on = false: nothing to take from it.  Same contract as walk_live_tiles.
template <int QG, int NP, int METRIC, class Src, class Mask, class Fold>
__device__ __forceinline__ uint32_t walk_live_pairs(Mask& m, const TileLoader& L, const float* qb, uint32_t n_tiles, uint32_t n_chunks, uint64_t live, int lane,
                                                    f32x2 (&accA)[QG / 2], f32x2 (&accB)[QG / 2], Fold&& fold) {
  u32x4 buf[2][2 * kLoads];
  typename Mask::Aux auxA[2], auxB[2];
  uint32_t loaded = 0;
  for (uint32_t w0 = 0;; w0 += kWave) {
    if (live != 0ull) {
      const uint32_t n_live = (uint32_t)__popcll(live);
      loaded += n_live;
      const uint32_t n_steps = ((n_live + 1) / 2) * n_chunks;
      uint64_t li = live;  // live tiles not yet issued, the current pair included
      uint64_t ri = li & (li - 1);
      uint32_t tA = w0 + (uint32_t)__ffsll((unsigned long long)li) - 1u, tB = ri ? w0 + (uint32_t)__ffsll((unsigned long long)ri) - 1u : tA, ci = 0;
      auto issue_next = [&](u32x4 (&r)[2 * kLoads], typename Mask::Aux& aA, typename Mask::Aux& aB) __attribute__((always_inline)) {
        const uint32_t soffA = tA * L.tile_bytes + ci * (kLoads * 1024u), soffB = tB * L.tile_bytes + ci * (kLoads * 1024u);
        aA = m.issue(tA);
        aB = m.issue(tB);
#pragma unroll
        for (int i = 0; i < kLoads; ++i) r[i] = __builtin_amdgcn_raw_buffer_load_b128(L.rsrc, L.lane_off, soffA + (uint32_t)i * 1024u, tile_aux<Src::kStreamOnce>());
#pragma unroll
        for (int i = 0; i < kLoads; ++i) r[kLoads + i] = __builtin_amdgcn_raw_buffer_load_b128(L.rsrc, L.lane_off, soffB + (uint32_t)i * 1024u, tile_aux<Src::kStreamOnce>());
        if (ci + 1 < n_chunks) ++ci;
        else if (ri & (ri - 1)) {  // another pair (else: stay on the last chunk, a harmless re-read)
          li = ri & (ri - 1);
          ri = li & (li - 1);
          tA = w0 + (uint32_t)__ffsll((unsigned long long)li) - 1u;
          tB = ri ? w0 + (uint32_t)__ffsll((unsigned long long)ri) - 1u : tA;
          ci = 0;
        }
      };
      issue_next(buf[0], auxA[0], auxB[0]);
      uint64_t lc = live;  // live tiles not yet consumed, the current pair included
      uint32_t cc = 0;
      for (uint32_t s0 = 0; s0 < n_steps; s0 += 2) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          issue_next(buf[b ^ 1], auxA[b ^ 1], auxB[b ^ 1]);
          if (s0 + b < n_steps) {  // uniform
            tile_chunk_compute2<QG, NP, METRIC>(accA, accB, buf[b], qb, cc);
            if (++cc == n_chunks) {
              cc = 0;
              const uint64_t rc = lc & (lc - 1);
              fold(accA, w0 + (uint32_t)__ffsll((unsigned long long)lc) - 1u, true, auxA[b]);
              fold(accB, rc ? w0 + (uint32_t)__ffsll((unsigned long long)rc) - 1u : w0, rc != 0ull, auxB[b]);
              lc = rc & (rc - 1);
            }
          }
        }
      }
    }
    if (w0 + kWave >= n_tiles) break;
    live = m.window(w0 + kWave, n_tiles, lane);  // the next window's words, between windows: the ring has drained
  }
  return loaded;
}

}  // namespace vers
