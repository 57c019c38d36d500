// filter_range.hip.h -- filtered range search: every ALLOWED row within a radius, the allowed set a per-call bitmap of vec ids.
//
// The composition of range.hip.h and filter.hip.h: a VIRTUAL vers_ivf_remove_batch of every id outside the bitmap for the duration of one
// range call.  The result is, bit for bit, what the unfiltered range call of the same mode returns on an index from which those ids were
// removed.
//
// filter_tile_mask_kernel (filter.hip.h) turns the bitmap into one u64 per 64-row storage tile, once per call and before the count pass;
// filter_range_scan_kernel is range_scan_kernel's count / fill walk (range.hip.h: the same items, the same slots, the same prefix between
// the passes, quads sharing one LDS query block, `next_quad`) over the LIVE tiles of each item only, the way filter_item walks them:
// before the streaming loop lane t loads the mask word of tile t of the item, the ballot of "word != 0" is a wave-uniform 64-bit set and
// the ring visits its set bits, one live tile per step.  A tile whose 64 rows are all disallowed is never loaded, in either pass; an item
// without a live tile returns before its first load, in both passes, and its count slots keep the driver's zero.  Items of more than 64
// tiles go window by window; the next window's words are loaded between windows, when the ring has drained anyway.
//
// ONE predicate for both passes, or the positions drift:   row < v.nrows  &&  bit `lane` of the tile's word  &&  dist <= r.
// Both passes read the same words: the call holds the index shared and the mask is built once.  A set bit implies that the row holds a
// vector (the mask kernel never sets one for 0xFFFFFFFF), so the count pass loads no row id at all -- not for kRangeRowsStored either --
// and the fill pass loads one only behind the wave-uniform "some lane hit" ballot, to obtain the id.  A NaN distance is an error on an
// allowed row only (count pass); a disallowed row is not scanned.  Keys, ids and positions are range_item's: base[slot] + hits of the
// item's earlier live tiles + hits in lower lanes; no atomics on the output.
//
// vers_ivf_filter_stats: planned / loaded tile visits and items skipped are counted in the COUNT pass only (FilterCounts, filter.hip.h) --
// what the fill pass skips for lack of hits is range search's own saving, not the filter's.
//
// What the walk asks of a source: range.hip.h's contract (range_query, range_slot, storage_row, kRangeRows).
#pragma once
#include "filter.hip.h"
#include "range.hip.h"

#pragma clang fp contract(off)

namespace vers {

// One work item, NP live query pairs (QG == 1: NP == 1; QG > 1: NP even, as range_item's).
template <int QG, int NP, int METRIC, bool FILL, class Src>
__device__ __forceinline__ void filter_range_item(const Src& src, const RangeParams& p, const FilterParams& f, uint32_t it, const ItemView<QG>& v, int lane,
                                                  bool& nan_seen, FilterCounts& fc) {
  constexpr bool kKeyId = Src::kRangeRows != kRangeRowsListed;  // the sort key's low word is the vec id itself
  const bool liveq = lane < QG && lane < (int)v.nq;
  const uint32_t n_tiles = (v.nrows + kWave - 1) / kWave;
  const uint32_t srow0 = src.storage_row(it);
  const uint64_t* words = f.tile_mask + (srow0 >> 6);
  // window 0's words: lane t holds tile t's (no load inside the streaming loop)
  uint64_t word = (uint32_t)lane < n_tiles ? words[lane] : 0ull;
  uint32_t vrad = 0, vseq = 0, vhits = 0;  // lane qi = query qi; vhits: the query's hits in the item's live tiles so far
  uint64_t vslot = 0, vbase = 0;
  if (liveq) vslot = src.range_slot(it, lane);
  if constexpr (FILL) {
    const uint32_t had = liveq ? p.counts[vslot] : 0u;
    if (__ballot(had != 0u) == 0) return;  // no query of the item counted a hit: not a byte of it is loaded (range_item's rule, wave-uniform)
  }
  uint64_t live = __ballot(word != 0ull);
  if (n_tiles <= (uint32_t)kWave && live == 0ull) {  // nothing allowed in the item: not a byte of it is loaded, its count slots stay zero (wave-uniform)
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
  f32x2 acc[(QG + 1) / 2];
#pragma unroll
  for (int p2 = 0; p2 < (QG + 1) / 2; ++p2) acc[p2] = f32x2{0.0f, 0.0f};
  uint32_t loaded = 0;

  // end of live tile t (of the item): lane r holds row r's exact distance for each live query
  auto tile_done = [&](uint32_t t) {
    const uint32_t row = t * kWave + lane;
    // THE predicate's first two terms, for both passes (an allowed row holds a vector: its id is not 0xFFFFFFFF)
    const bool allowed = row < v.nrows && ((readlane64(word, (int)(t & 63u)) >> lane) & 1ull);
    if constexpr (!FILL) {
#pragma unroll
      for (int qi = 0; qi < QG; ++qi) {
        if (qi < 2 * NP && qi < (int)v.nq) {
          const float a = acc[qi >> 1][qi & 1];
          const float dist = METRIC == 0 ? a : __fsub_rn(1.0f, a);
          nan_seen |= allowed && (dist != dist);
          const float r = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)vrad, qi));
          const uint32_t n = (uint32_t)__popcll(__ballot(allowed && dist <= r));
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
          any |= allowed && dist <= __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)vrad, qi));
        }
      if (__ballot(any) != 0) {  // (wave-uniform; a tile without a hit issues no memory operation)
        uint32_t id32 = srow0 + row;  // (kRangeRowsFlat: the row number is the vec id)
        if constexpr (Src::kRangeRows != kRangeRowsFlat) id32 = allowed ? p.row_ids[srow0 + row] : 0xFFFFFFFFu;
        const uint64_t id = id32;
#pragma unroll
        for (int qi = 0; qi < QG; ++qi)
          if (qi < 2 * NP && qi < (int)v.nq) {
            const float a = acc[qi >> 1][qi & 1];
            const float dist = METRIC == 0 ? a : __fsub_rn(1.0f, a);
            const bool hit = allowed && dist <= __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)vrad, qi));
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

  // filter_item's register ring over the (live tile, chunk) steps of one window of 64 tiles; every load unconditional (steps past the end
  // re-read the last chunk)
  constexpr int kBufs = QG == 1 ? 4 : 2;
  u32x4 buf[kBufs][kLoads];
  for (uint32_t w0 = 0;; w0 += kWave) {
    if (live != 0ull) {
      const uint32_t n_live = (uint32_t)__popcll(live);
      loaded += n_live;
      const uint32_t n_steps = n_live * p.n_chunks;
      uint64_t li = live, lc = live;  // live tiles not yet issued / not yet consumed, the current one included
      uint32_t ti = w0 + (uint32_t)__ffsll((unsigned long long)li) - 1u, ci = 0;  // (tile, chunk) the next issue fetches
      auto issue_next = [&](u32x4 (&r)[kLoads]) {
        L.template issue<tile_aux<Src::kStreamOnce>()>(r, ti, ci);
        if (ci + 1 < p.n_chunks) ++ci;
        else if (li & (li - 1)) { li &= li - 1; ci = 0; ti = w0 + (uint32_t)__ffsll((unsigned long long)li) - 1u; }  // else: stay on the last chunk
      };
#pragma unroll
      for (int b = 0; b < kBufs - 1; ++b) issue_next(buf[b]);
      uint32_t cc = 0;  // chunk being consumed
      for (uint32_t s0 = 0; s0 < n_steps; s0 += kBufs) {
#pragma unroll
        for (int b = 0; b < kBufs; ++b) {
          issue_next(buf[(b + kBufs - 1) % kBufs]);
          if (s0 + b < n_steps) {  // uniform; no vector-memory op inside (FILL: behind tile_done's ballot)
            tile_chunk_compute<QG, NP, METRIC>(acc, buf[b], v.qb, cc);
            if (++cc == p.n_chunks) {
              cc = 0;
              tile_done(w0 + (uint32_t)__ffsll((unsigned long long)lc) - 1u);
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

// FILL = false: the count pass; FILL = true: the fill pass.  range_scan_kernel's grid and hand-out; the count pass leaves the wave's
// filter counters in its own slot (filter_scan_kernel), so the host launches no more waves than there are slots.
template <int QG, int METRIC, bool FILL, class Src>
__global__ __launch_bounds__(kWave * kWavesPerBlock) void filter_range_scan_kernel(Src src, RangeParams p, FilterParams f) {
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
      filter_range_item<1, 1, METRIC, FILL>(src, p, f, it, v, lane, nan_seen, fc);
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
        if (np <= 2) filter_range_item<8, 2, METRIC, FILL>(src, p, f, it, v, lane, nan_seen, fc);
        else filter_range_item<8, 4, METRIC, FILL>(src, p, f, it, v, lane, nan_seen, fc);
      } else {
        switch (np) {
          case 2: filter_range_item<16, 2, METRIC, FILL>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 4: filter_range_item<16, 4, METRIC, FILL>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 6: filter_range_item<16, 6, METRIC, FILL>(src, p, f, it, v, lane, nan_seen, fc); break;
          default: filter_range_item<16, 8, METRIC, FILL>(src, p, f, it, v, lane, nan_seen, fc); break;
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
