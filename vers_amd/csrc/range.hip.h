// range.hip.h -- range search over the inverted lists: every row of the probed lists whose distance to the query is <= its radius.
//
// In the reference's terms an EXTENSION (ivfflat.rs has search_approximate only): the rows `ids[c]` of the min(nprobe, k) nearest
// lists, each scored with the reference's own arithmetic (scan.hip.h: one strictly ordered f32 chain per (row, query), separately
// rounded multiply and add) and kept when `dist <= radius[q]`, a plain f32 comparison.  No top_k, so no top-k fold: the result of a
// work item is a COUNT per query, and the whole result is laid out by a prefix sum over the counts --
//   pass 1 (FILL = false)  count the hits of every (query, probe, segment) slot;
//   prefix scan            slot order IS query-major, probe rank, segment: base[slot] is where the slot's hits start, the query's
//                          first slot its CSR limit, the last entry the total;
//   pass 2 (FILL = true)   the same walk; a hit is stored at base[slot] + hits of the slot's earlier tiles + hits in lower lanes.
// Every position is a function of the data alone: no atomics on the output, the same bytes whichever block takes which item.
// Items none of whose queries counted a hit are skipped before their first load, so with a small radius pass 2 streams almost nothing.
//
// The walk is scan_kernel's (scan.hip.h): the same items (IvfSrc<QG>, QG 1 / 8 / 16), quads sharing one LDS query block, the same
// register prefetch ring over (tile, chunk) steps -- built from TileLoader, tile_chunk_compute and ItemView as they are.
//
// + the EXHAUSTIVE range search (vers_flat_range_search, vers_ivf_range_search_exhaustive): the same two passes over the segment items of
// the exhaustive top-k scans (FlatSrc / SegSrc<QG, true>, QG 1 / 8; slot = q * n_segs + segment, which is query-major too).  One walk
// serves the three sources; what it asks of a source beyond scan_kernel's contract:
//   uint32_t range_query(it, qi) const    the batch's query behind slot qi of the item (its radius)
//   uint64_t range_slot(it, qi) const     the count slot of (item, query); one item per slot, a query's slots contiguous and ascending in walk order
//   uint32_t storage_row(it) const        the item's first storage row (row_ids index / row number)
//   static constexpr int kRangeRows       what a row of the item is (the constants: scan.hip.h) --
//       kRangeRowsListed  a row of an inverted list: live, vec id = row_ids[storage row]; the sort key carries the walk's sequence number
//                         (ties in probe-rank order) and the ids are staged beside the keys
//       kRangeRowsStored  a storage row of the index: row_ids[storage row] == 0xFFFFFFFF marks slack and freed rows, which are no result --
//                         in the count pass and in the fill pass alike, or the positions drift.  The id is loaded only for tiles in which
//                         some lane is within its radius (or NaN), behind the wave-uniform ballot: no load inside the streaming loop otherwise
//       kRangeRowsFlat    a row of the flat corpus: vec id = row number, every row below n is live, no id load at all
//     Stored / Flat: the sort key is make_key(dist, vec id) -- utils::search_exhaustive's stable order -- so the sorted keys alone
//     decode to (id, distance) and no id array is staged.
// On a handle sharded by cluster the same passes run over the lists (rows) the rank stores and end in (key, id) pairs; the cross-rank merge
// is range_merge.hip.h.
#pragma once
#include "scan.hip.h"

#pragma clang fp contract(off)

namespace vers {

struct RangeParams {
  uint32_t ld;              // columns of the blocked matrix
  uint32_t n_chunks;        // ld / kChunk
  uint32_t* status;         // device word: bit0 = NaN distance seen (count pass)
  const float* radius;      // [b]
  uint32_t* counts;         // [b * P * S_max]: hits per slot = pair * S_max + segment (zeroed before the count pass)
  const uint64_t* base;     // FILL: exclusive prefix of counts
  const uint32_t* row_ids;  // storage row -> vec id
  uint64_t* out_keys;       // FILL, sorted order: make_key(dist, seq) staging; nullptr = walk order (out_dist gets the distance itself).
                            // A rank's partial of a sharded search (RangePartial, ivf_search.hip) keeps the keys in walk order too: the caller's array
  uint64_t* out_ids;        // FILL: ids (staging in sorted order, the caller's array in walk order)
  float* out_dist;          // FILL, walk order without keys
  uint32_t* next_quad;      // batched kernels: dynamic quad hand-out counter (zeroed per launch) or nullptr
};

// One work item, NP live query pairs (QG == 1: NP == 1; QG > 1: NP even, tile_chunk_compute reads two pairs per ds_read_b128).
template <int QG, int NP, int METRIC, bool FILL, class Src>
__device__ __forceinline__ void range_item(const Src& src, const RangeParams& p, uint32_t it, const ItemView<QG>& v, int lane, bool& nan_seen) {
  // Per-query constants once, lane qi = query qi, read back with v_readlane (scan_item: no memory load inside the streaming loop).
  constexpr bool kKeyId = Src::kRangeRows != kRangeRowsListed;  // the sort key's low word is the vec id itself
  const bool live = lane < QG && lane < (int)v.nq;
  uint32_t vrad = 0, vseq = 0, vhits = 0;  // vhits: the query's hits in the item's tiles so far
  uint64_t vslot = 0, vbase = 0;
  if (live) {
    vrad = __float_as_uint(p.radius[src.range_query(it, lane)]);
    vslot = src.range_slot(it, lane);
    if (FILL && !kKeyId) vseq = src.seq_base(it, lane);
  }
  uint32_t srow0 = 0;
  if constexpr (!FILL && Src::kRangeRows == kRangeRowsStored) srow0 = src.storage_row(it);
  if constexpr (FILL) {
    const uint32_t had = live ? p.counts[vslot] : 0u;
    if (__ballot(had != 0u) == 0) return;  // nothing to store for any query of the item: not a byte of it is loaded (wave-uniform)
    if (live) vbase = p.base[vslot];
    srow0 = src.storage_row(it);
  }
  const uint32_t n_tiles = (v.nrows + kWave - 1) / kWave;
  TileLoader L;
  L.init(v.rows, (uint64_t)n_tiles * kWave * p.ld * 4u, p.ld, lane);
  f32x2 acc[(QG + 1) / 2];
#pragma unroll
  for (int p2 = 0; p2 < (QG + 1) / 2; ++p2) acc[p2] = f32x2{0.0f, 0.0f};

  // end of a tile: lane r holds row r's exact distance for each live query
  auto tile_done = [&](uint32_t t) {
    const uint32_t row = t * kWave + lane;
    const bool valid = row < v.nrows;  // rows of the last tile beyond the segment: slack, never a result
    if constexpr (!FILL) {
      bool ok = valid;
      if constexpr (Src::kRangeRows == kRangeRowsStored) {
        // is the row a vector at all?  Asked only when the answer matters: some lane is within its radius or NaN (wave-uniform)
        bool ask = false;
#pragma unroll
        for (int qi = 0; qi < QG; ++qi)
          if (qi < 2 * NP && qi < (int)v.nq) {
            const float a = acc[qi >> 1][qi & 1];
            const float dist = METRIC == 0 ? a : __fsub_rn(1.0f, a);
            ask |= valid && !(dist > __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)vrad, qi)));
          }
        if (__ballot(ask) != 0) ok = valid && p.row_ids[srow0 + row] != 0xFFFFFFFFu;
        else ok = false;  // (nothing to count, nothing to report)
      }
#pragma unroll
      for (int qi = 0; qi < QG; ++qi) {
        if (qi < 2 * NP && qi < (int)v.nq) {
          const float a = acc[qi >> 1][qi & 1];
          const float dist = METRIC == 0 ? a : __fsub_rn(1.0f, a);
          nan_seen |= ok && (dist != dist);
          const float r = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)vrad, qi));
          const uint32_t n = (uint32_t)__popcll(__ballot(ok && dist <= r));
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
          any |= valid && dist <= __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)vrad, qi));
        }
      if (__ballot(any) != 0) {  // (wave-uniform; a tile without a hit -- most of them at a small radius -- issues no memory operation)
        uint32_t id32 = srow0 + row;  // (kRangeRowsFlat: the row number is the vec id)
        bool ok = valid;
        if constexpr (Src::kRangeRows != kRangeRowsFlat) id32 = valid ? p.row_ids[srow0 + row] : 0xFFFFFFFFu;
        if constexpr (Src::kRangeRows == kRangeRowsStored) ok = valid && id32 != 0xFFFFFFFFu;  // the count pass's rule, to the letter
        const uint64_t id = id32;
#pragma unroll
        for (int qi = 0; qi < QG; ++qi)
          if (qi < 2 * NP && qi < (int)v.nq) {
            const float a = acc[qi >> 1][qi & 1];
            const float dist = METRIC == 0 ? a : __fsub_rn(1.0f, a);
            const bool hit = ok && dist <= __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)vrad, qi));
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

  // scan_item's register ring: kBufs chunk buffers, every load unconditional (steps past the end re-read the last chunk)
  constexpr int kBufs = QG == 1 ? 4 : 2;
  u32x4 buf[kBufs][kLoads];
  const uint32_t n_steps = n_tiles * p.n_chunks;
  uint32_t ti = 0, ci = 0;  // (tile, chunk) the next issue fetches
  auto issue_next = [&](u32x4 (&r)[kLoads]) {
    L.template issue<tile_aux<Src::kStreamOnce>()>(r, ti, ci);
    if (ci + 1 < p.n_chunks) ++ci;
    else if (ti + 1 < n_tiles) { ci = 0; ++ti; }
  };
  if (n_steps) {
#pragma unroll
    for (int b = 0; b < kBufs - 1; ++b) issue_next(buf[b]);
  }
  uint32_t tc = 0, cc = 0;  // (tile, chunk) being consumed
  for (uint32_t s0 = 0; s0 < n_steps; s0 += kBufs) {
#pragma unroll
    for (int b = 0; b < kBufs; ++b) {
      issue_next(buf[(b + kBufs - 1) % kBufs]);
      if (s0 + b < n_steps) {  // uniform
        tile_chunk_compute<QG, NP, METRIC>(acc, buf[b], v.qb, cc);
        if (++cc == p.n_chunks) {
          cc = 0;
          tile_done(tc++);
        }
      }
    }
  }
  if constexpr (!FILL) {
    if (live) p.counts[vslot] = vhits;  // (one item per slot: a plain store)
  }
}

// FILL = false: the count pass; FILL = true: the fill pass.  Same grid, same items (scan_kernel's contract for Src).
template <int QG, int METRIC, bool FILL, class Src>
__global__ __launch_bounds__(kWave * kWavesPerBlock) void range_scan_kernel(Src src, RangeParams p) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t n_items = src.n_items();
  bool nan_seen = false;
  if constexpr (QG == 1) {
    const uint32_t n_waves = gridDim.x * kWavesPerBlock;
    for (uint32_t it = blockIdx.x * kWavesPerBlock + wid; it < n_items; it += n_waves) {
      ItemView<QG> v;
      src.get(it, v);
      if (v.nrows == 0) continue;
      range_item<1, 1, METRIC, FILL>(src, p, it, v, lane, nan_seen);
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
        if (np <= 2) range_item<8, 2, METRIC, FILL>(src, p, it, v, lane, nan_seen);
        else range_item<8, 4, METRIC, FILL>(src, p, it, v, lane, nan_seen);
      } else {
        switch (np) {
          case 2: range_item<16, 2, METRIC, FILL>(src, p, it, v, lane, nan_seen); break;
          case 4: range_item<16, 4, METRIC, FILL>(src, p, it, v, lane, nan_seen); break;
          case 6: range_item<16, 6, METRIC, FILL>(src, p, it, v, lane, nan_seen); break;
          default: range_item<16, 8, METRIC, FILL>(src, p, it, v, lane, nan_seen); break;
        }
      }
    }
  }
  if constexpr (!FILL) {
    if (__ballot(nan_seen) != 0 && lane == 0) atomicOr(p.status, 1u);
  }
}

// CSR limits off the prefix: lims[q] = base[q * slots_per_query] (q = b: the total); the radii are checked on the way (a NaN radius is
// an argument error, and the device-pointer call sees them here first).  misc: [0..1] total (u64) | [2] status word | [3] NaN radius.
static __global__ void range_lims_kernel(const uint64_t* base, uint64_t slots_per_query, uint32_t b, const float* radius, const uint32_t* status,
                                  uint64_t* lims, uint32_t* misc) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q > b) return;
  const uint64_t v = base[(uint64_t)q * slots_per_query];
  lims[q] = v;
  if (q == b) {
    misc[0] = (uint32_t)v;
    misc[1] = (uint32_t)(v >> 32);
    misc[2] = *status;
  } else if (radius[q] != radius[q]) {
    atomicOr(misc + 3, 1u);
  }
}

// sorted order: the distances back out of the sorted keys' high words
static __global__ void range_decode_kernel(const uint64_t* keys, uint64_t n, float* out_dist) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out_dist[i] = __uint_as_float(order_bits_to_f32_bits((uint32_t)(keys[i] >> 32)));
}

// sorted order of the exhaustive range search: (vec id, distance) out of the sorted keys alone -- low word | high word
static __global__ void range_decode_ids_kernel(const uint64_t* keys, uint64_t n, uint64_t* out_ids, float* out_dist) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const uint64_t k = keys[i];
    out_ids[i] = (uint32_t)k;
    out_dist[i] = __uint_as_float(order_bits_to_f32_bits((uint32_t)(k >> 32)));
  }
}

// vers_range_phases (ivf_search.hip): one finished range call of b queries and `total` results; ms = plan, count, prefix + total, fill, sort
void range_phases_add(uint32_t b, uint64_t total, const float* ms5);

}  // namespace vers
