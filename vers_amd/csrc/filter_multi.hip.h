// filter_multi.hip.h -- filtered top-k search with a filter PER QUERY: up to kFltMaxFilters bitmaps per call, query q uses bitmap filter_of[q].
//
// Semantics: none of its own.  Row q of a multi call is, bit for bit, row q of the per-call filtered search (filter.hip.h) made with bitmap
// filter_of[q]: the same virtual removal, query by query.
//
// A mask word per (query of the group, tile) would cost 2 QG registers in a kernel that sits at 239 of 256 at QG = 16.  The
// layout here turns the mask around -- a word per ROW, a bit per BITMAP -- so that a wave carries one word per lane whatever QG is:
//   filter_multi_mask_kernel  one pass over row_ids, one wave per 64-row storage tile (filter_tile_mask_kernel's walk):
//                               row_sets[r]   bit f: storage row r holds a vector that bitmap f allows
//                               tile_sets[t]  bit f: some row of storage tile t is allowed by bitmap f (one ballot per bitmap)
//                             Slack and freed rows get 0.  Rebuilt by every call, like the per-call mask.
//   filter_multi_scan_kernel  filter_scan_kernel's walk.  Before the streaming loop lane qi loads filter_of of the item's query qi (an index at
//                             or beyond n_filters selects the empty filter and never reaches the masks); the OR of the live queries' bits is
//                             the item's filter set S, wave-uniform.  Lane t loads tile_sets of tile t; a tile is LIVE when its word meets S.
//                             The walk over the live tiles, the windows of 64 tiles, the register ring, `bounds`, `lower`, the hand-out counter
//                             and the wave-slot counters are filter_item's / filter_item2's.  Every step of the ring also loads the lane's
//                             row_sets word of the step's tile (8 bytes, unconditional, issued with the step's row loads and counted with
//                             them: a load outside the ring would drain it at every tile boundary, scan.hip.h); at the fold (row, qi) is
//                             valid when row < nrows and bit filter_of[qi] of the lane's word is set.
// A tile that is live for one query of a group only is loaded for the group; the other queries take no row from it.  A NaN distance counts
// for valid (row, query) pairs only.
//
// What the walk asks of a source beyond filter.hip.h's contract: range_query(it, qi), the batch's query behind slot qi of the item (range.hip.h).
#pragma once
#include "filter.hip.h"

#pragma clang fp contract(off)

namespace vers {

constexpr uint32_t kFltMaxFilters = 64;        // (VERS_FILTER_MAX: a bit per bitmap in one u64)
constexpr uint32_t kFltNoFilter = 0xFFFFFFFFu;  // a query whose filter_of entry is out of range: the empty filter

typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

struct FilterMultiParams {
  const uint64_t* row_sets;        // [n_tiles * 64]: bit f of word r = storage row r holds a vector bitmap f allows
  const uint64_t* tile_sets;       // [n_tiles]: bit f of word t = some row of storage tile t is allowed by bitmap f
  const uint32_t* filter_of;       // [b]: the bitmap of each query of the batch
  uint32_t n_filters;
  unsigned long long* stats;       // [kFltStats] of the call (FilterParams)
  unsigned long long* wave_slots;  // [launched waves][4] (FilterParams)
};

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

// The row_sets words of one item: lane l of tile t reads word 64 t + l of the item, through a buffer resource of its own (a step past the
// item's rows reads 0, never memory).
struct RowSetLoader {
  __amdgpu_buffer_rsrc_t rsrc;
  uint32_t lane_off;  // lane * 8 bytes
  __device__ __forceinline__ void init(const uint64_t* base, uint32_t n_tiles, int lane) {
    rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)(n_tiles * (kWave * 8u)), 0x00020000);
    lane_off = (uint32_t)lane * 8u;
  }
  __device__ __forceinline__ u32x2 issue(uint32_t tile) const { return __builtin_amdgcn_raw_buffer_load_b64(rsrc, lane_off, tile * (kWave * 8u), 0); }
};
__device__ __forceinline__ uint64_t row_set_word(u32x2 w) { return ((uint64_t)w.y << 32) | (uint64_t)w.x; }

// The item's per-query bitmaps: lane qi gets query qi's (kFltNoFilter: out of range), the return value is the item's filter set.
template <int QG, class Src>
__device__ __forceinline__ uint64_t item_filter_set(const Src& src, const FilterMultiParams& f, uint32_t it, uint32_t nq, int lane, uint32_t& vf) {
  vf = kFltNoFilter;
  if (lane < QG && lane < (int)nq) {
    const uint32_t x = f.filter_of[src.range_query(it, lane)];
    vf = x < f.n_filters ? x : kFltNoFilter;
  }
  uint64_t S = 0ull;
#pragma unroll
  for (int qi = 0; qi < QG; ++qi) {
    const uint32_t fq = (uint32_t)__builtin_amdgcn_readlane((int)vf, qi);
    if (fq != kFltNoFilter) S |= 1ull << (fq & 63u);
  }
  return S;
}

// filter_item with a filter per query (the kernel instantiates QG == 1, NP == 1).
template <int QG, int NP, int METRIC, class Src>
__device__ __forceinline__ void filter_multi_item(const Src& src, const ScanParams& p, const FilterMultiParams& f, uint32_t it, const ItemView<QG>& v, int lane,
                                                  bool& nan_seen, FilterCounts& fc) {
  const uint32_t n_tiles = (v.nrows + kWave - 1) / kWave;
  const uint32_t srow0 = src.storage_row(it);
  const uint64_t* words = f.tile_sets + (srow0 >> 6);
  uint32_t vf;
  const uint64_t S = item_filter_set<QG>(src, f, it, v.nq, lane, vf);
  // window 0's words: lane t holds tile t's (no load inside the streaming loop but the ring's own)
  uint64_t word = (uint32_t)lane < n_tiles ? words[lane] : 0ull;
  uint64_t live = __ballot((word & S) != 0ull);
  uint32_t loaded = 0;
  if (n_tiles <= (uint32_t)kWave && live == 0ull) {  // nothing allowed to any query of the item: not a byte of it is loaded (wave-uniform)
    fc.planned += n_tiles;
    fc.skipped += 1u;
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
  RowSetLoader R;
  R.init(f.row_sets + srow0, n_tiles, lane);
  f32x2 acc[(QG + 1) / 2];
#pragma unroll
  for (int p2 = 0; p2 < (QG + 1) / 2; ++p2) acc[p2] = f32x2{0.0f, 0.0f};
  uint32_t vseq = 0;
  uint64_t vout = 0;
  if (lane < QG && lane < (int)v.nq) {
    vseq = Src::kSeqIds ? 0u : src.seq_base(it, lane);
    vout = (uint64_t)src.out(it, lane);
  }
  bool first = true;  // no tile of the item folded yet: the lists are empty

  // end of tile t (of the item), rw: the lane's row_sets word of it
  auto tile_done = [&](uint32_t t, u32x2 rw) {
    const uint32_t row = t * kWave + lane;
    const uint64_t rs = row < v.nrows ? row_set_word(rw) : 0ull;
    uint32_t sid = 0;
    if constexpr (Src::kSeqIds) {  // the vec id, only where an allowed row can still enter a list (filter_item)
      bool ask = false;
#pragma unroll
      for (int qi = 0; qi < QG; ++qi)
        if (qi < 2 * NP && qi < (int)v.nq) {
          const uint32_t fq = (uint32_t)__builtin_amdgcn_readlane((int)vf, qi);
          const bool valid = fq != kFltNoFilter && ((rs >> (fq & 63u)) & 1ull);
          const float a = acc[qi >> 1][qi & 1];
          const float dist = METRIC == 0 ? a : __fsub_rn(1.0f, a);
          ask |= valid && f32_to_order_bits(dist) <= (uint32_t)(readlane64(list[qi], (int)p.k - 1) >> 32);
        }
      if (__ballot(ask) != 0) sid = (rs & S) != 0ull ? src.seq_ids(it)[row] : 0u;
    }
#pragma unroll
    for (int qi = 0; qi < QG; ++qi) {
      if (qi < 2 * NP && qi < (int)v.nq) {
        const uint32_t fq = (uint32_t)__builtin_amdgcn_readlane((int)vf, qi);
        const bool valid = fq != kFltNoFilter && ((rs >> (fq & 63u)) & 1ull);
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
  };

  // filter_item's register ring over the (live tile, chunk) steps of one window of 64 tiles; every load unconditional
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
          if (s0 + b < n_steps) {  // uniform; no vector-memory op inside (kSeqIds: behind tile_done's ballot)
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
  fc.planned += n_tiles;
  fc.loaded += loaded;
  if (loaded == 0) fc.skipped += 1u;
  if (loaded == 0) return;  // (an item of several windows without a live tile: slots stay kKeyMax)
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

// filter_item2 with a filter per query: two LIVE tiles per step, a row_sets word per tile and lane.
template <int QG, int NP, int METRIC, class Src>
__device__ __forceinline__ void filter_multi_item2(const Src& src, const ScanParams& p, const FilterMultiParams& f, uint32_t it, const ItemView<QG>& v, int lane,
                                                   bool& nan_seen, FilterCounts& fc) {
  const uint32_t n_tiles = (v.nrows + kWave - 1) / kWave;
  const uint32_t srow0 = src.storage_row(it);
  const uint64_t* words = f.tile_sets + (srow0 >> 6);
  uint32_t vf;
  const uint64_t S = item_filter_set<QG>(src, f, it, v.nq, lane, vf);
  uint64_t word = (uint32_t)lane < n_tiles ? words[lane] : 0ull;  // window 0's words: lane t holds tile t's
  uint64_t live = __ballot((word & S) != 0ull);
  if (n_tiles <= (uint32_t)kWave && live == 0ull) {  // nothing allowed to any query of the item: not a byte of it is loaded (wave-uniform)
    fc.planned += n_tiles;
    fc.skipped += 1u;
    return;
  }
  uint64_t list[QG];
#pragma unroll
  for (int qi = 0; qi < QG; ++qi) list[qi] = kKeyMax;
  TileLoader L;
  L.init(v.rows, (uint64_t)n_tiles * kWave * p.ld * 4u, p.ld, lane);
  RowSetLoader R;
  R.init(f.row_sets + srow0, n_tiles, lane);
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
  bool first = true;  // no tile of the item folded yet: the lists are empty
  uint32_t loaded = 0;
  // end of tile t (of the item; on = false: the B half of an odd last pair, nothing to fold), rw: the lane's row_sets word of it
  auto fold = [&](f32x2 (&acc)[QG / 2], uint32_t t, bool on, u32x2 rw) {
    const uint32_t row = t * kWave + lane;
    const uint64_t rs = on && row < v.nrows ? row_set_word(rw) : 0ull;
    uint32_t sid = 0;
    if constexpr (Src::kSeqIds) {  // the vec id, only where an allowed row can still enter a list (filter_item)
      bool ask = false;
#pragma unroll
      for (int qi = 0; qi < QG; ++qi)
        if (qi < 2 * NP && qi < (int)v.nq) {
          const uint32_t fq = (uint32_t)__builtin_amdgcn_readlane((int)vf, qi);
          const bool valid = fq != kFltNoFilter && ((rs >> (fq & 63u)) & 1ull);
          const float a = acc[qi >> 1][qi & 1];
          const float dist = METRIC == 0 ? a : __fsub_rn(1.0f, a);
          ask |= valid && f32_to_order_bits(dist) <= (uint32_t)(readlane64(list[qi], (int)p.k - 1) >> 32);
        }
      if (__ballot(ask) != 0) sid = (rs & S) != 0ull ? src.seq_ids(it)[row] : 0u;
    }
#pragma unroll
    for (int qi = 0; qi < QG; ++qi) {
      if (on && qi < 2 * NP && qi < (int)v.nq) {
        const uint32_t fq = (uint32_t)__builtin_amdgcn_readlane((int)vf, qi);
        const bool valid = fq != kFltNoFilter && ((rs >> (fq & 63u)) & 1ull);
        const float a = acc[qi >> 1][qi & 1];
        const float dist = METRIC == 0 ? a : __fsub_rn(1.0f, a);
        nan_seen |= valid && (dist != dist);
        const uint32_t seq = Src::kSeqIds ? sid : (uint32_t)__builtin_amdgcn_readlane((int)vseq, qi) + row;
        uint64_t cand = valid ? make_key(dist, seq) : kKeyMax;
        if (p.lower != nullptr && cand <= readlane64(vlower, qi)) cand = kKeyMax;  // ranked in an earlier pass
        const uint64_t bnd = p.bounds != nullptr ? readlane64(vbound, qi) : kKeyMax;
        if (first && p.k <= 16 && bnd == kKeyMax) wave_topk_fill(list[qi], p.k, cand, lane);
        else wave_topk_update(list[qi], p.k, cand, bnd);
      }
      acc[qi >> 1][qi & 1] = 0.0f;
    }
    first = false;
  };
  // filter_item2's 2-deep register ring over the (live tile pair, chunk) steps of one window of 64 tiles; every load unconditional
  u32x4 buf[2][2 * kLoads];
  u32x2 rswA[2], rswB[2];
  for (uint32_t w0 = 0;; w0 += kWave) {
    if (live != 0ull) {
      const uint32_t n_live = (uint32_t)__popcll(live);
      loaded += n_live;
      const uint32_t n_steps = ((n_live + 1) / 2) * p.n_chunks;
      uint64_t li = live;  // live tiles not yet issued, the current pair included
      uint64_t ri = li & (li - 1);
      uint32_t tA = w0 + (uint32_t)__ffsll((unsigned long long)li) - 1u, tB = ri ? w0 + (uint32_t)__ffsll((unsigned long long)ri) - 1u : tA, ci = 0;
      auto issue_next = [&](u32x4 (&r)[2 * kLoads], u32x2& rwA, u32x2& rwB) {
        const uint32_t soffA = tA * L.tile_bytes + ci * (kLoads * 1024u), soffB = tB * L.tile_bytes + ci * (kLoads * 1024u);
        rwA = R.issue(tA);
        rwB = R.issue(tB);
#pragma unroll
        for (int i = 0; i < kLoads; ++i) r[i] = __builtin_amdgcn_raw_buffer_load_b128(L.rsrc, L.lane_off, soffA + (uint32_t)i * 1024u, tile_aux<Src::kStreamOnce>());
#pragma unroll
        for (int i = 0; i < kLoads; ++i) r[kLoads + i] = __builtin_amdgcn_raw_buffer_load_b128(L.rsrc, L.lane_off, soffB + (uint32_t)i * 1024u, tile_aux<Src::kStreamOnce>());
        if (ci + 1 < p.n_chunks) ++ci;
        else if (ri & (ri - 1)) {  // another pair (else: stay on the last chunk, a harmless re-read)
          li = ri & (ri - 1);
          ri = li & (li - 1);
          tA = w0 + (uint32_t)__ffsll((unsigned long long)li) - 1u;
          tB = ri ? w0 + (uint32_t)__ffsll((unsigned long long)ri) - 1u : tA;
          ci = 0;
        }
      };
      issue_next(buf[0], rswA[0], rswB[0]);
      uint64_t lc = live;  // live tiles not yet consumed, the current pair included
      uint32_t cc = 0;
      for (uint32_t s0 = 0; s0 < n_steps; s0 += 2) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          issue_next(buf[b ^ 1], rswA[b ^ 1], rswB[b ^ 1]);
          if (s0 + b < n_steps) {  // uniform; no vector-memory op inside (kSeqIds: behind fold's ballot)
            tile_chunk_compute2<QG, NP, METRIC>(accA, accB, buf[b], v.qb, cc);
            if (++cc == p.n_chunks) {
              cc = 0;
              const uint64_t rc = lc & (lc - 1);
              fold(accA, w0 + (uint32_t)__ffsll((unsigned long long)lc) - 1u, true, rswA[b]);
              fold(accB, rc ? w0 + (uint32_t)__ffsll((unsigned long long)rc) - 1u : w0, rc != 0ull, rswB[b]);
              lc = rc & (rc - 1);
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
  fc.planned += n_tiles;
  fc.loaded += loaded;
  if (loaded == 0) {  // (an item of several windows without a live tile: slots stay kKeyMax)
    fc.skipped += 1u;
    return;
  }
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

// filter_scan_kernel's grid, hand-out and counters over the per-query items.
template <int QG, int METRIC, class Src>
__global__ __launch_bounds__(kWave * kWavesPerBlock) void filter_multi_scan_kernel(Src src, ScanParams p, FilterMultiParams f) {
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
      filter_multi_item<1, 1, METRIC>(src, p, f, it, v, lane, nan_seen, fc);
    }
  } else {
    static_assert(QG == 8 || QG == 16, "query groups are 1, 8 or 16 wide");
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
      const uint32_t np = (v.nq + 1) >> 1;  // live query pairs: dead pairs are not computed (wave-uniform dispatch, as scan_kernel's)
      if constexpr (QG == 8) {
        switch (np) {
          case 1: filter_multi_item2<8, 1, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 2: filter_multi_item2<8, 2, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 3: filter_multi_item2<8, 3, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          default: filter_multi_item2<8, 4, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
        }
      } else {
        switch (np) {
          case 1: filter_multi_item2<16, 1, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 2: filter_multi_item2<16, 2, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 3: filter_multi_item2<16, 3, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 4: filter_multi_item2<16, 4, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 5: filter_multi_item2<16, 5, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 6: filter_multi_item2<16, 6, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 7: filter_multi_item2<16, 7, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          default: filter_multi_item2<16, 8, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
        }
      }
    }
  }
  if (__ballot(nan_seen) != 0 && lane == 0) atomicOr(p.status, 1u);
  if (lane < 3 && fc.planned != 0u)  // the wave's counters into its own slot, once (a call's passes run one after the other on the stream)
    f.wave_slots[((size_t)blockIdx.x * kWavesPerBlock + wid) * 4 + lane] += (unsigned long long)(lane == kFltTilesPlanned ? fc.planned : lane == kFltTilesLoaded ? fc.loaded : fc.skipped);
}

}  // namespace vers
