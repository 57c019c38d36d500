// filter.hip.h -- filtered top-k search: the top_k nearest among the vec ids a per-call bitmap allows.
//
// In the reference's terms an EXTENSION: `ids[c].retain(|v| A.contains(v))` for the duration of one call -- a VIRTUAL vers_ivf_remove_batch of
// every id outside A, the index itself untouched.  The result is, bit for bit, what the unfiltered call of the same mode returns on an index
// from which those ids were removed.
//
// The device has no vec id -> storage row map and gets none.  Two kernels instead:
//   filter_tile_mask_kernel  one pass over row_ids (the walk of removal's marking pass, remove_scan_rows_kernel): the caller's bitmap over
//                            VEC IDS becomes one u64 per 64-row STORAGE TILE -- bit r of word t: row 64 t + r holds an allowed vector.
//                            Rebuilt by every call: no staleness protocol against add / remove / compact.
//   filter_scan_kernel       scan_kernel's walk (scan.hip.h: the same items, quads sharing one LDS query block, the register prefetch ring over
//                            (tile, chunk) steps, the ordered f32 chain, wave_topk_fill / _update, `bounds`, `lower`) over the LIVE tiles of
//                            each item only.  Before the streaming loop lane t loads the mask word of tile t of the item; the ballot of
//                            "word != 0" is a wave-uniform 64-bit set and the step walk visits its set bits: a tile whose 64 rows are all
//                            disallowed is never loaded, an item without a live tile returns before its first load and leaves its slots at
//                            kKeyMax (the fill the plan / the driver gave them).  Items of more than 64 tiles go window by window; the next
//                            window's words are loaded between windows, when the ring has drained anyway.
// Sequence numbers stay those of the unfiltered walk (seq_base + row; vec ids for SegSrc), so ivf_merge_kernel and seg_merge_kernel finish
// the call as they are: they count the keys they find and map a sequence number to a vec id whatever was skipped.
//
// What the walk asks of a source beyond scan_kernel's contract: storage_row(it) (range.hip.h).
#pragma once
#include "scan.hip.h"

#pragma clang fp contract(off)

namespace vers {

// slots of vers_ivf_filter_stats
constexpr int kFltTilesPlanned = 0, kFltTilesLoaded = 1, kFltItemsSkipped = 2, kFltRowsAllowed = 3, kFltStats = 4;

struct FilterParams {
  const uint64_t* tile_mask;       // [cap_rows / 64]: bit r of word t = storage row 64 t + r holds an allowed vector
  unsigned long long* stats;       // [kFltStats] of the call (zeroed by the driver)
  unsigned long long* wave_slots;  // [launched waves][4]: every wave's planned | loaded | skipped over the call's passes (zeroed by the driver)
};
// A wave's share of the counters (wave-uniform): summed over its items in registers and added to the wave's OWN slot when it has run out of
// items, with plain stores; filter_stats_fold_kernel sums the slots behind the call's last launch.  Atomics on three shared words serialise
// in the L2 at 13 ns each: one per item was 40 us of a 130 us launch, and even one per wave -- the waves of a short launch finish together
// -- was 16 us of 93 (N = 1M, 64 queries) and 2 us of a single query's 12 (measured).
struct FilterCounts {
  uint32_t planned = 0, loaded = 0, skipped = 0;
};

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

// One work item of a single query (the kernel instantiates QG == 1, NP == 1; the batched items are filter_item2's): scan_item with the tile
// walk restricted to the item's live tiles, one tile per step, a 4-deep ring.
template <int QG, int NP, int METRIC, class Src>
__device__ __forceinline__ void filter_item(const Src& src, const ScanParams& p, const FilterParams& f, uint32_t it, const ItemView<QG>& v, int lane,
                                            bool& nan_seen, FilterCounts& fc) {
  const uint32_t n_tiles = (v.nrows + kWave - 1) / kWave;
  const uint64_t* words = f.tile_mask + (src.storage_row(it) >> 6);
  // window 0's words: lane t holds tile t's (no load inside the streaming loop: scan_item says why)
  uint64_t word = (uint32_t)lane < n_tiles ? words[lane] : 0ull;
  uint64_t live = __ballot(word != 0ull);
  uint32_t loaded = 0;
  if (n_tiles <= (uint32_t)kWave && live == 0ull) {  // nothing allowed in the item: not a byte of it is loaded, its slots stay kKeyMax (wave-uniform)
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
  bool first = true;  // no tile of the item folded yet: the lists are empty

  // end of tile t (of the item): fold its allowed rows into the per-query lists
  auto tile_done = [&](uint32_t t) {
    const uint32_t row = t * kWave + lane;
    const bool valid = row < v.nrows && ((readlane64(word, (int)(t & 63u)) >> lane) & 1ull);  // (an allowed row holds a vector: its id is not 0xFFFFFFFF)
    uint32_t sid = 0;
    if constexpr (Src::kSeqIds) {
      // The sequence number is the vec id: loaded only for tiles in which some allowed row can still enter a list (its distance bits at or
      // below the list's k-th) -- behind the wave-uniform ballot, so that most tiles issue no memory operation between two steps.
      bool ask = false;
#pragma unroll
      for (int qi = 0; qi < QG; ++qi)
        if (qi < 2 * NP && qi < (int)v.nq) {
          const float a = acc[qi >> 1][qi & 1];
          const float dist = METRIC == 0 ? a : __fsub_rn(1.0f, a);
          ask |= valid && f32_to_order_bits(dist) <= (uint32_t)(readlane64(list[qi], (int)p.k - 1) >> 32);
        }
      if (__ballot(ask) != 0) sid = valid ? src.seq_ids(it)[row] : 0u;
    }
#pragma unroll
    for (int qi = 0; qi < QG; ++qi) {
      if (qi < 2 * NP && qi < (int)v.nq) {
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

  // scan_item's register ring over the (live tile, chunk) steps of one window of 64 tiles; every load unconditional (steps past the end
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
          if (s0 + b < n_steps) {  // uniform; no vector-memory op inside (kSeqIds: behind tile_done's ballot)
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

// One batched work item (QG > 1), two LIVE tiles per step: scan_item2 with the tile walk restricted to the item's live tiles (every
// query operand read from LDS feeds two row tiles: the LDS return bus bounds the batched math, scan.hip.h).  An odd last pair re-reads its
// first tile as B, rows masked.  Same contract as filter_item.
template <int QG, int NP, int METRIC, class Src>
__device__ __forceinline__ void filter_item2(const Src& src, const ScanParams& p, const FilterParams& f, uint32_t it, const ItemView<QG>& v, int lane,
                                             bool& nan_seen, FilterCounts& fc) {
  const uint32_t n_tiles = (v.nrows + kWave - 1) / kWave;
  const uint64_t* words = f.tile_mask + (src.storage_row(it) >> 6);
  uint64_t word = (uint32_t)lane < n_tiles ? words[lane] : 0ull;  // window 0's words: lane t holds tile t's
  uint64_t live = __ballot(word != 0ull);
  if (n_tiles <= (uint32_t)kWave && live == 0ull) {  // nothing allowed in the item: not a byte of it is loaded, its slots stay kKeyMax (wave-uniform)
    fc.planned += n_tiles;
    fc.skipped += 1u;
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
  bool first = true;  // no tile of the item folded yet: the lists are empty
  uint32_t loaded = 0;
  // end of tile t (of the item; on = false: the B half of an odd last pair, nothing to fold)
  auto fold = [&](f32x2 (&acc)[QG / 2], uint32_t t, bool on) {
    const uint32_t row = t * kWave + lane;
    const bool valid = on && row < v.nrows && ((readlane64(word, (int)(t & 63u)) >> lane) & 1ull);
    uint32_t sid = 0;
    if constexpr (Src::kSeqIds) {  // the vec id, only where an allowed row can still enter a list (filter_item)
      bool ask = false;
#pragma unroll
      for (int qi = 0; qi < QG; ++qi)
        if (qi < 2 * NP && qi < (int)v.nq) {
          const float a = acc[qi >> 1][qi & 1];
          const float dist = METRIC == 0 ? a : __fsub_rn(1.0f, a);
          ask |= valid && f32_to_order_bits(dist) <= (uint32_t)(readlane64(list[qi], (int)p.k - 1) >> 32);
        }
      if (__ballot(ask) != 0) sid = valid ? src.seq_ids(it)[row] : 0u;
    }
#pragma unroll
    for (int qi = 0; qi < QG; ++qi) {
      if (on && qi < 2 * NP && qi < (int)v.nq) {
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
  // scan_item2's 2-deep register ring over the (live tile pair, chunk) steps of one window of 64 tiles; every load unconditional
  u32x4 buf[2][2 * kLoads];
  for (uint32_t w0 = 0;; w0 += kWave) {
    if (live != 0ull) {
      const uint32_t n_live = (uint32_t)__popcll(live);
      loaded += n_live;
      const uint32_t n_steps = ((n_live + 1) / 2) * p.n_chunks;
      uint64_t li = live;  // live tiles not yet issued, the current pair included
      uint64_t ri = li & (li - 1);
      uint32_t tA = w0 + (uint32_t)__ffsll((unsigned long long)li) - 1u, tB = ri ? w0 + (uint32_t)__ffsll((unsigned long long)ri) - 1u : tA, ci = 0;
      auto issue_next = [&](u32x4 (&r)[2 * kLoads]) {
        const uint32_t soffA = tA * L.tile_bytes + ci * (kLoads * 1024u), soffB = tB * L.tile_bytes + ci * (kLoads * 1024u);
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
      issue_next(buf[0]);
      uint64_t lc = live;  // live tiles not yet consumed, the current pair included
      uint32_t cc = 0;
      for (uint32_t s0 = 0; s0 < n_steps; s0 += 2) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          issue_next(buf[b ^ 1]);
          if (s0 + b < n_steps) {  // uniform; no vector-memory op inside (kSeqIds: behind fold's ballot)
            tile_chunk_compute2<QG, NP, METRIC>(accA, accB, buf[b], v.qb, cc);
            if (++cc == p.n_chunks) {
              cc = 0;
              const uint64_t rc = lc & (lc - 1);
              fold(accA, w0 + (uint32_t)__ffsll((unsigned long long)lc) - 1u, true);
              fold(accB, rc ? w0 + (uint32_t)__ffsll((unsigned long long)rc) - 1u : w0, rc != 0ull);
              lc = rc & (rc - 1);
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

// scan_kernel's grid and hand-out (QG == 1: waves stride over items, filter_item; QG > 1: quads share one LDS query block, filter_item2).
template <int QG, int METRIC, class Src>
__global__ __launch_bounds__(kWave * kWavesPerBlock) void filter_scan_kernel(Src src, ScanParams p, FilterParams f) {
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
      filter_item<1, 1, METRIC>(src, p, f, it, v, lane, nan_seen, fc);
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
          case 1: filter_item2<8, 1, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 2: filter_item2<8, 2, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 3: filter_item2<8, 3, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          default: filter_item2<8, 4, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
        }
      } else {
        switch (np) {
          case 1: filter_item2<16, 1, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 2: filter_item2<16, 2, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 3: filter_item2<16, 3, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 4: filter_item2<16, 4, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 5: filter_item2<16, 5, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 6: filter_item2<16, 6, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          case 7: filter_item2<16, 7, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
          default: filter_item2<16, 8, METRIC>(src, p, f, it, v, lane, nan_seen, fc); break;
        }
      }
    }
  }
  if (__ballot(nan_seen) != 0 && lane == 0) atomicOr(p.status, 1u);
  if (lane < 3 && fc.planned != 0u)  // the wave's counters into its own slot, once (a call's passes run one after the other on the stream)
    f.wave_slots[((size_t)blockIdx.x * kWavesPerBlock + wid) * 4 + lane] += (unsigned long long)(lane == kFltTilesPlanned ? fc.planned : lane == kFltTilesLoaded ? fc.loaded : fc.skipped);
}

}  // namespace vers
