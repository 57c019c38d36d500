// filter_adaptive.hip.h -- adaptive depth for the probed filtered top-k search: every query of a batch probes lists until min_allowed rows its
// bitmap allows are in reach, between nprobe_min and nprobe_max lists.
//
// Semantics: none of its own.  Row q of an adaptive call is, bit for bit, row q of the filtered search (filter.hip.h; filter_multi.hip.h with a
// bitmap per query) made with nprobe = P_q, the depth adaptive_depth.hpp defines.  P_q depends on the query's list ranking and on the number of
// allowed rows per list only, and the device has both before the scan starts: the mask pass has seen every storage row, the ranked keys are
// in W->probe.  Two kernels between the mask pass and the plan's group step, and a twin of plan_queries_kernel:
//   filter_allowed_len_kernel        allowed_len[L] = allowed live rows of list L: the popcounts of the list's tile_mask words (lists start on
//                                    tile boundaries, a removal closes the gaps inside a list, slack and freed rows have mask bits 0)
//   filter_multi_allowed_len_kernel  the same per bitmap, allowed_len[f * k + L], from the row_sets words: a wave per list, lane f keeps bitmap
//                                    f's count, a tile costs one ballot per bitmap that has a row in it (tile_sets says which)
//   allowed_len_rank_sum_kernel      a sharded handle: the ranks' counts (each rank counts the lists it stores, the others read 0) summed into
//                                    the global ones, between the gather of the counts and the plan
//   plan_queries_adaptive_kernel     plan_queries_kernel with a second running sum: next to the row count of the unfiltered walk (pj_pref: the
//                                    sequence bases must stay those of the plain call) the allowed rows before each rank.  A rank the rule
//                                    does not visit is written as kNoList and adds nothing to cnt; np[q] = P_q.
// Everything behind the plan -- group_scatter_kernel, the filtered scan kernels, ivf_merge_kernel -- runs as it is: a kNoList entry is what a
// sharded or reference-mode plan leaves for a list this GPU does not scan.  The per-batch tables and the partial slots are sized by
// b x P_max, as those of the plain call at nprobe_max.
#pragma once
#include "adaptive_depth.hpp"
#include "plan.hip.h"

namespace vers {

// What the adaptive plan needs beyond PlanQ (PlanQ::P is P_max, the number of ranked lists).
struct AdaptiveQ {
  uint32_t p_min = 0;                     // min(nprobe_min, k)
  uint32_t min_allowed = 0;
  const uint32_t* allowed_len = nullptr;  // [n_filters or 1][k_lists] by centroid index
  const uint32_t* filter_of = nullptr;    // nullable: one bitmap for the batch.  An entry at or beyond n_filters: the empty filter
  uint32_t n_filters = 1;
  uint32_t* out_nprobe = nullptr;         // nullable, [b]
};

constexpr int kAdpThreads = 256;  // four waves: a list (the count kernels) or a query (the plan) each

// owner (nullable) / rank: a handle sharded by cluster counts the lists it stores; a list of another rank's is written as 0 and neither its
// list_off (which means nothing here) nor a mask word is read.  Every list has one owner: the ranks' counts add up to the global ones.
static __global__ __launch_bounds__(kAdpThreads) void filter_allowed_len_kernel(const uint64_t* tile_mask, const uint32_t* list_off, const uint32_t* list_len,
                                                                               uint32_t k_lists, uint32_t* allowed_len, const uint8_t* owner, uint32_t rank) {
  const uint32_t L = blockIdx.x * (kAdpThreads / kWave) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (L >= k_lists) return;  // (whole waves)
  if (owner != nullptr && (uint32_t)owner[L] != rank) {  // (wave-uniform)
    if (lane == 0) allowed_len[L] = 0u;
    return;
  }
  const uint32_t n_tiles = (list_len[L] + kWave - 1) / kWave;
  const uint64_t* words = tile_mask + (n_tiles ? (list_off[L] >> 6) : 0u);
  uint32_t n = 0;
  for (uint32_t t = (uint32_t)lane; t < n_tiles; t += kWave) n += (uint32_t)__popcll(words[t]);
  for (int s = 32; s >= 1; s >>= 1) n += __shfl_xor(n, s);
  if (lane == 0) allowed_len[L] = n;
}

static __global__ __launch_bounds__(kAdpThreads) void filter_multi_allowed_len_kernel(const uint64_t* row_sets, const uint64_t* tile_sets, const uint32_t* list_off,
                                                                                     const uint32_t* list_len, uint32_t k_lists, uint32_t n_filters,
                                                                                     uint32_t* allowed_len, const uint8_t* owner, uint32_t rank) {
  const uint32_t L = blockIdx.x * (kAdpThreads / kWave) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (L >= k_lists) return;  // (whole waves)
  if (owner != nullptr && (uint32_t)owner[L] != rank) {  // (wave-uniform; filter_allowed_len_kernel's guard)
    if ((uint32_t)lane < n_filters) allowed_len[(uint64_t)lane * k_lists + L] = 0u;
    return;
  }
  const uint32_t n_tiles = (list_len[L] + kWave - 1) / kWave;
  const uint64_t t0 = n_tiles ? (uint64_t)(list_off[L] >> 6) : 0ull;
  uint32_t mine = 0;  // lane f: bitmap f's rows in the list
  for (uint32_t w0 = 0; w0 < n_tiles; w0 += kWave) {  // windows of 64 tiles: lane t holds tile w0 + t's set of bitmaps
    const uint64_t word = w0 + (uint32_t)lane < n_tiles ? tile_sets[t0 + w0 + lane] : 0ull;
    uint64_t live = __ballot(word != 0ull);
    if (live == 0ull) continue;
    uint64_t rs_next = row_sets[(t0 + w0 + (uint32_t)(__ffsll((unsigned long long)live) - 1)) * kWave + lane];
    while (live) {
      const int t = __ffsll((unsigned long long)live) - 1;
      live &= live - 1;
      const uint64_t rs = rs_next;
      if (live) rs_next = row_sets[(t0 + w0 + (uint32_t)(__ffsll((unsigned long long)live) - 1)) * kWave + lane];  // (the next live tile's words: in flight under the ballots)
      uint64_t todo = readlane64(word, t);  // the bitmaps with a row in this tile (bits below n_filters only)
      while (todo) {
        const int f = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t c = (uint32_t)__popcll(__ballot((rs >> f) & 1ull));
        if (lane == f) mine += c;
      }
    }
  }
  if ((uint32_t)lane < n_filters) allowed_len[(uint64_t)lane * k_lists + L] = mine;
}

// The allowed counts of a sharded handle's ranks, gathered as [world][n] (n = n_filters x k_lists), summed into the global ones: every list
// has exactly one owner and the others wrote 0 for it, so the sum is that owner's count.
static __global__ __launch_bounds__(kAdpThreads) void allowed_len_rank_sum_kernel(const uint32_t* gathered, uint32_t world, uint64_t n, uint32_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * kAdpThreads + threadIdx.x;
  if (i >= n) return;
  uint32_t sum = 0;
  for (uint32_t r = 0; r < world; ++r) sum += gathered[(uint64_t)r * n + i];
  out[i] = sum;
}

// One chunk (64 probe ranks) of a query's adaptive plan: plan_query_chunk in nprobe mode with the depth rule in place of "every ranked list".
// `carry` links the row counts of the chunks, `acarry` the allowed-row counts.
__device__ __forceinline__ void plan_adaptive_chunk(const PlanQ& a, const AdaptiveQ& ad, const uint32_t* alen, uint32_t q, int lane, uint32_t c0, uint64_t key,
                                                    uint32_t& carry, uint32_t& acarry, uint32_t& n_visited) {
  const uint32_t j = c0 + (uint32_t)lane;
  const uint32_t L = (j < a.P && key != kKeyMax) ? (uint32_t)key : kNoList;  // centroid index
  const uint32_t len = L != kNoList ? a.list_len[L] : 0u;
  const uint32_t slot = L != kNoList ? a.list_slot[L] : kNoList;
  const uint32_t al = (L != kNoList && alen != nullptr) ? alen[L] : 0u;
  const uint32_t own = (a.owner != nullptr && L != kNoList) ? (uint32_t)a.owner[L] : a.rank;  // (plan_query_chunk's: with the lengths)
  const uint32_t inc = wave_incl_u32(len);
  const uint32_t pref = carry + inc - len;
  carry += (uint32_t)__builtin_amdgcn_readlane((int)inc, kWave - 1);
  const uint32_t ainc = wave_incl_u32(al);
  const uint32_t abefore = acarry + ainc - al;
  acarry += (uint32_t)__builtin_amdgcn_readlane((int)ainc, kWave - 1);
  const bool visited = L != kNoList && adaptive_rank_visited(j, abefore, ad.p_min, a.P, ad.min_allowed);
  // (lists the filter empties are scanned as the plain call scans them: the kernel skips their tiles.  Depth, pj_pref and np come from the
  // GLOBAL lengths and allowed counts -- the same on every rank of a sharded handle --, the scan and cnt cover the lists this rank stores)
  const bool scan = visited && len > 0 && a.top_k > 0 && own == a.rank;
  if (j < a.P) {
    a.pj_list[(uint64_t)q * a.P + j] = scan ? slot : kNoList;
    a.pj_pref[(uint64_t)q * a.P + j] = pref;
    a.pj_take[(uint64_t)q * a.P + j] = visited ? a.top_k : 0u;
    if (a.pj_nq) {
      const uint32_t sr = list_seg_rows(len, a.seg_rows, a.seg_target);
      a.pj_nq[(uint64_t)q * a.P + j] = scan ? ((len + sr - 1) / sr + 3) / 4 : 0u;
    }
  }
  if (scan) atomicAdd(&a.cnt[slot], 1u);
  if (scan && c0 == 0 && j < a.hot_ranks) a.hot[slot] = 1u;
  n_visited += (uint32_t)__popcll(__ballot(visited));
}

// plan_queries_kernel's twin: a wave per query reads its P_max ranked lists from `probe`.
static __global__ __launch_bounds__(kAdpThreads) void plan_queries_adaptive_kernel(PlanQ a, AdaptiveQ ad, const uint64_t* probe) {
  const uint32_t q = blockIdx.x * (kAdpThreads / kWave) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (q >= a.b) return;  // (whole waves)
  const uint32_t* alen = ad.allowed_len;
  if (ad.filter_of != nullptr) {
    const uint32_t f = ad.filter_of[q];
    alen = f < ad.n_filters ? ad.allowed_len + (uint64_t)f * a.k_lists : nullptr;  // (out of range: the empty filter, every a_j is 0)
  }
  uint32_t carry = 0, acarry = 0, n_visited = 0;
  for (uint32_t c0 = 0; c0 < a.P; c0 += kWave) {
    const uint32_t j = c0 + (uint32_t)lane;
    plan_adaptive_chunk(a, ad, alen, q, lane, c0, j < a.P ? probe[(uint64_t)q * a.P + j] : kKeyMax, carry, acarry, n_visited);
  }
  if (lane == 0) {
    a.np[q] = n_visited;
    if (ad.out_nprobe != nullptr) ad.out_nprobe[q] = n_visited;
  }
}

}  // namespace vers
