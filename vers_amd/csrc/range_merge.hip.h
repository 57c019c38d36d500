// range_merge.hip.h -- the cross-rank merge of a sharded range search: `world` variable-length sorted runs of (key, id) pairs per query
// -> one CSR result (vers_range_merge_dev, vers_ivf_range_search_sharded_dev).
//
// The top-k merge (rank_merge_kernel, finish.hip.h: one wave per query over world x top_k slots) does not carry over: a query may own 10^5
// results and its neighbour none.  This merge is data-parallel over ELEMENTS instead.  A thread takes one gathered entry -- rank r, index i
// in the rank's array, a coalesced load -- finds its query q by bisection of the rank's limits, and stores it at
//     out_lims[q] + (i - rank_lims[r][q]) + SUM over r' != r of lower_bound(run of r' for q, key)
// The keys of a query are unique across ranks (probed rows: make_key(dist, seq) with seq the row's number in the query's probe order over
// the GLOBAL list lengths; exhaustive: make_key(dist, vec id)), so the lower bounds alone give every entry its own position: no ties to
// break, no atomics, the same bytes whichever block runs first.  In walk order the runs ascend by seq -- the key's low word -- and the low
// words are compared instead of the keys.  The distance is decoded from the key's high word (range_decode_kernel's rule).
// Every loop is bounded: the bisections by 64 halvings (they end after log2 of the run), the rank loop by `world`, the element loop by the
// rank's total.  Padding behind a rank's total (the gather pads every rank to the longest) is never read.
#pragma once
#include "scan.hip.h"

namespace vers {

constexpr int kRangeMergeThreads = 256;  // four waves of 64

// out_lims[q] = SUM_r rank_lims[r][q], q = 0 .. b (the last entry: the global total)
static __global__ __launch_bounds__(kRangeMergeThreads) void range_merge_lims_kernel(const uint64_t* rank_lims, uint32_t world, uint32_t b, uint64_t* out_lims) {
  const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q > b) return;
  uint64_t s = 0;
  for (uint32_t r = 0; r < world; ++r) s += rank_lims[(uint64_t)r * (b + 1) + q];
  out_lims[q] = s;
}

// first index in [lo, hi) of `keys` whose (key & mask) is not below `want`; the run ascends by (key & mask)
__device__ __forceinline__ uint64_t range_lower_bound(const uint64_t* keys, uint64_t lo, uint64_t hi, uint64_t want, uint64_t mask) {
  for (int s = 0; s < 64 && lo < hi; ++s) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if ((keys[mid] & mask) < want) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// grid: x = blocks striding over a rank's entries, y = rank.  rank_stride: elements between two ranks' arrays (keys and ids alike).
static __global__ __launch_bounds__(kRangeMergeThreads) void range_merge_kernel(const uint64_t* keys, const uint64_t* ids, uint64_t rank_stride, const uint64_t* rank_lims,
                                                                                uint32_t world, uint32_t b, uint64_t mask, uint64_t* out_ids, float* out_dist) {
  const uint32_t r = blockIdx.y;
  const uint64_t* lims = rank_lims + (uint64_t)r * (b + 1);
  uint64_t n = lims[b];
  if (n > rank_stride) n = rank_stride;  // (a total beyond the rank's array would be the caller's error: never read past it)
  const uint64_t* mine = keys + (uint64_t)r * rank_stride;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t key = mine[i];
    const uint64_t id = ids[(uint64_t)r * rank_stride + i];
    // the query: the last q with lims[q] <= i (empty runs before it share the limit: the last one is the run that holds i)
    uint32_t lo = 0, hi = b;  // invariant: lims[lo] <= i, and lims[hi] > i (lims[b] = n > i)
    for (int s = 0; s < 32 && hi - lo > 1; ++s) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (lims[mid] <= i) lo = mid;
      else hi = mid;
    }
    const uint32_t q = lo;
    uint64_t pos = i - lims[q];
    const uint64_t want = key & mask;
    uint64_t total = 0;
    for (uint32_t o = 0; o < world; ++o) {
      const uint64_t* ol = rank_lims + (uint64_t)o * (b + 1);
      const uint64_t b0 = ol[q], b1 = ol[q + 1];
      pos += b0;  // (summed over every rank, this one included: out_lims[q])
      total += ol[b];
      if (o != r && b1 > b0 && b1 <= rank_stride) pos += range_lower_bound(keys + (uint64_t)o * rank_stride, b0, b1, want, mask) - b0;
    }
    if (pos >= total) continue;  // (limits that are no limits -- not ascending, runs not sorted: never a store outside the result)
    out_ids[pos] = id;
    out_dist[pos] = __uint_as_float(order_bits_to_f32_bits((uint32_t)(key >> 32)));
  }
}

// sorted order of a rank's exhaustive partial: the vec ids out of the sorted keys' low words (the keys stay: they are the result)
static __global__ void range_key_ids_kernel(const uint64_t* keys, uint64_t n, uint64_t* out_ids) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out_ids[i] = (uint32_t)keys[i];
}

// queues the two kernels on `st`; rank_stride == 0 (no rank has a result): the limits alone
inline int32_t launch_range_merge(const uint64_t* keys, const uint64_t* ids, uint64_t rank_stride, const uint64_t* rank_lims, uint32_t world, uint32_t b, bool walk,
                                  uint64_t* out_lims, uint64_t* out_ids, float* out_dist, hipStream_t st) {
  hipLaunchKernelGGL(range_merge_lims_kernel, dim3((unsigned)(((uint64_t)b + 1 + kRangeMergeThreads - 1) / kRangeMergeThreads)), dim3(kRangeMergeThreads), 0, st, rank_lims,
                     world, b, out_lims);
  if (hipGetLastError() != hipSuccess) return VERS_ERR_HIP;
  if (rank_stride == 0 || keys == nullptr) return VERS_OK;
  const uint64_t want_blocks = (rank_stride + kRangeMergeThreads - 1) / kRangeMergeThreads;
  const unsigned bx = (unsigned)(want_blocks < 2048 ? want_blocks : 2048);  // (grid-stride beyond: 2048 x world blocks fill the chip many times over)
  hipLaunchKernelGGL(range_merge_kernel, dim3(bx, world), dim3(kRangeMergeThreads), 0, st, keys, ids, rank_stride, rank_lims, world, b,
                     walk ? 0xFFFFFFFFull : ~0ull, out_ids, out_dist);
  if (hipGetLastError() != hipSuccess) return VERS_ERR_HIP;
  return VERS_OK;
}

}  // namespace vers
