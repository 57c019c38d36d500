// fetch.hip.h -- the kernels of vers_ivf_fetch and vers_ivf_search_by_id (ivf_fetch.hip): stored vectors read back by vec id.
//
//   fetch_map_kernel      the vec id -> storage row map (vers_ivf::FetchMap::row_of) from row_ids, over host-made tile jobs (fetch_plan.hpp):
//                         only rows below their list's length are looked at
//   fetch_check_kernel    the range test and the map lookup of a call's ids: the storage row of every request into the call's workspace,
//                         the verdict and the two counts into its counters.  NOTHING of the caller's is written here.
//   fetch_locate_kernel   the same without the map (its allocation failed): the pass over the live rows looks every vec id up in the call's
//                         sorted requests
//   fetch_meta_kernel     clusters and status, after the host has read the verdict: the list of a storage row by binary search over the
//                         CURRENT list_off (upd::list_of_row; tile_list is stale after a re-layout)
//   fetch_rows_rm_kernel  the gather from the row-major copy: a wave per requested row, whole sectors in, contiguous stores out
//   fetch_tiles_kernel    the gather from the f32 tiles: the requests ordered by storage row, a block per touched tile
//   byid_drop_self_kernel VERS_BYID_EXCLUDE_SELF: the search's top_k + 1 rows without the query's own id
//   shard_*_kernel        handles sharded by cluster: the rank's words of the where round, the source list of a packed chunk, clusters and
//                         status from the resolved table, and the rows of a gathered chunk to their requests (a wave per row)
//
// The two rules of DESIGN section 2 decide the gathers: from the tiles a row is d / 4 separate 16-byte pieces, each in its own 64-byte
// sector (4x the useful bytes); from the row-major copy it is whole sectors.  A tile of which at least `lds_min` rows are wanted is read as
// it lies -- contiguous 1 KiB pieces -- and turned through LDS; below that the wanted rows' pieces are read directly.  (Where `lds_min`
// lies was measured, not derived: ivf_fetch.hip, kFetchLdsMin.)
#pragma once
#include "scan.hip.h"  // f32x4, lds_barrier
#include "fetch_plan.hpp"
#include "shard_where.hpp"
#include "update_plan.hpp"

namespace vers {

constexpr uint32_t kFetchNone = 0xFFFFFFFFu;  // row_of / a request's storage row: the id is in no list
constexpr uint32_t kFetchCols4 = 64;  // float4 columns per LDS pass, as the build's tile kernels: 64 rows x 65 float4 = 66.5 KB
// the call's counters (u64 each)
constexpr int kFtBad = 0, kFtFound = 1, kFtMissing = 2, kFtJobs = 3, kFtWords = 4;

__global__ void fetch_map_kernel(const MapJob* jobs, uint32_t n_jobs, const uint32_t* row_ids, uint64_t n_total, uint64_t id_lo, uint32_t* row_of) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)n_jobs * 64u) return;
  const MapJob jb = jobs[i >> 6];
  const uint32_t r = (uint32_t)(i & 63u);
  if (r < jb.first || r >= jb.end) return;
  const uint64_t row = (uint64_t)jb.tile * 64u + r;
  const uint32_t v = row_ids[row];
  if ((uint64_t)v < n_total && (uint64_t)v >= id_lo) row_of[v] = (uint32_t)row;
}

// src[i] = the storage row of ids[i] (kFetchNone: in no list, or out of range -- then the verdict is set too)
__global__ void fetch_check_kernel(const uint64_t* ids, uint64_t n, uint64_t n_total, const uint32_t* row_of, uint32_t* src, unsigned long long* misc) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false, found = false, missing = false;
  if (i < n) {
    const uint64_t v = ids[i];
    uint32_t r = kFetchNone;
    if (v >= n_total) bad = true;
    else r = row_of[v];
    found = r != kFetchNone;
    missing = !bad && !found;
    src[i] = r;
  }
  const unsigned long long nb = __popcll(__ballot(bad)), nf = __popcll(__ballot(found)), nm = __popcll(__ballot(missing));
  if ((threadIdx.x & 63u) == 0u) {
    if (nb) atomicAdd(misc + kFtBad, nb);
    if (nf) atomicAdd(misc + kFtFound, nf);
    if (nm) atomicAdd(misc + kFtMissing, nm);
  }
}

// ---- without the map: the requests as (vec id, request) pairs, sorted by id; every live row looks its id up ------------------------------
// keys[i] = the id's low word (an id out of range sets the verdict and sorts behind every id that can be stored), vals[i] = i, src[i] = none
__global__ void fetch_keys_kernel(const uint64_t* ids, uint64_t n, uint64_t n_total, uint32_t* keys, uint32_t* vals, uint32_t* src, unsigned long long* misc) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t v = ids[i];
  if (v >= n_total) atomicAdd(misc + kFtBad, 1ull);
  keys[i] = v >= n_total ? kFetchNone : (uint32_t)v;
  vals[i] = (uint32_t)i;
  src[i] = kFetchNone;
}
__global__ void fetch_locate_kernel(const MapJob* jobs, uint32_t n_jobs, const uint32_t* row_ids, uint64_t n_total, const uint32_t* skeys, const uint32_t* svals,
                                    uint64_t n, uint32_t* src) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)n_jobs * 64u) return;
  const MapJob jb = jobs[i >> 6];
  const uint32_t r = (uint32_t)(i & 63u);
  if (r < jb.first || r >= jb.end) return;
  const uint64_t row = (uint64_t)jb.tile * 64u + r;
  const uint32_t v = row_ids[row];
  if ((uint64_t)v >= n_total) return;
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (skeys[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  for (; lo < n && skeys[lo] == v; ++lo) src[svals[lo]] = (uint32_t)row;  // every occurrence of a repeated id
}
__global__ void fetch_count_kernel(const uint32_t* src, uint64_t n, unsigned long long* misc) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool found = i < n && src[i] != kFetchNone, missing = i < n && !found;
  const unsigned long long nf = __popcll(__ballot(found)), nm = __popcll(__ballot(missing));
  if ((threadIdx.x & 63u) == 0u) {
    if (nf) atomicAdd(misc + kFtFound, nf);
    if (nm) atomicAdd(misc + kFtMissing, nm);
  }
}

// out_clusters / out_status (each nullable) of requests [0, n): assignments[v] and 0, or UINT64_MAX and 2 for an id in no list
__global__ void fetch_meta_kernel(const uint32_t* src, uint64_t n, const uint32_t* list_off, uint32_t k, uint64_t* out_clusters, uint8_t* out_status) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = src[i];
  if (out_clusters) out_clusters[i] = r == kFetchNone ? 0xFFFFFFFFFFFFFFFFull : (uint64_t)upd::list_of_row(list_off, k, r);
  if (out_status) out_status[i] = r == kFetchNone ? upd::kSkipped : (uint8_t)0;
}

// ---- the gather from the row-major copy --------------------------------------------------------------------------------------------------
// One WAVE per requested row (four to a block): rows_rm row src[i] -- ld floats, whole sectors -- to out row i (pitch floats).  Lane j takes
// float4 j, j + 64, ...: contiguous 16-byte loads and stores (vec: out and pitch are 16-byte aligned); otherwise a float per lane.  Columns
// d .. pitch - 1 of the output, and the copy's padding columns d .. ld - 1, are never touched; an id in no list leaves as +0.0.
__global__ __launch_bounds__(256) void fetch_rows_rm_kernel(const float* rows_rm, uint32_t ld, uint32_t d, const uint32_t* src, uint64_t n, float* out, uint64_t pitch,
                                                            int vec) {
  const uint64_t i = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (i >= n) return;
  const uint32_t r = src[i];
  const float* in = rows_rm + (uint64_t)(r == kFetchNone ? 0u : r) * ld;
  float* o = out + i * pitch;
  if (vec) {
    const uint32_t d4 = d / 4u;
    for (uint32_t j = lane; j < d4; j += 64u) {
      f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
      if (r != kFetchNone) v = reinterpret_cast<const f32x4*>(in)[j];
      reinterpret_cast<f32x4*>(o)[j] = v;
    }
    const uint32_t c = d4 * 4u + lane;
    if (c < d) o[c] = r != kFetchNone ? in[c] : 0.0f;
  } else {
    for (uint32_t c = lane; c < d; c += 64u) o[c] = r != kFetchNone ? in[c] : 0.0f;
  }
}

// ---- the gather from the tiles: jobs -----------------------------------------------------------------------------------------------------
// The requests sorted by storage row (skeys ascending, svals = the request): position p starts a job when its tile differs from its
// predecessor's; a request for an id in no list is a job of its own (its row of zeros).  heads[p] = 1 / 0, heads[n] = 0 (the prefix's total).
__global__ void iota_u32_kernel(uint32_t* v, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = (uint32_t)i;
}
__global__ void fetch_heads_kernel(const uint32_t* skeys, uint64_t n, uint32_t* heads) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p > n) return;
  heads[p] = p < n && (p == 0 || skeys[p] == kFetchNone || (skeys[p] >> 6) != (skeys[p - 1] >> 6)) ? 1u : 0u;
}
__global__ void fetch_jobs_kernel(const uint32_t* heads, const uint64_t* base, uint64_t n, uint32_t* job_begin, unsigned long long* misc) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p > n) return;
  if (p == n) misc[kFtJobs] = base[n];
  else if (heads[p]) job_begin[base[p]] = (uint32_t)p;
}

// [fetch gather kernel: begin] (tests/test_fetch_kernel_host.py runs the text between the two markers on the host)
// One float4 of a requested row to its place: piece j4 of out row `req`.  Whole pieces inside d leave as one 16-byte store when the output
// allows it (vec); the piece that holds column d - 1 and an unaligned output leave float by float.  Columns >= d are never written.
__device__ inline void fetch_store_piece(float* out, uint64_t pitch, uint32_t req, uint32_t j4, f32x4 v, uint32_t d, int vec) {
  float* o = out + (uint64_t)req * pitch + (uint64_t)j4 * 4u;
  if (vec && j4 * 4u + 4u <= d) {
    *reinterpret_cast<f32x4*>(o) = v;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (j4 * 4u + (uint32_t)u < d) o[u] = v[u];
  }
}
// One BLOCK per job = per touched tile (job_begin[blockIdx.x] .. the next job's begin, or n_req): the requests skeys[p] (storage row) ->
// svals[p] (output row) of one tile, repeated ids included -- several output rows per stored row.  Three forms:
//   an id in no list     its output row's d floats as +0.0
//   >= lds_min requests  tiles_to_live_rows_kernel (ivf_build.hip) with a destination per REQUEST: the tile's 1 KiB pieces are read as they lie, kFetchCols4
//                        float4 columns at a time, and every requested row leaves LDS as contiguous float4s.  Rows nobody asked for -- slack
//                        among them, whatever it holds -- get as far as LDS and no further.
//   fewer                each requested row's 16-byte pieces are read where they lie (a 64-byte sector each) by consecutive threads, which
//                        store them contiguously
// Only the f32 tiles are read.  Dynamic LDS: [64][kFetchCols4 + 1] float4s.
__global__ __launch_bounds__(256) void fetch_tiles_kernel(const float* in, uint32_t ld, uint32_t d, const uint32_t* job_begin, uint32_t n_jobs, uint32_t n_req,
                                                          const uint32_t* skeys, const uint32_t* svals, uint32_t lds_min, float* out, uint64_t pitch, int vec) {
  extern __shared__ __attribute__((aligned(16))) f32x4 tl[];  // [64][kFetchCols4 + 1]
  constexpr uint32_t kPitch = kFetchCols4 + 1;
  const uint32_t begin = job_begin[blockIdx.x];
  const uint32_t end = blockIdx.x + 1u < n_jobs ? job_begin[blockIdx.x + 1u] : n_req;
  const uint32_t n_here = end - begin;
  const uint32_t d4 = (d + 3u) / 4u;
  const uint32_t row0 = skeys[begin];
  if (row0 == 0xFFFFFFFFu) {
    const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t i = threadIdx.x; i < n_here * d4; i += 256u) fetch_store_piece(out, pitch, svals[begin + i / d4], i % d4, z, d, vec);
    return;
  }
  const f32x4* tile = reinterpret_cast<const f32x4*>(in + (uint64_t)(row0 >> 6) * 64ull * ld);
  if (n_here < lds_min) {
    for (uint32_t i = threadIdx.x; i < n_here * d4; i += 256u) {  // a row's pieces by consecutive threads
      const uint32_t p = begin + i / d4, j = i % d4;
      fetch_store_piece(out, pitch, svals[p], j, tile[(uint64_t)j * 64 + (skeys[p] & 63u)], d, vec);
    }
    return;
  }
  for (uint32_t c0 = 0; c0 < d4; c0 += kFetchCols4) {
    const uint32_t nc = d4 - c0 < kFetchCols4 ? d4 - c0 : kFetchCols4;
    for (uint32_t i = threadIdx.x; i < 64u * nc; i += 256u) {  // a piece's 64 rows by consecutive threads: 1 KiB contiguous
      const uint32_t j = i / 64u, r = i % 64u;
      tl[r * kPitch + j] = tile[(uint64_t)(c0 + j) * 64 + r];
    }
    lds_barrier();
    for (uint32_t i = threadIdx.x; i < n_here * kFetchCols4; i += 256u) {  // a request's float4s by consecutive threads
      const uint32_t p = begin + i / kFetchCols4, j = i % kFetchCols4;
      if (j < nc) fetch_store_piece(out, pitch, svals[p], c0 + j, tl[(skeys[p] & 63u) * kPitch + j], d, vec);
    }
    lds_barrier();
  }
}
// [fetch gather kernel: end]

// ---- handles sharded by cluster: the "where" round and the row round (shard_where.hpp) ---------------------------------------------------
// words[i] = the list of storage row src[i] (by the CURRENT list_off, as fetch_meta_kernel), shw::kNoWord for an id this rank stores in no
// list: what the rank sends in the where round.  Only the call's exchange buffer is written.
__global__ void shard_where_kernel(const uint32_t* src, uint64_t n, const uint32_t* list_off, uint32_t k, uint32_t* words) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = src[i];
  words[i] = r == kFetchNone ? shw::kNoWord : upd::list_of_row(list_off, k, r);
}
// csrc[p] = src[req[p]]: the storage rows of the requests this rank found in one chunk, in request order -- the source list that drives the
// existing gathers (fetch_rows_rm_kernel / fetch_tiles_kernel) into the packed send buffer
__global__ void shard_pack_src_kernel(const uint32_t* src, const uint32_t* req, uint64_t m, uint32_t* csrc) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < m) csrc[p] = src[req[p]];
}
// out_clusters / out_status (each nullable) from the resolved table: cluster[i] = the list of request i on its owner, shw::kNoWord = in no list
__global__ void shard_meta_kernel(const uint32_t* cluster, uint64_t n, uint64_t* out_clusters, uint8_t* out_status) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = cluster[i];
  if (out_clusters) out_clusters[i] = c == shw::kNoWord ? 0xFFFFFFFFFFFFFFFFull : (uint64_t)c;
  if (out_status) out_status[i] = c == shw::kNoWord ? upd::kSkipped : (uint8_t)0;
}
// One WAVE per request of a chunk (four to a block), as fetch_rows_rm_kernel: request i0 + i takes row slot[i0 + i] of the gathered chunk
// (recv: [world][pad] rows at a pitch of exactly d floats) to out row i0 + i (pitch floats); a request in no list leaves as d zeros.  Whole
// 16-byte pieces when both sides allow it (vec: d, pitch and out are multiples of 16 bytes; recv is); otherwise a float per lane.  Columns
// d .. pitch - 1 are never written.
__global__ __launch_bounds__(256) void shard_place_rows_kernel(const float* recv, uint32_t d, const uint32_t* slot, uint64_t i0, uint64_t m, float* out, uint64_t pitch,
                                                               int vec) {
  const uint64_t il = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (il >= m) return;
  const uint64_t i = i0 + il;
  const uint32_t s = slot[i];
  const bool have = s != shw::kNoWord;
  const float* in = recv + (uint64_t)(have ? s : 0u) * d;
  float* o = out + i * pitch;
  if (vec) {
    for (uint32_t j = lane; j < d / 4u; j += 64u) {
      f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
      if (have) v = reinterpret_cast<const f32x4*>(in)[j];
      reinterpret_cast<f32x4*>(o)[j] = v;
    }
  } else {
    for (uint32_t c = lane; c < d; c += 64u) o[c] = have ? in[c] : 0.0f;
  }
}

// ---- search by stored id: VERS_BYID_EXCLUDE_SELF -----------------------------------------------------------------------------------------
// Row q of the search at top_k + 1 (ids / dist [b][top_k + 1], cnt [b]) without the entry whose id is self[q] -- or without its last entry
// when self[q] is not there -- in the same order: in the one global stable order of nprobe >= 1 that is the search on the index from which
// self[q] alone was removed.  out_count[q] = min(count, top_k); entries past it are written as zeros.
__global__ void byid_drop_self_kernel(const uint64_t* ids, const float* dist, const uint32_t* cnt, const uint64_t* self, uint32_t b, uint32_t top_k,
                                      uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= b) return;
  const uint32_t k1 = top_k + 1u;
  const uint32_t c = cnt[q] < k1 ? cnt[q] : k1;
  const uint64_t me = self[q];
  const uint64_t* qi = ids + (uint64_t)q * k1;
  const float* qd = dist + (uint64_t)q * k1;
  uint32_t w = 0;
  bool dropped = false;
  for (uint32_t i = 0; i < c && w < top_k; ++i) {
    if (!dropped && qi[i] == me) { dropped = true; continue; }
    out_ids[(uint64_t)q * top_k + w] = qi[i];
    out_dist[(uint64_t)q * top_k + w] = qd[i];
    ++w;
  }
  out_count[q] = w;
  for (; w < top_k; ++w) {
    out_ids[(uint64_t)q * top_k + w] = 0;
    out_dist[(uint64_t)q * top_k + w] = 0.0f;
  }
}

}  // namespace vers
