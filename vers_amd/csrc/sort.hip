// sort.hip -- stable grouping of row indices by cluster id (plumbing, not the hot path):
// ids sorted by (cluster, ascending row index) == the reference's inverted lists
// `ids[cluster].push(vec_id)` in ascending vec_id (ivfflat.rs:123-127).  Uses rocPRIM's
// LSD radix sort, which is stable.
// + the two rocPRIM steps of the range search (range.hip.h): the prefix over the per-slot hit counts and the per-query sort of
// (key, id) pairs -- of keys alone for the exhaustive range search.  rocPRIM is instantiated in this translation unit only.
#include <cstdlib>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "kmeans.hpp"

namespace vers {

__global__ void iota_kernel(uint32_t* v, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = i;
}

size_t group_by_cluster_temp_bytes(uint32_t n, uint32_t k) {
  size_t bytes = 0;
  unsigned bits = 1;
  while ((1ull << bits) < k) ++bits;
  (void)rocprim::radix_sort_pairs(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr,
                                  (uint32_t*)nullptr, (size_t)n, 0u, bits, (hipStream_t) nullptr);
  return bytes + 3ull * n * sizeof(uint32_t) + 256;
}

// assign[n] -> sorted_ids[n]; temp must hold group_by_cluster_temp_bytes(n, k).
int32_t group_by_cluster(const uint32_t* assign, uint32_t n, uint32_t k, uint32_t* sorted_ids, void* temp,
                         size_t temp_bytes, hipStream_t st) {
  if (n == 0) return VERS_OK;
  unsigned bits = 1;
  while ((1ull << bits) < k) ++bits;
  uint32_t* iota = (uint32_t*)temp;
  uint32_t* keys_out = iota + n;
  char* rp_tmp = (char*)(keys_out + n);
  rp_tmp = (char*)(((uintptr_t)rp_tmp + 255) & ~(uintptr_t)255);
  size_t rp_bytes = temp_bytes - (size_t)(rp_tmp - (char*)temp);
  hipLaunchKernelGGL(iota_kernel, dim3((n + 255) / 256), dim3(256), 0, st, iota, n);
  VERS_HIP_TRY(hipGetLastError());
  VERS_HIP_TRY(rocprim::radix_sort_pairs((void*)rp_tmp, rp_bytes, assign, keys_out, (const uint32_t*)iota, sorted_ids,
                                         (size_t)n, 0u, bits, st));
  return VERS_OK;
}

// ---- range search: counts -> offsets, per-query sort ---------------------------------------------------------------
// base[i] = counts[0] + ... + counts[i - 1] as u64, i in [0, n): the caller appends a zero count so that base[n - 1] is the total
size_t range_scan_temp_bytes(size_t n) {
  size_t bytes = 0;
  (void)rocprim::exclusive_scan(nullptr, bytes, (const uint32_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, n, rocprim::plus<uint64_t>(), (hipStream_t) nullptr);
  return bytes + 256;
}
int32_t range_scan_counts(const uint32_t* counts, uint64_t* base, size_t n, void* temp, size_t temp_bytes, hipStream_t st) {
  if (n == 0) return VERS_OK;
  VERS_HIP_TRY(rocprim::exclusive_scan(temp, temp_bytes, counts, base, (uint64_t)0, n, rocprim::plus<uint64_t>(), st));
  return VERS_OK;
}
// segment s = [lims[s], lims[s + 1]) of (keys_in, ids_in) sorted ascending by the whole 64-bit key into (keys_out, ids_out); n < 2^32
size_t range_sort_temp_bytes(uint32_t n, uint32_t segments) {
  size_t bytes = 0;
  (void)rocprim::segmented_radix_sort_pairs(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint64_t*)nullptr, (uint64_t*)nullptr, n, segments,
                                            (const uint64_t*)nullptr, (const uint64_t*)nullptr, 0u, 64u, (hipStream_t) nullptr);
  return bytes + 256;
}
int32_t range_sort_segments(const uint64_t* keys_in, uint64_t* keys_out, const uint64_t* ids_in, uint64_t* ids_out, uint32_t n, uint32_t segments,
                            const uint64_t* lims, void* temp, size_t temp_bytes, hipStream_t st) {
  if (n == 0 || segments == 0) return VERS_OK;
  VERS_HIP_TRY(rocprim::segmented_radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, ids_in, ids_out, n, segments, lims, lims + 1, 0u, 64u, st));
  return VERS_OK;
}
// the same for keys alone (exhaustive range search: the key's low word IS the id)
size_t range_sort_keys_temp_bytes(uint32_t n, uint32_t segments) {
  size_t bytes = 0;
  (void)rocprim::segmented_radix_sort_keys(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, n, segments, (const uint64_t*)nullptr,
                                           (const uint64_t*)nullptr, 0u, 64u, (hipStream_t) nullptr);
  return bytes + 256;
}
int32_t range_sort_segment_keys(const uint64_t* keys_in, uint64_t* keys_out, uint32_t n, uint32_t segments, const uint64_t* lims, void* temp,
                                size_t temp_bytes, hipStream_t st) {
  if (n == 0 || segments == 0) return VERS_OK;
  VERS_HIP_TRY(rocprim::segmented_radix_sort_keys(temp, temp_bytes, keys_in, keys_out, n, segments, lims, lims + 1, 0u, 64u, st));
  return VERS_OK;
}

// ---- vers_ivf_fetch: the requests ordered by storage row (or, without the id map, by vec id) -----------------------------------------
size_t fetch_sort_temp_bytes(size_t n) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_pairs(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, n, 0u, 32u,
                                  (hipStream_t) nullptr);
  return bytes + 256;
}
int32_t fetch_sort_pairs(const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out, size_t n, void* temp, size_t temp_bytes,
                         hipStream_t st) {
  if (n == 0) return VERS_OK;
  VERS_HIP_TRY(rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, 0u, 32u, st));
  return VERS_OK;
}

}  // namespace vers
