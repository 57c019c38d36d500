// range_driver.hip.h -- the two-phase protocol of every range search (range.hip.h): count pass, prefix scan and CSR limits, ONE synchronisation
// for total / status / NaN radius, fill pass, segmented sort, decode, synchronisation -- over whichever source supplies the items: the probed
// lists or the stored rows of the index (ivf_search.hip), the flat corpus (flat.hip).
#pragma once
#include <cstring>
#include <functional>
#include <string>
#include <type_traits>

#include "range.hip.h"
#include "range_scratch.hpp"
#include "scan_launch.hip.h"

namespace vers {

// A range call that ends in (key, id) pairs instead of (id, distance) -- a rank's PARTIAL of a sharded range search: the same count pass,
// prefix scan and fill pass over the lists (rows) this handle stores, the keys always staged, the segmented sort without the decode.
struct RangePartial {
  uint64_t* keys = nullptr;  // where the keys go, beside ids_dev
  // The sharded call, between the count and the fill: told the local total, it agrees with the peers (exchange 1), names where keys and ids
  // go and may call the fill off (go = false).  Without it: the cap protocol of the unsharded calls, on the local total.
  std::function<int32_t(uint64_t local_total, uint64_t*& keys, uint64_t*& ids, bool& go)> decide;
};

// one pass (FILL = false: count, true: fill) of the range walk over the items of `src`; not timed by the scan-timing ring
template <int QG, bool FILL, class Src>
inline int32_t launch_range_pass(int n_cu, uint32_t ld, int metric, const Src& src, uint32_t items, const RangeParams& p, hipStream_t st) {
  return with_metric(metric, [&](auto m) -> int32_t {
    return launch_scan(range_scan_kernel<QG, decltype(m)::value, FILL, Src>, scan_grid(n_cu, QG, ld, items), kWavesPerBlock, scan_lds_bytes(QG, ld), st, src, p);
  });
}

// Range search of b >= 1 queries on `st`.  own_out: ids / distances go to buffers of the source's, sized by the total (the host-pointer call
// copies them out), else to ids_dev / dist_dev -- when total <= cap (too small a buffer: the limits are complete, ids / distances untouched).
// part: (key, id) pairs instead; dist_dev is not used.  What a Source supplies:
//   static constexpr bool kKeyIds    the sort key's low word is the vec id (stored rows, flat corpus): keys alone are sorted and decode to
//                                    (id, distance); else (probed lists) it is the walk's sequence number and the ids travel beside the keys
//   static constexpr bool kPartials  the source serves partials; with kKeyIds it then has launch_key_ids(keys, n, ids, st): a partial's ids out of
//                                    its sorted keys (range_merge.hip.h's kernel, which only a handle that shards includes)
//   const char* who                  the entry point's name in error strings
//   int32_t prepare(st, &slots_per_query)   plan, or stage the queries and cut the segments; refuses a batch whose slots do not fit 32 bits;
//                                    whatever it queues is counted as the first phase
//   uint32_t ld() / uint32_t* status() / const uint32_t* row_ids()
//   int32_t launch(fill_tag, const RangeParams&, st)   one pass over its items
//   int32_t status_rc(word)          the status word the count pass left -> a return code
//   bool walk_order(flags, partial)  does the result stay in walk order
//   int32_t own_out(total, ids&, dist&)   its buffers for a host-pointer call's result
template <class Source>
int32_t range_search_run(Source& src, RangeScratch& R, uint32_t b, const float* radius_dev, uint32_t flags, uint64_t* lims_dev, uint64_t* ids_dev, float* dist_dev,
                         uint64_t cap, bool own_out, uint64_t* out_total, hipStream_t st, RangePartial* part = nullptr) {
  const std::string who = src.who;
  for (auto& e : R.ev)
    if (!e) VERS_HIP_TRY(hipEventCreate(&e));
  VERS_HIP_TRY(hipEventRecord(R.ev[0], st));
  uint64_t per_q = 0;
  if (int32_t rc = src.prepare(st, per_q)) return rc;
  const uint64_t n_slots = (uint64_t)b * per_q;
  const size_t scan_tmp = range_scan_temp_bytes((size_t)n_slots + 1);
  if (int32_t rc = R.counts.reserve(((size_t)n_slots + 1) * sizeof(uint32_t))) return rc;
  if (int32_t rc = R.base.reserve(((size_t)n_slots + 1) * sizeof(uint64_t))) return rc;
  if (int32_t rc = R.misc.reserve(16)) return rc;
  if (int32_t rc = R.tmp.reserve(scan_tmp)) return rc;
  VERS_HIP_TRY(hipMemsetAsync(R.counts.p, 0, ((size_t)n_slots + 1) * sizeof(uint32_t), st));  // (+ one zero count: the prefix's last entry is the total)
  VERS_HIP_TRY(hipMemsetAsync(R.misc.p, 0, 16, st));
  RangeParams rp;
  rp.ld = src.ld(); rp.n_chunks = src.ld() / kChunk; rp.status = src.status(); rp.radius = radius_dev; rp.counts = R.counts.as<uint32_t>();
  rp.base = R.base.as<uint64_t>(); rp.row_ids = src.row_ids(); rp.out_keys = nullptr; rp.out_ids = nullptr; rp.out_dist = nullptr; rp.next_quad = nullptr;
  VERS_HIP_TRY(hipEventRecord(R.ev[1], st));
  if (int32_t rc = src.launch(std::false_type{}, rp, st)) return rc;
  VERS_HIP_TRY(hipEventRecord(R.ev[2], st));
  if (int32_t rc = range_scan_counts(rp.counts, R.base.as<uint64_t>(), (size_t)n_slots + 1, R.tmp.p, scan_tmp, st)) return rc;
  hipLaunchKernelGGL(range_lims_kernel, dim3((b + 1 + 255) / 256), dim3(256), 0, st, rp.base, per_q, b, radius_dev, (const uint32_t*)rp.status, lims_dev,
                     R.misc.as<uint32_t>());
  VERS_HIP_TRY(hipGetLastError());
  if (!R.pin) VERS_HIP_TRY(hipHostMalloc((void**)&R.pin, 16, hipHostMallocDefault));  // pinned landing words: total | status | NaN radius
  VERS_HIP_TRY(hipMemcpyAsync(R.pin, R.misc.p, 16, hipMemcpyDeviceToHost, st));
  VERS_HIP_TRY(hipEventRecord(R.ev[3], st));
  VERS_HIP_TRY(hipStreamSynchronize(st));
  uint32_t misc[4];
  std::memcpy(misc, R.pin, sizeof(misc));
  if (int32_t rc = src.status_rc(misc[2])) return rc;
  if (misc[3]) return fail(VERS_ERR_INVALID, who + ": NaN radius");
  const uint64_t total = ((uint64_t)misc[1] << 32) | misc[0];
  if (total > 0xFFFFFFFFull) return fail(VERS_ERR_INVALID, who + ": more than 2^32 - 1 results in one call; split the batch");
  *out_total = total;
  float ms[5] = {};
  auto phases = [&](int n_ev) {
    for (int i = 0; i + 1 < n_ev; ++i) (void)hipEventElapsedTime(&ms[i], R.ev[i], R.ev[i + 1]);
    range_phases_add(b, total, ms);
  };
  bool go = total != 0 && total <= cap;
  if (part && part->decide)
    if (int32_t rc = part->decide(total, part->keys, ids_dev, go)) return rc;
  if (!go) { phases(4); return VERS_OK; }
  if (own_out)
    if (int32_t rc = src.own_out(total, ids_dev, dist_dev)) return rc;
  const bool walk = src.walk_order(flags, part != nullptr);
  // staging of the sorted order: keys in | keys out (a partial's sorted keys are its result: they go to its array) | ids in unless the keys
  // carry them, + rocPRIM's temporary
  size_t sort_tmp = 0;
  uint64_t *k_in = nullptr, *k_out = nullptr, *i_in = nullptr;
  if (!walk) {
    if constexpr (Source::kKeyIds) sort_tmp = range_sort_keys_temp_bytes((uint32_t)total, b);
    else sort_tmp = range_sort_temp_bytes((uint32_t)total, b);
    if (int32_t rc = R.stage.reserve((Source::kKeyIds || part ? 2 : 3) * (size_t)total * sizeof(uint64_t))) return rc;
    if (int32_t rc = R.tmp.reserve(sort_tmp)) return rc;
    k_in = R.stage.as<uint64_t>(); k_out = part ? part->keys : k_in + total;
    if constexpr (!Source::kKeyIds) i_in = k_in + (part ? 1 : 2) * total;
  }
  if constexpr (Source::kKeyIds) {
    rp.out_keys = k_in; rp.out_ids = walk ? ids_dev : nullptr; rp.out_dist = walk ? dist_dev : nullptr;
  } else if (part) {  // (a key beside every id, in walk order too)
    rp.out_keys = walk ? part->keys : k_in; rp.out_ids = walk ? ids_dev : i_in; rp.out_dist = nullptr;
  } else {
    rp.out_keys = k_in; rp.out_ids = walk ? ids_dev : i_in; rp.out_dist = dist_dev;
  }
  if (int32_t rc = src.launch(std::true_type{}, rp, st)) return rc;
  VERS_HIP_TRY(hipEventRecord(R.ev[4], st));
  if (!walk) {
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if constexpr (Source::kKeyIds) {
      if (int32_t rc = range_sort_segment_keys(k_in, k_out, (uint32_t)total, b, lims_dev, R.tmp.p, sort_tmp, st)) return rc;
      if constexpr (Source::kPartials) {
        if (part) src.launch_key_ids(k_out, total, ids_dev, st);
      }
      if (!part) hipLaunchKernelGGL(range_decode_ids_kernel, dim3(blocks), dim3(256), 0, st, (const uint64_t*)k_out, total, ids_dev, dist_dev);
    } else {
      if (int32_t rc = range_sort_segments(k_in, k_out, i_in, ids_dev, (uint32_t)total, b, lims_dev, R.tmp.p, sort_tmp, st)) return rc;
      if (!part) hipLaunchKernelGGL(range_decode_kernel, dim3(blocks), dim3(256), 0, st, (const uint64_t*)k_out, total, dist_dev);
    }
    VERS_HIP_TRY(hipGetLastError());
  }
  VERS_HIP_TRY(hipEventRecord(R.ev[5], st));
  VERS_HIP_TRY(hipStreamSynchronize(st));
  phases(6);
  return VERS_OK;
}

}  // namespace vers
