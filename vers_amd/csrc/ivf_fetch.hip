// ivf_fetch.hip -- reading the index back by vec id: vers_ivf_fetch / _fetch_dev (the stored vector, its list and whether it is still there)
// and vers_ivf_search_by_id / _dev (a search whose queries are stored vectors, optionally without the query's own id in the answer).
// Specification: include/vers_hip.h.  Kernels: fetch.hip.h.  The map's refresh rule and its jobs: fetch_plan.hpp.
//
// A call is two halves around ONE read-back:
//   locate   the vec id -> storage row map brought up to date (or, without it, the per-call table), the storage row of every request into
//            the leased workspace, the verdict and the counts -- and, where the rows come from the tiles, the requests sorted by storage
//            row and cut into one job per touched tile.  Everything so far wrote the workspace only.
//   deliver  after the host has read the verdict: clusters and status, and the gather.
// The calls take the handle the way searches do (shared; the mutators exclude them) and lease a workspace like them.
//
// On a handle sharded by cluster (vers_ivf_fetch_sharded_dev, vers_ivf_search_by_id_sharded_dev) the halves are the same with two exchanges
// between them: locate finds what THIS rank stores, the where round (shard_where.hpp) tells every rank each request's owner and list, and
// the row round carries the found rows, packed by the same two gathers, to every rank.
#include <chrono>

#include "ivf_handle.hpp"
#include "fetch.hip.h"

namespace vers {
namespace ivf {

// The smallest number of requests for one tile at which the gather turns the whole tile through LDS instead of reading the wanted rows'
// pieces directly (option "fetch_lds_min"; 1 = always LDS, 65 or more = never).  By bytes alone the forms would meet at 16 -- 64 rows of
// whole sectors against n rows at 4x their useful bytes -- but the wanted rows of one tile share their sectors through the L2, and MEASURED
// (profiles/r21_fetch.txt) the direct form wins at 1 .. 32 rows per tile at d = 128 and d = 768; at 64 the LDS form
// wins at d = 128 (0.72 against 0.74 ms per 15,132 tiles) and loses at d = 768 (0.48 against 0.42 ms per 2,998 tiles), where a row takes
// three LDS passes with two barriers each.  So: the whole tile wanted, and a row that fits one pass.
constexpr uint32_t kFetchLdsMin = 64;
inline uint32_t fetch_lds_min(uint32_t d) {
  const int64_t dflt = (d + 3u) / 4u <= kFetchCols4 ? (int64_t)kFetchLdsMin : 65;
  return (uint32_t)std::max<int64_t>(1, std::min<int64_t>(opt_get("fetch_lds_min", dflt), 0x7FFFFFFF));
}

constexpr int kFetchPhases = 8;
static std::mutex g_ft_mu;
static double g_ft[kFetchPhases] = {};  // vers_fetch_phases: calls, ids, found, staging, map, check + gather, copy out, inside a sharded call's callbacks (ms)

namespace {
struct PhaseClock {  // host wall clock of one phase of one call, the call's stream synchronised at its end
  double* acc;
  hipStream_t st;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  PhaseClock(double* a, hipStream_t s) : acc(a), st(s) {}
  int32_t done() {
    VERS_HIP_TRY(hipStreamSynchronize(st));
    *acc += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return VERS_OK;
  }
};
void phases_commit(const double* ph) {  // a call that succeeded (a refused call counts nowhere)
  std::lock_guard<std::mutex> lk(g_ft_mu);
  for (int i = 0; i < kFetchPhases; ++i) g_ft[i] += ph[i];
}
inline unsigned blocks_for(uint64_t n) { return (unsigned)((n + 255) / 256); }
// the owner table of a handle sharded by cluster (h_len holds GLOBAL lengths, h_off only the owned lists' offsets: the map's passes cover the
// owned lists alone, and row_of holds 0xFFFFFFFF for ids stored elsewhere); nullptr: every list is this handle's
inline const uint8_t* owned(const vers_ivf* h) { return h->world > 1 ? h->h_owner.data() : nullptr; }

int32_t upload_jobs(const std::vector<MapJob>& jobs, DevBuf& buf, hipStream_t st) {
  if (int32_t rc = buf.reserve(std::max<size_t>(1, jobs.size()) * sizeof(MapJob))) return rc;
  if (!jobs.empty()) VERS_HIP_TRY(hipMemcpyAsync(buf.p, jobs.data(), jobs.size() * sizeof(MapJob), hipMemcpyHostToDevice, st));
  return VERS_OK;
}

// The handle's map, up to date, or *out = nullptr: option "fetch_map" = 0 (A/B runs and the tests of the per-call table) or no room for it --
// it is optional memory.  Runs under the map's mutex; a refresh has finished on the device when this returns.
int32_t map_sync(vers_ivf* h, hipStream_t st, const uint32_t** out, double* ms) {
  vers_ivf::FetchMap& fm = h->fm;
  *out = nullptr;
  if (opt_get("fetch_map", 1) == 0) return VERS_OK;
  std::lock_guard<std::mutex> lk(fm.mu);
  MapRefresh how = fetch_map_decide(fm.built, fm.seen_moved, fm.seen_appended, h->flt_moved, h->flt_appended);
  if (how == MapRefresh::kAppended && (fm.snap_len.size() != h->k || fm.snap_n_total > h->n_total)) how = MapRefresh::kFull;
  if (how == MapRefresh::kNone) {
    fm.hits += 1;
    *out = fm.row_of.as<uint32_t>();
    return VERS_OK;
  }
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t n_total = h->n_total;
  if (n_total > fm.cap_ids || !fm.row_of.p) {
    const uint64_t cap = n_total + n_total / 8 + 1024;  // (room for the ids of later appends)
    DevBuf nb;
    if (nb.reserve((size_t)cap * sizeof(uint32_t)) != VERS_OK) {
      (void)hipGetLastError();
      fm.row_of.release();
      fm.cap_ids = 0;
      fm.built = false;
      return VERS_OK;  // the per-call table serves this call
    }
    if (how == MapRefresh::kAppended) {
      VERS_HIP_TRY(hipMemcpyAsync(nb.p, fm.row_of.p, (size_t)fm.snap_n_total * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
      VERS_HIP_TRY(hipStreamSynchronize(st));
    }
    std::swap(fm.row_of.p, nb.p);
    std::swap(fm.row_of.cap, nb.cap);
    fm.cap_ids = cap;
  }
  std::vector<MapJob> jobs;
  uint64_t id_lo = 0;
  if (how == MapRefresh::kFull) {
    fetch_map_plan(nullptr, h->h_len.data(), h->h_off.data(), owned(h), h->rank, h->k, jobs);
    if (n_total) VERS_HIP_TRY(hipMemsetAsync(fm.row_of.p, 0xFF, (size_t)n_total * sizeof(uint32_t), st));
    fm.builds += 1;
  } else {
    id_lo = fm.snap_n_total;
    fetch_map_plan(fm.snap_len.data(), h->h_len.data(), h->h_off.data(), owned(h), h->rank, h->k, jobs);
    if (n_total > id_lo) VERS_HIP_TRY(hipMemsetAsync(fm.row_of.as<uint32_t>() + id_lo, 0xFF, (size_t)(n_total - id_lo) * sizeof(uint32_t), st));
    fm.tails += 1;
  }
  fm.built = false;  // (until the pass below has run)
  for (const MapJob& j : jobs)
    if ((uint64_t)j.tile * 64u + j.end > h->cap_rows) return fail(VERS_ERR_HIP, "vers_ivf_fetch: a list lies outside its storage (inconsistent index)");
  if (int32_t rc = upload_jobs(jobs, fm.jobs, st)) return rc;
  if (!jobs.empty()) {
    hipLaunchKernelGGL(fetch_map_kernel, dim3(blocks_for(jobs.size() * 64)), dim3(256), 0, st, (const MapJob*)fm.jobs.as<MapJob>(), (uint32_t)jobs.size(),
                       (const uint32_t*)h->row_ids.as<uint32_t>(), n_total, id_lo, fm.row_of.as<uint32_t>());
    VERS_HIP_TRY(hipGetLastError());
  }
  VERS_HIP_TRY(hipStreamSynchronize(st));  // (the jobs' host copy, and other streams' fetches, which start behind this mutex)
  fm.built = true;
  fm.seen_moved = h->flt_moved;
  fm.seen_appended = h->flt_appended;
  fm.snap_n_total = n_total;
  fm.snap_len = h->h_len;
  *out = fm.row_of.as<uint32_t>();
  *ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return VERS_OK;
}

struct Located {
  uint64_t bad = 0, found = 0, missing = 0, n_jobs = 0;
  bool tiles = false;  // the requests are sorted and cut into tile jobs (W->ft_pairs, W->ft_jobs)
};

// The tile gather's plan: the (storage row, request) pairs of src [n] in storage order (W->ft_pairs' two last quarters), a job per touched
// tile (W->ft_jobs), the job count into misc[kFtJobs].  Queued on `st`.
int32_t tile_jobs(const uint32_t* src, uint64_t n, unsigned long long* misc, hipStream_t st) {
  const size_t sort_tmp = fetch_sort_temp_bytes((size_t)n);
  if (int32_t rc = W->ft_pairs.reserve((size_t)n * 4 * sizeof(uint32_t))) return rc;
  if (int32_t rc = W->ft_tmp.reserve(std::max(sort_tmp, range_scan_temp_bytes((size_t)n + 1)))) return rc;
  if (int32_t rc = W->ft_heads.reserve(((size_t)n + 1) * sizeof(uint32_t))) return rc;
  if (int32_t rc = W->ft_base.reserve(((size_t)n + 1) * sizeof(uint64_t))) return rc;
  if (int32_t rc = W->ft_jobs.reserve((size_t)n * sizeof(uint32_t))) return rc;
  uint32_t *vin = W->ft_pairs.as<uint32_t>() + n, *kout = vin + n, *vout = kout + n;
  hipLaunchKernelGGL(iota_u32_kernel, dim3(blocks_for(n)), dim3(256), 0, st, vin, n);
  VERS_HIP_TRY(hipGetLastError());
  if (int32_t rc = fetch_sort_pairs(src, kout, vin, vout, (size_t)n, W->ft_tmp.p, sort_tmp, st)) return rc;
  hipLaunchKernelGGL(fetch_heads_kernel, dim3(blocks_for(n + 1)), dim3(256), 0, st, (const uint32_t*)kout, n, W->ft_heads.as<uint32_t>());
  VERS_HIP_TRY(hipGetLastError());
  if (int32_t rc = range_scan_counts(W->ft_heads.as<uint32_t>(), W->ft_base.as<uint64_t>(), (size_t)n + 1, W->ft_tmp.p, W->ft_tmp.cap, st)) return rc;
  hipLaunchKernelGGL(fetch_jobs_kernel, dim3(blocks_for(n + 1)), dim3(256), 0, st, (const uint32_t*)W->ft_heads.as<uint32_t>(),
                     (const uint64_t*)W->ft_base.as<uint64_t>(), n, W->ft_jobs.as<uint32_t>(), misc);
  VERS_HIP_TRY(hipGetLastError());
  return VERS_OK;
}

// The first half of a call: ids_dev [n] -> W->ft_src, the counters, and with `want_rows` on a handle without a row-major copy the tile jobs.
// Waits for `st` once, for the counters.  n < 2^32.
int32_t locate(vers_ivf* h, const uint64_t* ids_dev, uint64_t n, bool want_rows, hipStream_t st, Located& L, double* ph) {
  const uint32_t* row_of = nullptr;
  if (int32_t rc = map_sync(h, st, &row_of, &ph[4])) return rc;
  PhaseClock clk(&ph[5], st);
  const uint64_t n_total = h->n_total;
  L.tiles = want_rows && h->rows_rm.p == nullptr;
  if (int32_t rc = W->ft_src.reserve((size_t)n * sizeof(uint32_t))) return rc;
  if (int32_t rc = W->ft_misc.reserve(kFtWords * sizeof(uint64_t))) return rc;
  VERS_HIP_TRY(hipMemsetAsync(W->ft_misc.p, 0, kFtWords * sizeof(uint64_t), st));
  unsigned long long* misc = W->ft_misc.as<unsigned long long>();
  uint32_t* src = W->ft_src.as<uint32_t>();
  uint32_t *kin = nullptr, *vin = nullptr, *kout = nullptr, *vout = nullptr;
  size_t sort_tmp = 0;
  if (L.tiles || row_of == nullptr) {
    sort_tmp = fetch_sort_temp_bytes((size_t)n);
    if (int32_t rc = W->ft_pairs.reserve((size_t)n * 4 * sizeof(uint32_t))) return rc;
    if (int32_t rc = W->ft_tmp.reserve(std::max(sort_tmp, range_scan_temp_bytes((size_t)n + 1)))) return rc;
    kin = W->ft_pairs.as<uint32_t>(); vin = kin + n; kout = vin + n; vout = kout + n;
  }
  if (row_of != nullptr) {
    hipLaunchKernelGGL(fetch_check_kernel, dim3(blocks_for(n)), dim3(256), 0, st, ids_dev, n, n_total, row_of, src, misc);
    VERS_HIP_TRY(hipGetLastError());
  } else {  // the per-call table: the requests sorted by vec id, one pass over the live rows
    std::vector<MapJob> jobs;
    fetch_map_plan(nullptr, h->h_len.data(), h->h_off.data(), owned(h), h->rank, h->k, jobs);
    for (const MapJob& j : jobs)
      if ((uint64_t)j.tile * 64u + j.end > h->cap_rows) return fail(VERS_ERR_HIP, "vers_ivf_fetch: a list lies outside its storage (inconsistent index)");
    DevBuf djobs;
    if (int32_t rc = upload_jobs(jobs, djobs, st)) return rc;
    hipLaunchKernelGGL(fetch_keys_kernel, dim3(blocks_for(n)), dim3(256), 0, st, ids_dev, n, n_total, kin, vin, src, misc);
    VERS_HIP_TRY(hipGetLastError());
    if (int32_t rc = fetch_sort_pairs(kin, kout, vin, vout, (size_t)n, W->ft_tmp.p, sort_tmp, st)) return rc;
    if (!jobs.empty()) {
      hipLaunchKernelGGL(fetch_locate_kernel, dim3(blocks_for(jobs.size() * 64)), dim3(256), 0, st, (const MapJob*)djobs.as<MapJob>(), (uint32_t)jobs.size(),
                         (const uint32_t*)h->row_ids.as<uint32_t>(), n_total, (const uint32_t*)kout, (const uint32_t*)vout, n, src);
    }
    hipLaunchKernelGGL(fetch_count_kernel, dim3(blocks_for(n)), dim3(256), 0, st, (const uint32_t*)src, n, misc);
    VERS_HIP_TRY(hipGetLastError());
    VERS_HIP_TRY(hipStreamSynchronize(st));  // (djobs and the host's jobs leave scope)
  }
  if (L.tiles)
    if (int32_t rc = tile_jobs(src, n, misc, st)) return rc;
  uint64_t words[kFtWords] = {};
  VERS_HIP_TRY(hipMemcpyAsync(words, misc, sizeof(words), hipMemcpyDeviceToHost, st));
  if (int32_t rc = clk.done()) return rc;
  L.bad = words[kFtBad]; L.found = words[kFtFound]; L.missing = words[kFtMissing]; L.n_jobs = words[kFtJobs];
  return VERS_OK;
}

// The gather proper: the stored rows src [n] to out rows 0 .. n - 1 -- from the row-major copy, or (tiles: tile_jobs has run over src, n_jobs
// of them) from the f32 tiles.
int32_t gather_rows(vers_ivf* h, const uint32_t* src, uint64_t n, bool tiles, uint64_t n_jobs, float* out_rows, uint64_t pitch, hipStream_t st) {
  const int vec = ((uintptr_t)out_rows % 16u == 0 && pitch % 4u == 0) ? 1 : 0;
  if (!tiles) {
    if ((n + 3) / 4 > 0x7FFFFFFFull) return fail(VERS_ERR_INVALID, "vers_ivf_fetch: too many ids for one call");
    hipLaunchKernelGGL(fetch_rows_rm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, (const float*)h->rows_rm.as<float>(), h->ld, h->d, src, n, out_rows, pitch,
                       vec);
  } else {
    if (n_jobs == 0 || n_jobs > 0x7FFFFFFFull) return fail(VERS_ERR_HIP, "vers_ivf_fetch: the tile jobs do not match the requests");
    const size_t lds = 64 * (size_t)(kFetchCols4 + 1) * sizeof(f32x4);
    if (int32_t rc = scan_prepare_launch(fetch_tiles_kernel, lds)) return rc;
    const uint32_t lds_min = fetch_lds_min(h->d);
    const uint32_t* pairs = W->ft_pairs.as<uint32_t>();
    hipLaunchKernelGGL(fetch_tiles_kernel, dim3((unsigned)n_jobs), dim3(256), lds, st, (const float*)h->rows.as<float>(), h->ld, h->d,
                       (const uint32_t*)W->ft_jobs.as<uint32_t>(), (uint32_t)n_jobs, (uint32_t)n, pairs + 2 * n, pairs + 3 * n, lds_min, out_rows, pitch, vec);
  }
  VERS_HIP_TRY(hipGetLastError());
  return VERS_OK;
}

// The second half: clusters / status (each nullable) and the rows (nullable) of the n located requests, queued on `st`.
int32_t deliver(vers_ivf* h, uint64_t n, const Located& L, float* out_rows, uint64_t pitch, uint64_t* out_clusters, uint8_t* out_status, hipStream_t st) {
  const uint32_t* src = W->ft_src.as<uint32_t>();
  if (out_clusters != nullptr || out_status != nullptr) {
    hipLaunchKernelGGL(fetch_meta_kernel, dim3(blocks_for(n)), dim3(256), 0, st, src, n, (const uint32_t*)h->list_off.as<uint32_t>(), h->k, out_clusters, out_status);
    VERS_HIP_TRY(hipGetLastError());
  }
  if (out_rows == nullptr) return VERS_OK;
  return gather_rows(h, src, n, L.tiles, L.n_jobs, out_rows, pitch, st);
}

// what a fetch refuses from the locked handle
int32_t fetch_check_handle(vers_ivf* h, const char* who, bool shards = false) {
  if (h->world > 1 && !shards) return fail(VERS_ERR_INVALID, std::string(who) + ": the handle is sharded by cluster (whether an id is live is known to its owner alone)");
  if (h->up.open) return fail(VERS_ERR_EMPTY, std::string(who) + " while a streamed upload is in progress: the handle holds no index until vers_ivf_upload_end");
  if (h->k == 0) return fail(VERS_ERR_EMPTY, std::string(who) + ": the handle holds no centroids");
  return VERS_OK;
}
}  // namespace

// ---- search by stored id -------------------------------------------------------------------------------------------------------------
// ids_dev [b] on the device.  The id check (one read-back), the queries fetched into W->ft_q at the query pitch, then the search itself --
// for VERS_BYID_EXCLUDE_SELF at top_k + 1 into W->ft_res with byid_drop_self_kernel behind it.  `search` runs search_dev_locked (the host
// call wraps it in the reference mode's retries).
template <class Search>
static int32_t by_id_locked(vers_ivf* h, const char* who, const uint64_t* ids_dev, uint32_t b, uint32_t top_k, uint32_t flags, uint64_t* out_ids, float* out_dist,
                            uint32_t* out_count, hipStream_t st, Search&& search) {
  double ph[kFetchPhases] = {};
  Located L;
  if (int32_t rc = locate(h, ids_dev, b, true, st, L, ph)) return rc;
  if (L.bad) return fail(VERS_ERR_INVALID, std::string(who) + ": a vec id at or beyond n of vers_ivf_info; nothing was written");
  if (L.missing) return fail(VERS_ERR_INVALID, std::string(who) + ": a vec id that is in no list (vers_ivf_fetch tells which); nothing was written");
  if (top_k == 0) {
    VERS_HIP_TRY(hipMemsetAsync(out_count, 0, sizeof(uint32_t) * b, st));
    return VERS_OK;
  }
  const size_t q_bytes = (size_t)b * h->ldq * sizeof(float);
  if (int32_t rc = W->ft_q.reserve(q_bytes)) return rc;
  VERS_HIP_TRY(hipMemsetAsync(W->ft_q.p, 0, q_bytes, st));  // (the padding columns of a query block are zeros)
  if (int32_t rc = deliver(h, b, L, W->ft_q.as<float>(), h->ldq, nullptr, nullptr, st)) return rc;
  if (!(flags & VERS_BYID_EXCLUDE_SELF)) return search(W->ft_q.as<float>(), top_k, out_ids, out_dist, out_count);
  const uint32_t k1 = top_k + 1u;
  const size_t ids_b = (size_t)b * k1 * sizeof(uint64_t), dist_b = (((size_t)b * k1 * sizeof(float)) + 7) & ~(size_t)7;
  if (int32_t rc = W->ft_res.reserve(ids_b + dist_b + (size_t)b * sizeof(uint32_t))) return rc;
  uint64_t* r_ids = W->ft_res.as<uint64_t>();
  float* r_dist = (float*)((char*)W->ft_res.p + ids_b);
  uint32_t* r_cnt = (uint32_t*)((char*)W->ft_res.p + ids_b + dist_b);
  if (int32_t rc = search(W->ft_q.as<float>(), k1, r_ids, r_dist, r_cnt)) return rc;
  hipLaunchKernelGGL(byid_drop_self_kernel, dim3((b + 63) / 64), dim3(64), 0, st, (const uint64_t*)r_ids, (const float*)r_dist, (const uint32_t*)r_cnt, ids_dev, b, top_k,
                     out_ids, out_dist, out_count);
  VERS_HIP_TRY(hipGetLastError());
  return VERS_OK;
}

static int32_t by_id_args(vers_ivf* h, const char* who, const void* ids, uint32_t b, uint32_t top_k, uint32_t nprobe, uint32_t flags, const void* out_ids,
                          const void* out_dist, const void* out_count) {
  if (flags & ~(uint32_t)VERS_BYID_EXCLUDE_SELF) return fail(VERS_ERR_INVALID, std::string(who) + ": unknown flag bits");
  if ((flags & VERS_BYID_EXCLUDE_SELF) && nprobe == 0)
    return fail(VERS_ERR_INVALID, std::string(who) + ": VERS_BYID_EXCLUDE_SELF needs nprobe >= 1 (the reference's spill walk has no such identity)");
  if ((flags & VERS_BYID_EXCLUDE_SELF) && top_k == 0xFFFFFFFFu) return fail(VERS_ERR_INVALID, std::string(who) + ": top_k + 1 overflows");
  if (b && (!ids || !out_count || (top_k && (!out_ids || !out_dist)))) return fail(VERS_ERR_INVALID, std::string(who) + ": bad arguments");
  (void)h;
  return VERS_OK;
}
static int32_t by_id_handle(vers_ivf* h, const char* who, bool shards = false) {
  if (h->world > 1 && !shards) return fail(VERS_ERR_INVALID, std::string(who) + ": the handle is sharded by cluster (whether an id is live is known to its owner alone)");
  if (h->k == 0) return fail(VERS_ERR_INSUFFICIENT, "search on an index without centroids (reference: index out of bounds, ivfflat.rs:169)");
  return VERS_OK;
}

// ---- handles sharded by cluster (shard_where.hpp) ------------------------------------------------------------------------------------
// what the three sharded calls refuse from a communicator, before the lock and under it
static int32_t shard_comm_args(const std::string& who, const vers_comm_t* comm) {
  if (comm && (comm->world == 0 || comm->rank >= comm->world || comm->world > 255u || !comm->all_gather)) return fail(VERS_ERR_INVALID, who + ": incomplete vers_comm_t");
  return VERS_OK;
}
static int32_t shard_comm_handle(vers_ivf* h, const std::string& who, const vers_comm_t* comm) {
  const uint32_t world = comm ? comm->world : 1u;
  if (world != h->world || (comm && world > 1 && comm->rank != h->rank))
    return fail(VERS_ERR_INVALID, who + ": the handle is sharded as rank " + std::to_string(h->rank) + " of " + std::to_string(h->world) + ", the communicator says otherwise");
  return VERS_OK;
}

struct Where {  // the gathered table, resolved: the same on every rank
  std::vector<uint32_t> claimer, cluster;
  uint64_t found = 0, missing = 0;
};

// The where round over the n requests located in W->ft_src (local_rc != 0: this rank failed locally and says so in its status word).  ONE
// comm->all_gather of 4 * (n + 1) bytes per rank; nothing of the caller's is written.  A non-zero status word of any rank is every rank's
// return value (the first failing rank's, in rank order).
static int32_t where_round(vers_ivf* h, const std::string& who, const vers_comm_t* comm, uint64_t n, hipStream_t st, int32_t local_rc, Where& wh, double* cb_ms) {
  const uint32_t world = h->world, me = h->rank;
  const size_t nw = (size_t)n + 1;
  const std::string local_why = local_rc ? std::string(vers_last_error()) : std::string();
  {
    int32_t rc = W->g_recv.reserve((size_t)world * nw * sizeof(uint32_t));
    if (!rc && comm) rc = W->g_send.reserve(nw * sizeof(uint32_t));
    if (rc)  // (nothing the library can send: the host aborts the group on a non-zero return, as for the sharded build)
      return local_rc ? local_rc : fail(rc, who + ": the exchange buffers could not be reserved -- this rank cannot join the where round; abort the group");
  }
  uint32_t* mine = comm ? W->g_send.as<uint32_t>() : W->g_recv.as<uint32_t>() + (size_t)me * nw;
  if (!local_rc && n) {
    hipLaunchKernelGGL(shard_where_kernel, dim3(blocks_for(n)), dim3(256), 0, st, (const uint32_t*)W->ft_src.as<uint32_t>(), n, (const uint32_t*)h->list_off.as<uint32_t>(), h->k, mine);
    if (hipGetLastError() != hipSuccess) local_rc = VERS_ERR_HIP;
  }
  if (local_rc && n) (void)hipMemsetAsync(mine, 0xFF, (size_t)n * sizeof(uint32_t), st);
  const uint32_t stw = (uint32_t)local_rc;
  if (hipMemcpyAsync(mine + n, &stw, sizeof(stw), hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return local_rc ? local_rc : fail(VERS_ERR_HIP, who + ": this rank's row of the where table could not be written; abort the group");
  if (comm) {
    const auto t0 = std::chrono::steady_clock::now();
    const int32_t crc = comm->all_gather(comm->ctx, W->g_send.p, W->g_recv.p, (uint64_t)nw * sizeof(uint32_t));
    *cb_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (crc) return local_rc ? local_rc : fail(VERS_ERR_COMM, "vers_comm_t::all_gather reported failure (status " + std::to_string(crc) + ")");
  }
  std::vector<uint32_t> table((size_t)world * nw);
  if (hipMemcpy(table.data(), W->g_recv.p, table.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
    return local_rc ? local_rc : fail(VERS_ERR_HIP, who + ": reading the gathered where table failed");
  uint32_t bad_rank = 0;
  if (const uint32_t s = shw::where_first_failure(table.data(), world, n, &bad_rank)) {
    if (bad_rank == me && local_rc) return fail((int32_t)s, local_why);
    return fail((int32_t)s, who + ": rank " + std::to_string(bad_rank) + " reported status " + std::to_string(s) + "; nothing was written");
  }
  wh.claimer.resize((size_t)n);
  wh.cluster.resize((size_t)n);
  const std::vector<uint8_t> all_mine(h->h_owner.size() == h->k ? 0 : h->k, 0);  // (a one-rank communicator on an unsharded handle)
  const uint8_t* owner = h->h_owner.size() == h->k ? h->h_owner.data() : all_mine.data();
  if (shw::where_resolve(table.data(), world, n, owner, h->k, wh.claimer.data(), wh.cluster.data()) != shw::kWhereOk)
    return fail(VERS_ERR_HIP, who + ": a vec id is claimed by two ranks, or by a rank that does not own its list (inconsistent index); nothing was written");
  wh.found = wh.missing = 0;
  for (uint64_t i = 0; i < n; ++i) (wh.claimer[i] != shw::kNoWord ? wh.found : wh.missing) += 1;
  return VERS_OK;
}

// The row round: the rows of the n resolved requests to out rows 0 .. n - 1 (pitch floats; a request in no list: d zeros), in chunks of
// option "add_batch_rows" requests -- this rank's found rows of a chunk gathered (either local source) in request order at a pitch of d
// floats, padded to the largest rank's count, ONE all_gather per chunk in which any rank found something, shard_place_rows_kernel behind
// it.  A local failure in here has no round left to be told in: the peers are inside their callback and the host aborts the group.
static int32_t row_round(vers_ivf* h, const std::string& who, const vers_comm_t* comm, const Where& wh, uint64_t n, float* out, uint64_t pitch, hipStream_t st,
                         double* cb_ms) {
  const uint32_t world = h->world, me = h->rank, d = h->d;
  const uint64_t R = std::min<uint64_t>((uint64_t)std::max<int64_t>(1, opt_get("add_batch_rows", 131072)), 0xFFFFFFFEull / world);
  std::vector<uint32_t> counts, pad, slot, req;
  std::vector<uint64_t> begin;
  shw::where_plan_rows(wh.claimer.data(), n, world, R, counts, pad, slot);
  shw::where_my_requests(wh.claimer.data(), n, me, R, req, begin);
  uint32_t pad_max = 0;
  for (uint32_t p : pad) pad_max = std::max(pad_max, p);
  const size_t row_b = (size_t)d * sizeof(float);
  // slots [n] | this rank's requests | the compacted source rows of one chunk
  const size_t slot_off = 0, req_off = (size_t)n * 4, csrc_off = req_off + req.size() * 4, stage_b = csrc_off + (size_t)std::max<uint32_t>(pad_max, 1u) * 4;
  if (int32_t rc = W->ft_stage.reserve(stage_b)) return rc;
  if (int32_t rc = W->g_recv.reserve(std::max<size_t>(16, (size_t)world * pad_max * row_b))) return rc;
  if (comm)
    if (int32_t rc = W->g_send.reserve(std::max<size_t>(16, (size_t)pad_max * row_b))) return rc;
  char* stage = (char*)W->ft_stage.p;
  VERS_HIP_TRY(hipMemcpyAsync(stage + slot_off, slot.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  if (!req.empty()) VERS_HIP_TRY(hipMemcpyAsync(stage + req_off, req.data(), req.size() * 4, hipMemcpyHostToDevice, st));
  const uint32_t* slot_dev = (const uint32_t*)(stage + slot_off);
  const uint32_t* req_dev = (const uint32_t*)(stage + req_off);
  uint32_t* csrc = (uint32_t*)(stage + csrc_off);
  const bool tiles = h->rows_rm.p == nullptr;
  const int vec = ((uintptr_t)out % 16u == 0 && pitch % 4u == 0 && d % 4u == 0) ? 1 : 0;
  const uint64_t chunks = shw::where_chunks(n, R);
  for (uint64_t j = 0; j < chunks; ++j) {
    const uint64_t i0 = j * R, m = std::min<uint64_t>(R, n - i0), mine = begin[j + 1] - begin[j];
    if (pad[j]) {
      float* send = comm ? W->g_send.as<float>() : W->g_recv.as<float>() + (size_t)me * pad[j] * d;
      if (mine < pad[j]) VERS_HIP_TRY(hipMemsetAsync(send + mine * d, 0, (size_t)(pad[j] - mine) * row_b, st));  // the padding behind a shorter rank: defined bytes
      if (mine) {
        hipLaunchKernelGGL(shard_pack_src_kernel, dim3(blocks_for(mine)), dim3(256), 0, st, (const uint32_t*)W->ft_src.as<uint32_t>(), req_dev + begin[j], mine, csrc);
        VERS_HIP_TRY(hipGetLastError());
        uint64_t n_jobs = 0;
        if (tiles) {
          unsigned long long* misc = W->ft_misc.as<unsigned long long>();
          VERS_HIP_TRY(hipMemsetAsync(misc + kFtJobs, 0, sizeof(uint64_t), st));
          if (int32_t rc = tile_jobs(csrc, mine, misc, st)) return rc;
          VERS_HIP_TRY(hipMemcpyAsync(&n_jobs, misc + kFtJobs, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
          VERS_HIP_TRY(hipStreamSynchronize(st));
        }
        if (int32_t rc = gather_rows(h, csrc, mine, tiles, n_jobs, send, d, st)) return rc;
      }
      VERS_HIP_TRY(hipStreamSynchronize(st));  // (the callbacks are synchronous: the packed rows are in place)
      if (comm) {
        const auto t0 = std::chrono::steady_clock::now();
        const int32_t crc = comm->all_gather(comm->ctx, W->g_send.p, W->g_recv.p, shw::where_chunk_bytes(pad[j], d));
        *cb_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (crc) return fail(VERS_ERR_COMM, "vers_comm_t::all_gather reported failure (status " + std::to_string(crc) + ")");
      }
    }
    if ((m + 3) / 4 > 0x7FFFFFFFull) return fail(VERS_ERR_INVALID, who + ": too many ids for one chunk");
    hipLaunchKernelGGL(shard_place_rows_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, (const float*)W->g_recv.as<float>(), d, slot_dev, i0, m, out, pitch, vec);
    VERS_HIP_TRY(hipGetLastError());
    VERS_HIP_TRY(hipStreamSynchronize(st));  // (the next chunk overwrites the gathered rows)
  }
  return VERS_OK;
}

// locate + the refusal of an id >= n (0 callbacks) + the where round, for the fetch and the search by id
static int32_t locate_and_agree(vers_ivf* h, const std::string& who, const vers_comm_t* comm, const uint64_t* ids_dev, uint64_t n, hipStream_t st, Where& wh, double* ph) {
  Located L;
  int32_t lrc = locate(h, ids_dev, n, false, st, L, ph);
  if (!lrc && L.bad) return fail(VERS_ERR_INVALID, who + ": a vec id at or beyond n of vers_ivf_info; nothing was written");
  if (!lrc && test_fail_sharded_ref().load() > 0 && test_fail_sharded_ref().fetch_sub(1) > 0) lrc = fail(VERS_ERR_HIP, who + ": injected local failure (test hook)");
  return where_round(h, who, comm, n, st, lrc, wh, &ph[7]);
}

}  // namespace ivf
}  // namespace vers

extern "C" {

int32_t vers_ivf_fetch_dev(vers_ivf_t* h, const uint64_t* vec_ids_dev, uint64_t n, float* out_rows_dev, uint64_t ld_floats, uint64_t* out_clusters_dev,
                           uint8_t* out_status_dev, uint64_t* out_counts, void* stream) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if ((n && !vec_ids_dev) || (out_rows_dev && (ld_floats < h->d || ld_floats % 4)) || n > 0xFFFFFFFFull) return fail(VERS_ERR_INVALID, "vers_ivf_fetch_dev: bad arguments");
  std::shared_lock<std::shared_mutex> lk(h->index);
  if (int32_t rc = fetch_check_handle(h, "vers_ivf_fetch_dev")) return rc;
  if (n == 0) {
    if (out_counts) out_counts[0] = out_counts[1] = 0;
    return VERS_OK;
  }
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)stream;
  WsLease lease(h, true, st);
  if (lease.rc) return lease.rc;
  if (int32_t rc = lease.order_on(st)) return rc;
  double ph[kFetchPhases] = {};
  Located L;
  if (int32_t rc = locate(h, vec_ids_dev, n, out_rows_dev != nullptr, st, L, ph)) return rc;
  if (L.bad) return fail(VERS_ERR_INVALID, "vers_ivf_fetch_dev: a vec id at or beyond n of vers_ivf_info; nothing was written");
  {
    PhaseClock clk(&ph[5], st);
    if (int32_t rc = deliver(h, n, L, out_rows_dev, ld_floats, out_clusters_dev, out_status_dev, st)) return rc;
    if (int32_t rc = clk.done()) return rc;  // the call waits for its stream
  }
  if (out_counts) { out_counts[0] = L.found; out_counts[1] = L.missing; }
  ph[0] = 1.0; ph[1] = (double)n; ph[2] = (double)L.found;
  phases_commit(ph);
  return VERS_OK;
}

int32_t vers_ivf_fetch(vers_ivf_t* h, const uint64_t* vec_ids, uint64_t n, float* out_rows, uint64_t row_stride_bytes, uint64_t* out_clusters, uint8_t* out_status,
                       uint64_t* out_counts) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if ((n && !vec_ids) || (out_rows && (row_stride_bytes < (uint64_t)h->d * 4 || row_stride_bytes % 4))) return fail(VERS_ERR_INVALID, "vers_ivf_fetch: bad arguments");
  std::shared_lock<std::shared_mutex> lk(h->index);
  if (int32_t rc = fetch_check_handle(h, "vers_ivf_fetch")) return rc;
  for (uint64_t i = 0; i < n; ++i)  // ALL OR NOTHING: every id before the first store
    if (vec_ids[i] >= h->n_total) return fail(VERS_ERR_INVALID, "vers_ivf_fetch: a vec id at or beyond n of vers_ivf_info; nothing was written");
  if (n == 0) {
    if (out_counts) out_counts[0] = out_counts[1] = 0;
    return VERS_OK;
  }
  DeviceGuard g(h->device);
  WsLease lease(h);
  if (lease.rc) return lease.rc;
  if (!W->io_stream) VERS_HIP_TRY(hipStreamCreateWithFlags(&W->io_stream, hipStreamNonBlocking));
  const hipStream_t st = W->io_stream;
  if (W->used && W->last_stream != st) VERS_HIP_TRY(hipStreamWaitEvent(st, W->done, 0));
  lease.st = st;
  // bounded staging, the mutators' options: a chunk of rows as add_batch stages them, a chunk of ids as remove_batch does
  const uint64_t chunk = std::min<uint64_t>(n, (uint64_t)std::max<int64_t>(1, out_rows ? opt_get("add_batch_rows", 131072) : opt_get("remove_batch_ids", 1 << 20)));
  const uint32_t d = h->d, ldx = h->ldx;
  const size_t ids_b = ((size_t)chunk * 8 + 15) & ~(size_t)15, rows_b = out_rows ? (size_t)chunk * ldx * 4 : 0, cl_b = out_clusters ? (size_t)chunk * 8 : 0;
  const size_t st_b = out_status ? (size_t)chunk : 0, total_b = ids_b + rows_b + cl_b + st_b;
  if (total_b > W->io_pin_cap) {
    if (W->io_pin) (void)hipHostFree(W->io_pin);
    W->io_pin = nullptr; W->io_pin_cap = 0;
    VERS_HIP_TRY(hipHostMalloc(&W->io_pin, total_b, hipHostMallocDefault));
    W->io_pin_cap = total_b;
  }
  if (int32_t rc = W->ft_stage.reserve(total_b)) return rc;
  char *pin = (char*)W->io_pin, *dev = (char*)W->ft_stage.p;
  double ph[kFetchPhases] = {};
  uint64_t found = 0, missing = 0;
  for (uint64_t i0 = 0; i0 < n; i0 += chunk) {
    const uint64_t m = std::min(chunk, n - i0);
    {
      PhaseClock clk(&ph[3], st);
      std::memcpy(pin, vec_ids + i0, (size_t)m * 8);
      VERS_HIP_TRY(hipMemcpyAsync(dev, pin, (size_t)m * 8, hipMemcpyHostToDevice, st));
      if (int32_t rc = clk.done()) return rc;
    }
    Located L;
    if (int32_t rc = locate(h, (const uint64_t*)dev, m, out_rows != nullptr, st, L, ph)) return rc;
    if (L.bad) return fail(VERS_ERR_HIP, "vers_ivf_fetch: the device disagrees with the host's range check");
    {
      PhaseClock clk(&ph[5], st);
      if (int32_t rc = deliver(h, m, L, out_rows ? (float*)(dev + ids_b) : nullptr, ldx, out_clusters ? (uint64_t*)(dev + ids_b + rows_b) : nullptr,
                               out_status ? (uint8_t*)(dev + ids_b + rows_b + cl_b) : nullptr, st))
        return rc;
      if (int32_t rc = clk.done()) return rc;
    }
    {
      PhaseClock clk(&ph[6], st);
      if (total_b > ids_b) VERS_HIP_TRY(hipMemcpyAsync(pin + ids_b, dev + ids_b, total_b - ids_b, hipMemcpyDeviceToHost, st));
      VERS_HIP_TRY(hipStreamSynchronize(st));
      if (out_rows)
        for (uint64_t i = 0; i < m; ++i) std::memcpy((char*)out_rows + (size_t)(i0 + i) * row_stride_bytes, pin + ids_b + (size_t)i * ldx * 4, (size_t)d * 4);
      if (out_clusters) std::memcpy(out_clusters + i0, pin + ids_b + rows_b, (size_t)m * 8);
      if (out_status) std::memcpy(out_status + i0, pin + ids_b + rows_b + cl_b, (size_t)m);
      if (int32_t rc = clk.done()) return rc;
    }
    found += L.found; missing += L.missing;
  }
  if (out_counts) { out_counts[0] = found; out_counts[1] = missing; }
  ph[0] = 1.0; ph[1] = (double)n; ph[2] = (double)found;
  phases_commit(ph);
  return VERS_OK;
}

int32_t vers_fetch_phases(double* out8, int32_t reset) {
  std::lock_guard<std::mutex> lk(g_ft_mu);
  if (out8)
    for (int i = 0; i < kFetchPhases; ++i) out8[i] = g_ft[i];
  if (reset)
    for (double& v : g_ft) v = 0.0;
  return VERS_OK;
}

int32_t vers_ivf_search_by_id_dev(vers_ivf_t* h, const uint64_t* vec_ids_dev, uint32_t b, uint32_t top_k, uint32_t nprobe, uint32_t flags, uint64_t* out_ids_dev,
                                  float* out_dist_dev, uint32_t* out_count_dev, void* stream) {
  const char* who = "vers_ivf_search_by_id_dev";
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (int32_t rc = by_id_args(h, who, vec_ids_dev, b, top_k, nprobe, flags, out_ids_dev, out_dist_dev, out_count_dev)) return rc;
  std::shared_lock<std::shared_mutex> lk(h->index);
  if (int32_t rc = by_id_handle(h, who)) return rc;
  if (b == 0) return VERS_OK;
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)stream;
  WsLease lease(h, true, st);
  if (lease.rc) return lease.rc;
  if (int32_t rc = lease.order_on(st)) return rc;
  return by_id_locked(h, who, vec_ids_dev, b, top_k, flags, out_ids_dev, out_dist_dev, out_count_dev, st,
                      [&](const float* q, uint32_t kk, uint64_t* o_ids, float* o_dist, uint32_t* o_cnt) -> int32_t {
                        return search_dev_locked(h, q, h->ldq, b, kk, nprobe, o_ids, o_dist, o_cnt, nullptr, st);
                      });
}

int32_t vers_ivf_search_by_id(vers_ivf_t* h, const uint64_t* vec_ids, uint32_t b, uint32_t top_k, uint32_t nprobe, uint32_t flags, uint64_t* out_ids, float* out_dist,
                              uint32_t* out_count) {
  const char* who = "vers_ivf_search_by_id";
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (int32_t rc = by_id_args(h, who, vec_ids, b, top_k, nprobe, flags, out_ids, out_dist, out_count)) return rc;
  std::shared_lock<std::shared_mutex> lk(h->index);
  if (int32_t rc = by_id_handle(h, who)) return rc;
  for (uint32_t q = 0; q < b; ++q)
    if (vec_ids[q] >= h->n_total) return fail(VERS_ERR_INVALID, std::string(who) + ": a vec id at or beyond n of vers_ivf_info; nothing was written");
  if (b == 0) return VERS_OK;
  DeviceGuard g(h->device);
  WsLease lease(h);
  if (lease.rc) return lease.rc;
  HostStatusSlot slot(h);
  if (!W->io_stream) VERS_HIP_TRY(hipStreamCreateWithFlags(&W->io_stream, hipStreamNonBlocking));
  const hipStream_t st = W->io_stream;
  if (W->used && W->last_stream != st) VERS_HIP_TRY(hipStreamWaitEvent(st, W->done, 0));
  lease.st = st;
  // ids in, results out: one device block (the queries never leave the device)
  const size_t need = (size_t)b * std::max<uint32_t>(top_k, 1);
  const size_t ids_off = (size_t)b * 8, dist_off = ids_off + need * 8, cnt_off = dist_off + ((need * 4 + 7) & ~(size_t)7), total = cnt_off + (size_t)b * 4;
  if (int32_t rc = W->ft_stage.reserve(total)) return rc;
  char* dev = (char*)W->ft_stage.p;
  VERS_HIP_TRY(hipMemcpyAsync(dev, vec_ids, (size_t)b * 8, hipMemcpyHostToDevice, st));
  int32_t status_rc = VERS_OK;
  const int32_t rc = by_id_locked(
      h, who, (const uint64_t*)dev, b, top_k, flags, (uint64_t*)(dev + ids_off), (float*)(dev + dist_off), (uint32_t*)(dev + cnt_off), st,
      [&](const float* q, uint32_t kk, uint64_t* o_ids, float* o_dist, uint32_t* o_cnt) -> int32_t {
        // reference mode as vers_ivf_search walks it: 16 ranked lists first, then 48, then 64 by the exact coarse quantiser, at last all of them
        for (int attempt = nprobe == 0 ? 0 : 1; attempt < 4; ++attempt) {
          W->ref_shallow = attempt == 0;
          W->ref_deep = attempt == 2;
          W->ref_all = attempt == 3;
          VERS_HIP_TRY(hipMemsetAsync(o_ids, 0, (size_t)b * kk * 8, st));
          VERS_HIP_TRY(hipMemsetAsync(o_dist, 0, (size_t)b * kk * 4, st));
          VERS_HIP_TRY(hipMemsetAsync(o_cnt, 0, (size_t)b * 4, st));
          const uint32_t slice = attempt == 3 ? std::max<uint32_t>(1u, 65536u / std::max<uint32_t>(1u, h->k)) : b;
          int32_t r = VERS_OK;
          for (uint32_t q0 = 0; q0 < b && r == VERS_OK; q0 += slice)
            r = search_dev_locked(h, q + (size_t)q0 * h->ldq, h->ldq, std::min(slice, b - q0), kk, nprobe, o_ids + (size_t)q0 * kk, o_dist + (size_t)q0 * kk, o_cnt + q0,
                                  nullptr, st);
          W->ref_shallow = W->ref_deep = W->ref_all = false;
          if (r) return r;
          uint32_t s = 0;
          VERS_HIP_TRY(hipMemcpyAsync(&s, W->st_word(), sizeof(s), hipMemcpyDeviceToHost, st));
          VERS_HIP_TRY(hipStreamSynchronize(st));
          status_rc = status_to_rc(h, s, W->st_slot);
          if (status_rc != kRetrySpill) break;
          if ((attempt == 0 && h->k <= 16) || (attempt == 1 && h->k <= 48) || (attempt == 2 && h->k <= 64)) break;  // every list was ranked already
        }
        return status_rc == kRetrySpill ? VERS_ERR_INVALID : status_rc;
      });
  if (rc) {
    (void)hipStreamSynchronize(st);  // (the staging copy read the caller's memory)
    return rc;
  }
  VERS_HIP_TRY(hipStreamSynchronize(st));
  if (top_k) {
    VERS_HIP_TRY(hipMemcpy(out_ids, dev + ids_off, (size_t)b * top_k * 8, hipMemcpyDeviceToHost));
    VERS_HIP_TRY(hipMemcpy(out_dist, dev + dist_off, (size_t)b * top_k * 4, hipMemcpyDeviceToHost));
  }
  VERS_HIP_TRY(hipMemcpy(out_count, dev + cnt_off, (size_t)b * 4, hipMemcpyDeviceToHost));
  return VERS_OK;
}

int32_t vers_ivf_fetch_sharded_dev(vers_ivf_t* h, const vers_comm_t* comm, const uint64_t* vec_ids_dev, uint64_t n, float* out_rows_dev, uint64_t ld_floats,
                                   uint64_t* out_clusters_dev, uint8_t* out_status_dev, uint64_t* out_counts, void* stream) {
  const std::string who = "vers_ivf_fetch_sharded_dev";
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if ((n && !vec_ids_dev) || (out_rows_dev && (ld_floats < h->d || ld_floats % 4)) || n > 0xFFFFFFFEull) return fail(VERS_ERR_INVALID, who + ": bad arguments");
  if (int32_t rc = shard_comm_args(who, comm)) return rc;
  std::shared_lock<std::shared_mutex> lk(h->index);
  if (int32_t rc = shard_comm_handle(h, who, comm)) return rc;
  if (comm == nullptr) {  // an unsharded handle: the existing call
    lk.unlock();
    return vers_ivf_fetch_dev(h, vec_ids_dev, n, out_rows_dev, ld_floats, out_clusters_dev, out_status_dev, out_counts, stream);
  }
  if (int32_t rc = fetch_check_handle(h, who.c_str(), true)) return rc;
  if (n == 0) {
    if (out_counts) out_counts[0] = out_counts[1] = 0;
    return VERS_OK;
  }
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)stream;
  WsLease lease(h, true, st);
  if (lease.rc) return lease.rc;
  if (int32_t rc = lease.order_on(st)) return rc;
  double ph[kFetchPhases] = {};
  Where wh;
  if (int32_t rc = locate_and_agree(h, who, comm, vec_ids_dev, n, st, wh, ph)) return rc;
  {
    PhaseClock clk(&ph[5], st);
    const double cb0 = ph[7];
    if (out_clusters_dev != nullptr || out_status_dev != nullptr) {
      if (int32_t rc = W->ft_res.reserve((size_t)n * sizeof(uint32_t))) return rc;
      VERS_HIP_TRY(hipMemcpyAsync(W->ft_res.p, wh.cluster.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(shard_meta_kernel, dim3(blocks_for(n)), dim3(256), 0, st, (const uint32_t*)W->ft_res.as<uint32_t>(), n, out_clusters_dev, out_status_dev);
      VERS_HIP_TRY(hipGetLastError());
    }
    if (out_rows_dev != nullptr)
      if (int32_t rc = row_round(h, who, comm, wh, n, out_rows_dev, ld_floats, st, &ph[7])) return rc;
    if (int32_t rc = clk.done()) return rc;  // the call waits for its stream
    ph[5] -= ph[7] - cb0;                    // (the callbacks are counted in [7] alone)
  }
  if (out_counts) { out_counts[0] = wh.found; out_counts[1] = wh.missing; }
  ph[0] = 1.0; ph[1] = (double)n; ph[2] = (double)wh.found;
  phases_commit(ph);
  return VERS_OK;
}

int32_t vers_ivf_search_by_id_sharded_dev(vers_ivf_t* h, const vers_comm_t* comm, const vers_gather_t* g, const uint64_t* vec_ids_dev, uint32_t b, uint32_t top_k,
                                          uint32_t nprobe, uint32_t flags, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev, void* stream) {
  const char* who_c = "vers_ivf_search_by_id_sharded_dev";
  const std::string who = who_c;
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (int32_t rc = by_id_args(h, who_c, vec_ids_dev, b, top_k, nprobe, flags, out_ids_dev, out_dist_dev, out_count_dev)) return rc;
  if (int32_t rc = shard_comm_args(who, comm)) return rc;
  if (g && (g->world == 0 || g->rank >= g->world || (g->world > 1 && !g->all_gather_async))) return fail(VERS_ERR_INVALID, who + ": incomplete vers_gather_t");
  if ((comm == nullptr) != (g == nullptr)) return fail(VERS_ERR_INVALID, who + ": comm and g come together (both NULL on an unsharded handle)");
  if (comm && (comm->world != g->world || comm->rank != g->rank)) return fail(VERS_ERR_INVALID, who + ": comm and g name different ranks");
  std::shared_lock<std::shared_mutex> lk(h->index);
  if (int32_t rc = shard_comm_handle(h, who, comm)) return rc;
  if (comm == nullptr) {  // an unsharded handle: the existing call
    lk.unlock();
    return vers_ivf_search_by_id_dev(h, vec_ids_dev, b, top_k, nprobe, flags, out_ids_dev, out_dist_dev, out_count_dev, stream);
  }
  if (int32_t rc = by_id_handle(h, who_c, true)) return rc;
  if (b == 0) return VERS_OK;
  DeviceGuard gd(h->device);
  hipStream_t st = (hipStream_t)stream;
  WsLease lease(h, true, st);
  if (lease.rc) return lease.rc;
  if (int32_t rc = lease.order_on(st)) return rc;
  double ph[kFetchPhases] = {};
  Where wh;
  if (int32_t rc = locate_and_agree(h, who, comm, vec_ids_dev, b, st, wh, ph)) return rc;
  if (wh.missing) return fail(VERS_ERR_INVALID, who + ": a vec id that is in no list (vers_ivf_fetch_sharded_dev tells which); nothing was written");
  if (top_k == 0) {
    VERS_HIP_TRY(hipMemsetAsync(out_count_dev, 0, sizeof(uint32_t) * b, st));
    return VERS_OK;
  }
  const uint32_t ldq = h->ldq;
  const size_t q_bytes = (size_t)b * ldq * sizeof(float);
  if (int32_t rc = W->ft_q.reserve(q_bytes)) return rc;
  VERS_HIP_TRY(hipMemsetAsync(W->ft_q.p, 0, q_bytes, st));  // (the padding columns of a query block are zeros)
  if (int32_t rc = row_round(h, who, comm, wh, b, W->ft_q.as<float>(), ldq, st, &ph[7])) return rc;
  const float* q = W->ft_q.as<float>();
  // From here on the protocol is the sharded search's, which takes the handle and a workspace of its own: this call keeps its workspace
  // (the query block) and gives the handle back first.
  lk.unlock();
  if (!(flags & VERS_BYID_EXCLUDE_SELF)) return vers_ivf_search_sharded_dev(h, g, q, ldq, b, top_k, nprobe, out_ids_dev, out_dist_dev, out_count_dev, stream);
  const uint32_t k1 = top_k + 1u;
  const size_t ids_b = (size_t)b * k1 * sizeof(uint64_t), dist_b = (((size_t)b * k1 * sizeof(float)) + 7) & ~(size_t)7;
  if (int32_t rc = W->ft_res.reserve(ids_b + dist_b + (size_t)b * sizeof(uint32_t))) return rc;
  uint64_t* r_ids = W->ft_res.as<uint64_t>();
  float* r_dist = (float*)((char*)W->ft_res.p + ids_b);
  uint32_t* r_cnt = (uint32_t*)((char*)W->ft_res.p + ids_b + dist_b);
  if (int32_t rc = vers_ivf_search_sharded_dev(h, g, q, ldq, b, k1, nprobe, r_ids, r_dist, r_cnt, stream)) return rc;
  hipLaunchKernelGGL(byid_drop_self_kernel, dim3((b + 63) / 64), dim3(64), 0, st, (const uint64_t*)r_ids, (const float*)r_dist, (const uint32_t*)r_cnt, vec_ids_dev, b, top_k,
                     out_ids_dev, out_dist_dev, out_count_dev);
  VERS_HIP_TRY(hipGetLastError());
  return VERS_OK;
}

}  // extern "C"
