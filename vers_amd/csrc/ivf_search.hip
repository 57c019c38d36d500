// ivf_search.hip -- the second half of search_approximate (ivfflat.rs:166-198): the inverted-list scans (single query: item
// records; batches in nprobe mode: matrix-core pre-selection + exact finish, prescan.hip.h; otherwise the ordered-chain
// engine, scan.hip.h), the per-query merges + id mapping, the exhaustive scan of the stored rows (utils.rs:68-82), the
// cross-GPU merge of partial results, host-pointer staging, and the search entry points of the C ABI.
#include <chrono>
#include <cstring>
#include <functional>
#include <limits>
#include <optional>
#include <vector>

#include "finish.hip.h"
#include "ball_filter.hip.h"
#include "head_filter.hip.h"
#include "flat_shadow.hpp"
#include "ivf_src.hip.h"
#include "single.hip.h"
#include "finish_wide.hip.h"
#include "range_driver.hip.h"
#include "range_merge.hip.h"
#include "filter.hip.h"
#include "filter_multi.hip.h"
#include "filter_adaptive.hip.h"
#include "filter_range.hip.h"
#include "filter_range_multi.hip.h"
#include "filter_prepared.hip.h"

namespace vers {

// final merge + id mapping: one block per query.  Results wider than 64 keys come 64 ranks per pass (ScanParams::lower):
// this pass emits ranks rank0 .. rank0+63 of every merge group into output row q (pitch top_k) and leaves the group's
// last key as the next pass's lower bound.
struct MergeArgs {
  const uint64_t* partials; uint32_t P, S_max, k_keep; int ref_mode;
  const uint32_t *np, *pj_list, *pj_pref, *pj_take, *list_off, *row_ids;
  uint32_t top_k, rank0;
  uint64_t* out_ids; float* out_dist; uint32_t* out_count; uint64_t* out_keys; uint64_t* lower_out;
  const uint32_t* st_word = nullptr; uint32_t* st_host = nullptr;  // host-pointer single-query call: the stream's status word goes out with the result
};
template <int NW>
__device__ __forceinline__ void ivf_merge_block(const MergeArgs& m, uint32_t q, uint64_t (*sh)[kWave]) {
  const uint32_t P = m.P, S_max = m.S_max, k_keep = m.k_keep, top_k = m.top_k, rank0 = m.rank0;
  const int lane = threadIdx.x & 63;
  const bool w0 = threadIdx.x < kWave;
  const uint64_t* pq = m.partials + (uint64_t)q * P * S_max * k_keep;
  const uint64_t o_base = (uint64_t)q * top_k;
  uint32_t written = 0;
  const uint32_t n_groups = m.ref_mode ? m.np[q] : 1;
  SeqRowsPre pre = {};  // (nprobe mode, P <= 64: what maps a key to its storage row, in flight under the merge)
  const bool pre_ok = !m.ref_mode && P <= (uint32_t)kWave;
  if (w0 && pre_ok) pre = wave_seq_rows_load(lane, m.pj_list + (uint64_t)q * P, m.pj_pref + (uint64_t)q * P, P);
  auto mid = [&]() { if (w0 && pre_ok) wave_seq_rows_load2(pre, m.list_off); };
  if (w0 && m.out_keys && rank0 == 0)
    for (uint32_t i = (uint32_t)lane; i < top_k; i += kWave) m.out_keys[o_base + i] = kKeyMax;  // holes = other GPUs' lists
  for (uint32_t grp = 0; grp < n_groups; ++grp) {
    uint64_t list;
    uint32_t n_emit;
    if (m.ref_mode) {
      const uint32_t take = m.pj_take[(uint64_t)q * P + grp];
      if (take == 0) continue;  // uniform per block
      n_emit = take > rank0 ? (take - rank0 < (uint32_t)kWave ? take - rank0 : (uint32_t)kWave) : 0u;
      if (m.pj_list[(uint64_t)q * P + grp] == kNoList || n_emit == 0) {  // scanned by the GPU that owns the list / this pair is complete
        written += take;
        continue;
      }
      list = block_merge_keys<NW>(pq + (uint64_t)grp * S_max * k_keep, S_max * k_keep, k_keep, sh);
      if (w0) {
        const bool have = lane < (int)n_emit && list != kKeyMax;
        const uint32_t row = have ? m.list_off[m.pj_list[(uint64_t)q * P + grp]] + ((uint32_t)list - m.pj_pref[(uint64_t)q * P + grp]) : 0u;
        if (have) {
          const uint64_t o = o_base + written + rank0 + lane;
          m.out_ids[o] = m.row_ids[row];
          m.out_dist[o] = __uint_as_float(order_bits_to_f32_bits((uint32_t)(list >> 32)));
          if (m.out_keys) m.out_keys[o] = list;
        }
        if (m.lower_out && lane == kWave - 1) m.lower_out[(uint64_t)q * P + grp] = list;
      }
      written += take;
    } else {
      n_emit = top_k - rank0 < (uint32_t)kWave ? top_k - rank0 : (uint32_t)kWave;
      list = block_merge_keys<NW>(pq, P * S_max * k_keep, k_keep, sh, mid);
      if (w0) {
        const bool have = lane < (int)n_emit && list != kKeyMax;
        const uint32_t row = pre_ok ? wave_seq_rows_map(list, have, lane, pre)
                                    : wave_seq_rows(list, have, lane, m.pj_list + (uint64_t)q * P, m.pj_pref + (uint64_t)q * P, P, m.list_off);
        if (have) {
          const uint64_t o = o_base + rank0 + lane;
          m.out_ids[o] = m.row_ids[row];
          m.out_dist[o] = __uint_as_float(order_bits_to_f32_bits((uint32_t)(list >> 32)));
          if (m.out_keys) m.out_keys[o] = list;
        }
        if (m.lower_out && lane == kWave - 1) m.lower_out[(uint64_t)q * P] = list;
        const uint32_t cnt = (uint32_t)__popcll(__ballot(have));
        written = rank0 == 0 || cnt ? rank0 + cnt : 0xFFFFFFFFu;  // (a later pass that finds nothing leaves the count alone)
      }
    }
  }
  if (w0 && lane == 0 && written != 0xFFFFFFFFu && (m.ref_mode ? rank0 == 0 : true)) m.out_count[q] = written;
  // host-pointer single-query call: the status word goes out with the result, LAST and at system scope -- the host spins on this
  // pinned word instead of sleeping in hipStreamSynchronize (host_io_end), so everything wave 0 wrote above must be visible first
  if (m.st_host && w0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    if (lane == 0) __hip_atomic_store(m.st_host, __hip_atomic_load(m.st_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
template <int NW>
__global__ __launch_bounds__(kWave * NW) void ivf_merge_kernel(MergeArgs m) {
  __shared__ uint64_t sh[NW][kWave];
  ivf_merge_block<NW>(m, blockIdx.x, sh);
}

// exhaustive merge for the IVF handle (seq == vec_id already): ranks rank0 .. rank0 + k - 1 of output row q (pitch top_k);
// top_k > 64 comes 64 ranks per pass (ScanParams::lower)
__global__ __launch_bounds__(kWave * kMergeWaves) void seg_merge_kernel(const uint64_t* partials, uint32_t n_segs, uint32_t k, uint32_t top_k,
                                                                        uint32_t rank0, uint64_t* out_ids, float* out_dist,
                                                                        uint32_t* out_count, uint64_t* lower_out) {
  __shared__ uint64_t sh[kMergeWaves][kWave];
  const uint32_t q = blockIdx.x;
  uint64_t list = block_merge_keys(partials + (uint64_t)q * n_segs * k, n_segs * k, k, sh);
  if (threadIdx.x >= kWave) return;
  const int lane = threadIdx.x;
  const bool have = lane < (int)k && list != kKeyMax;
  if (have) {
    out_ids[(uint64_t)q * top_k + rank0 + lane] = (uint32_t)list;
    out_dist[(uint64_t)q * top_k + rank0 + lane] = __uint_as_float(order_bits_to_f32_bits((uint32_t)(list >> 32)));
  }
  if (lower_out != nullptr && lane == (int)k - 1) lower_out[q] = list;  // (kKeyMax when the rows ran out: the next pass finds nothing)
  const uint32_t cnt = (uint32_t)__popcll(__ballot(have));
  if (lane == 0 && (rank0 == 0 || cnt)) out_count[q] = rank0 + cnt;
}

// cross-GPU merge of per-rank partial results ([world][b][k] keys + ids, kKeyMax padded): one wave per query.
// nprobe mode: global top-k by key.  reference mode: position p of the output belongs to exactly one rank
// (the owner of the list that position came from), so the merge is a position-wise minimum.
// status != nullptr: a rank whose partial is poisoned (it failed locally, see kStPeerFailed) is reported there.
__global__ __launch_bounds__(kWave) void rank_merge_kernel(const uint64_t* keys, const uint64_t* ids, uint64_t rank_stride,
                                                           uint32_t world, uint32_t b, uint32_t k, int ref_mode,
                                                           uint64_t* out_ids, float* out_dist, uint32_t* out_count, uint32_t* status = nullptr) {
  const uint32_t q = blockIdx.x;
  const int lane = threadIdx.x;
  if (status != nullptr && q == 0)
    for (uint32_t r = lane; r < world; r += kWave)
      if (keys[r * rank_stride] == kKeyMax && ids[r * rank_stride] == kPoisonId) atomicOr(status, kStPeerFailed);
  uint32_t total = 0;
  uint64_t lower = 0;  // nprobe mode, k > 64: 64 ranks per pass, keys at or below the previous pass's last key are skipped
  for (uint32_t r0 = 0; r0 < k; r0 += kWave) {
    const uint32_t kk = k - r0 < (uint32_t)kWave ? k - r0 : (uint32_t)kWave;
    uint64_t key = kKeyMax, id = 0;
    if (ref_mode) {
      if (lane < (int)kk)
        for (uint32_t r = 0; r < world; ++r) {
          const uint64_t kx = keys[r * rank_stride + (uint64_t)q * k + r0 + lane];
          if (kx < key) { key = kx; id = ids[r * rank_stride + (uint64_t)q * k + r0 + lane]; }
        }
    } else {
      uint64_t list = kKeyMax;
      const uint32_t n = world * k;
      for (uint32_t i = 0; i < n; i += kWave) {
        uint64_t cand = kKeyMax;
        if (i + lane < n) cand = keys[(uint64_t)((i + lane) / k) * rank_stride + (uint64_t)q * k + (i + lane) % k];
        if (cand <= lower) cand = kKeyMax;
        wave_topk_update(list, kk, cand, kKeyMax);
      }
      key = lane < (int)kk ? list : kKeyMax;
      if (key != kKeyMax)  // keys are unique: find where this one came from to pick up its id
        for (uint32_t i = 0; i < n; ++i) {
          const uint64_t o = (uint64_t)(i / k) * rank_stride + (uint64_t)q * k + i % k;
          if (keys[o] == key) { id = ids[o]; break; }
        }
      lower = readlane64(list, (int)kk - 1);
    }
    const bool have = key != kKeyMax;
    if (have) {
      out_ids[(uint64_t)q * k + r0 + lane] = id;
      out_dist[(uint64_t)q * k + r0 + lane] = __uint_as_float(order_bits_to_f32_bits((uint32_t)(key >> 32)));
    }
    total += (uint32_t)__popcll(__ballot(have));
    if (!ref_mode && lower == kKeyMax) break;  // fewer keys than ranks: nothing left for later passes
  }
  if (lane == 0) out_count[q] = total;
}

// local exhaustive results -> (key, vec_id) pairs for the cross-GPU merge: key = (order bits of the distance << 32) |
// vec_id, the reference's stable order (utils.rs:77: ties -> lower index); kKeyMax padded
__global__ void pack_exhaustive_keys_kernel(const uint64_t* ids, const float* dist, const uint32_t* cnt, uint32_t b, uint32_t k,
                                            uint64_t* out_keys, uint64_t* out_ids) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b * k) return;
  const uint32_t q = i / k, j = i - q * k;
  const bool have = j < cnt[q];
  out_keys[i] = have ? make_key(dist[i], (uint32_t)ids[i]) : kKeyMax;
  out_ids[i] = have ? ids[i] : ~0ull;
}

}  // namespace vers

namespace vers {
namespace ivf {

static size_t filter_wave_slots(const vers_ivf* h) { return (size_t)h->n_cu * 3 * kWavesPerBlock; }  // (filter_scan_kernel: at most 3 blocks per CU)

// The filtered kernel a pass launches: none, the per-call mask's (filter.hip.h, filter_range.hip.h) or the per-query sets' (filter_multi.hip.h,
// filter_range_multi.hip.h).  A call's FilterMasks (below) hands it out once filter_begin has filled them; the top-k drivers and the range source
// pass it down, and nothing else about a pass differs between the two.
struct FilterChoice {
  const FilterParams* one = nullptr;
  const FilterMultiParams* multi = nullptr;
  explicit operator bool() const { return one != nullptr || multi != nullptr; }
};

// One pass of the ordered-chain list scan over the planned items, timed through the scan-timing ring.  Without a filter, option "scan_debug"
// decides: bit 3 switches the pruning bounds off (A/B runs), bit 4 stamps phases, bit 5 switches the hand-out counter off.  flt: the filtered
// kernel (filter.hip.h), which knows no diagnosis switches -- bounds and counter always on for QG != 1 -- and launches no more waves than it
// has counter slots (filter_begin).  The per-query kernel (filter_multi.hip.h) is launched the same way.
template <int QG>
int32_t launch_ivf_scan(vers_ivf* h, const IvfSrc<QG>& src, uint32_t items_bound, hipStream_t st, const uint64_t* lower, FilterChoice flt = {}) {
  ScanParams p = ivf_scan_params(h, src.k_keep, lower);
  p.debug = flt ? 0u : scan_debug_flags();
  if (p.debug & 16u) {  // diagnosis only
    if (int32_t rc = W->stamps.reserve(512)) return rc;
    VERS_HIP_TRY(hipMemsetAsync(W->stamps.p, 0, 128, st));
    p.stamps = W->stamps.as<unsigned long long>();
  }
  // pruning bounds shared between the items of a merge group (they run at different times here, unlike the segment scans)
  if (QG != 1 && !(p.debug & 8u)) p.bounds = W->partials.as<uint64_t>() + W->ivf_bounds_off;
  if (QG != 1 && !(p.debug & 32u))
    if (int32_t rc = fresh_quad_counter(st, &p.next_quad)) return rc;
  const size_t lds = scan_lds_bytes(QG, h->ld);
  const uint32_t blocks = scan_grid(h->n_cu, QG, h->ld, items_bound, flt ? (uint32_t)(filter_wave_slots(h) / kWavesPerBlock) : 0xFFFFFFFFu);
  return with_metric(h->metric, [&](auto m) -> int32_t {
    constexpr int M = decltype(m)::value;
    if (flt.multi) return launch_scan_timed(filter_multi_scan_kernel<QG, M, IvfSrc<QG>>, blocks, kWavesPerBlock, lds, st, src, p, *flt.multi);
    if (flt.one) return launch_scan_timed(filter_scan_kernel<QG, M, IvfSrc<QG>>, blocks, kWavesPerBlock, lds, st, src, p, *flt.one);
    return launch_scan_timed(scan_kernel<QG, M, IvfSrc<QG>>, blocks, kWavesPerBlock, lds, st, src, p);
  });
}

// a single query's list scan over item records (scan1_kernel); timed through the same event ring.  No stamps (bit 4 of "scan_debug" masked).
int32_t launch_scan1(vers_ivf* h, const Scan1Args& a, uint32_t items_bound, hipStream_t st, const uint64_t* lower, bool few_tiles) {
  ScanParams p = ivf_scan_params(h, a.k_keep, lower);
  p.debug = scan_debug_flags() & ~16u;
  // a tile per block of 16 waves (scan1t_kernel: the whole tile in flight at once) instead of a tile per wave; option "scan1t" = 0: the latter
  // ... when the query visits few tiles -- the reference's own mode, a few probes --: with a tile per CU and round, 1361 tiles (nprobe = 32 at
  // cfg3 without a shadow) take 72 us against the tile-per-wave kernel's 58
  const bool tile_per_block = opt_get("scan1t", 1) != 0 && few_tiles && knobs().seg_rows <= 0;  // (a record is ONE tile unless the tuning knob cut the lists differently)
  return with_metric(h->metric, [&](auto m) -> int32_t {
    constexpr int M = decltype(m)::value;
    if (tile_per_block)
      return launch_scan_timed(scan1t_kernel<M>, std::max<uint32_t>(1u, std::min<uint32_t>(items_bound, (uint32_t)h->n_cu)), kT1Waves, kT1LdsBytes, st, a, p);
    // (W->items holds items_bound + 4 records: one per launched wave)
    return launch_scan_timed(scan1_kernel<M>, scan_grid(h->n_cu, 1, h->ld, items_bound), kWavesPerBlock, 0, st, a, p);
  });
}

// a single query's list scan on the fp16 shadow (scan1h_kernel: a block per record); timed through the same event ring
int32_t launch_scan1h(vers_ivf* h, const Scan1hArgs& a, uint32_t items_bound, hipStream_t st) {
  // (W->items holds items_bound + 4 records: one per launched block)
  return launch_scan_timed(scan1h_kernel, items_bound ? items_bound : 1u, kS1hWaves, scan1h_lds_bytes(h->ld), st, a);
}

// the matrix-core list scan (prescan.hip.h); timed through the same event ring as launch_ivf_scan
template <int NQ>
int32_t launch_prescan(vers_ivf* h, const IvfSrc<NQ>& src, uint32_t items_bound, uint32_t kp, uint32_t* qflags, uint32_t* quad_ctr,
                       bool shadow, bool hi_only, uint32_t b, hipStream_t st) {
  PreParams p;
  p.rows_bf = shadow ? h->rows_bf.as<uint16_t>() : nullptr;
  p.ld = h->ld;
  p.n_chunks = h->ld / kChunk;
  p.kp = kp;
  p.status = W->st_word();
  p.bounds32 = reinterpret_cast<uint32_t*>(W->partials.as<uint64_t>() + W->ivf_bounds_off);  // 0xFF-initialised with the slots
  p.qflags = qflags;
  p.xnorm = h->xnorm.as<float>();
  p.debug = scan_debug_flags();
  p.metric = (uint32_t)h->metric;
  p.stamps = nullptr;
  if (p.debug & 16u) {
    if (int32_t rc = W->stamps.reserve(512)) return rc;
    VERS_HIP_TRY(hipMemsetAsync(W->stamps.p, 0, 128, st));
    p.stamps = W->stamps.as<unsigned long long>();
  }
  p.next_quad = (p.debug & 32u) ? nullptr : quad_ctr;  // zeroed with the planning tables
  hi_only = hi_only && shadow;
  // Early abandon of tiles whose first columns rule every row out (prescan.hip.h, prune_lower): hi-only query blocks on the shadow,
  // squared L2, rows of at least three steps (one boundary with a step left to save).  option "pre_prune" = 0: every tile is read whole.
  const uint32_t n_steps = h->ld / 64u;
  // (the table's rows must fit LDS beside what the planner chose the block width for: prescan_lds_bytes_g)
  // Not on a sharded handle: a rank holds an eighth of the lists, its launch is short and the lists that are some query's nearest sit
  // mostly on other ranks -- thresholds arrive too late to abandon anything, and the test is not free (profiles/r07_summary.txt).
  const bool prune = hi_only && h->metric == 0 && h->world == 1 && opt_get("pre_prune", 1) != 0 && n_steps >= 3 && n_steps <= kPruneMaxSteps && h->pre_misc.p != nullptr && h->prune_ctr.p != nullptr &&
                     prescan_lds_bytes_g(h->ld, kp, NQ, true, true) <= 160u * 1024u;
  p.prune_tab = nullptr; p.prune_first = 0; p.prune_until = 0; p.prune_om = 0.0f; p.prune_last = nullptr; p.prune_tot = nullptr; p.hot_single = 0u;
  W->prune_last = nullptr;
  W->head_last = nullptr;
  W->ball_last = nullptr;
  // The int8 head (head_filter.hip.h): where tiles are abandoned early and the handle holds a valid head, the scan is THREE launches -- the
  // hot quads, the head's filter over the cold ones, the cold quads the filter left.  option "pre_head" = 0, an invalid head, candidate
  // lists of more than one key per lane or a hand-out switched off for diagnosis: one launch, as ever.
  const uint32_t H = h->head_cols;
  bool head_rest = false;  // the back-off (vers_ivf::head_watch): this batch sits the split out
  if (h->head_watch != nullptr && opt_get("pre_head_backoff", 1) != 0) {
    if (*(volatile uint32_t*)h->head_watch != 0u) {
      *(volatile uint32_t*)h->head_watch = 0u;
      h->head_backoff.store(kHeadBackoff, std::memory_order_relaxed);
    }
    uint32_t left = h->head_backoff.load(std::memory_order_relaxed);
    while (left != 0u && !h->head_backoff.compare_exchange_weak(left, left - 1u, std::memory_order_relaxed)) {}
    head_rest = left != 0u;
  }
  const bool split = prune && !head_rest && opt_get("pre_head", kPreHeadDefault) != 0 && h->head_valid && h->rows_h8.p != nullptr && H >= kHeadMinCols && H <= kHeadMaxCols && H + 64u <= h->ld &&
                     kp <= kPreMaxKp && !(p.debug & 32u) && h->head_ctr.p != nullptr && h->head_watch != nullptr && opt_get("pre_hot_single", 1) != 0;
  // The lists' balls (ball_filter.hip.h): inside a split scan, on a handle that holds valid ones, a fourth launch in front of the head's
  // filter rules cold quads out from the sub-cluster centres alone; the head's filter then walks the quads that are left.  option
  // "pre_ball" = 0 or invalid balls: the three launches as they were.
  const bool balls = split && opt_get("pre_ball", kPreBallDefault) != 0 && h->balls_valid && h->ball_cent.p != nullptr && h->ball_f.p != nullptr && h->ball_cnt.p != nullptr && h->ball_off.p != nullptr &&
                     h->ball_ctr.p != nullptr && h->ld <= kBallMaxLd;
  if (prune) {
    if (int32_t rc = W->prune_tab.reserve((size_t)b * n_steps * sizeof(float))) return rc;
    if (split) {
      if (int32_t rc = W->head_q8.reserve((size_t)b * H)) return rc;
      if (int32_t rc = W->head_q.reserve((size_t)b * 2 * sizeof(float))) return rc;
    }
    if (balls) {
      if (int32_t rc = W->ball_qh.reserve((size_t)b * h->ld * sizeof(uint16_t))) return rc;
      if (int32_t rc = W->ball_q.reserve((size_t)b * 2 * sizeof(float))) return rc;
      if (int32_t rc = W->ball_surv.reserve(((size_t)items_bound / 4 + 1) * sizeof(uint32_t))) return rc;
    }
    hipLaunchKernelGGL(prune_table_kernel, dim3((b + 3) / 4), dim3(256), 0, st, src.qp, src.ldq, h->ld, b, (const uint32_t*)h->pre_misc.as<uint32_t>(),
                       W->prune_tab.as<float>(), split ? H : 0u, split ? W->head_q8.as<int8_t>() : (int8_t*)nullptr, split ? W->head_q.as<float>() : (float*)nullptr,
                       balls ? W->ball_qh.as<uint16_t>() : (uint16_t*)nullptr, balls ? W->ball_q.as<float>() : (float*)nullptr);
    VERS_HIP_TRY(hipGetLastError());
    p.prune_tab = W->prune_tab.as<float>();
    p.prune_first = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(opt_get("pre_prune_first", 2), n_steps));
    p.prune_until = std::max<uint32_t>(p.prune_first, n_steps / 2u);
    p.prune_om = (float)(1.0 - prune_eps(h->ld));  // (rounds to nearest: eps carries a few u of slack for it)
    p.prune_last = quad_ctr + 1;  // (the three words behind the hand-out counter: zeroed with it)
    p.prune_tot = h->prune_ctr.as<unsigned long long>();
    W->prune_last = quad_ctr + 1;
    // the hot lists' quads singly (pre_run_len): only where thresholds can let tiles go.  option "pre_hot_single" = 0: guided runs throughout.
    p.hot_single = opt_get("pre_hot_single", 1) != 0 ? 1u : 0u;
  }
  if (NQ == kPreQWide && !hi_only) return fail(VERS_ERR_INVALID, "internal: 64-query blocks exist on the fp16 shadow with the hi-only query block");
  const size_t lds = prescan_lds_bytes_g(h->ld, kp, NQ, hi_only, prune);
  const bool wide_lists = kp > kPreMaxKp;  // (candidate lists of more than one key per lane: plan_search chose hi-only blocks of 32 or 16 queries on the shadow)
  if (wide_lists && (!hi_only || NQ == kPreQWide || kp > kWideMaxKp)) return fail(VERS_ERR_INVALID, "internal: wide candidate lists need the fp16 shadow with hi-only query blocks of <= 32 queries");
  // (prune: the instantiation that abandons tiles early; without it -- switch off, cosine distance, sharded handle, hi + lo or f32
  // blocks -- the kernel is the one it was before the early abandon existed)
  using Kern = void (*)(IvfSrc<NQ>, PreParams);
  Kern kern;
  if constexpr (NQ == kPreQWide) {
    kern = prune ? (Kern)prescan_kernel_g<true, NQ, IvfSrc<NQ>, false, false, true> : (Kern)prescan_kernel_g<true, NQ, IvfSrc<NQ>, false>;
  } else if (wide_lists) {
    kern = prune ? (Kern)prescan_kernel_g<true, NQ, IvfSrc<NQ>, false, true, true> : (Kern)prescan_kernel_g<true, NQ, IvfSrc<NQ>, false, true>;
  } else if (hi_only) {
    kern = prune ? (Kern)prescan_kernel_g<true, NQ, IvfSrc<NQ>, false, false, true> : (Kern)prescan_kernel_g<true, NQ, IvfSrc<NQ>, false>;
  } else {
    kern = shadow ? (Kern)prescan_kernel_g<true, NQ, IvfSrc<NQ>> : (Kern)prescan_kernel_g<false, NQ, IvfSrc<NQ>>;
  }
  // the grid is the prescan's own: its blocks per CU by its LDS, less the CUs it leaves to the other batches in flight
  const uint32_t per_cu = std::max<uint32_t>(1, std::min<uint32_t>(2, (uint32_t)((160u * 1024u) / lds)));  // 1 at d = 768 (measured: as fast as 2)
  const uint32_t reserve = scan_reserve(h, st);  // (vers_set_option "scan_reserve_cus"; auto: only while another batch is in flight)
  const uint32_t blocks = std::max<uint32_t>(1u, std::min<uint32_t>((items_bound + kWavesPerBlock - 1) / kWavesPerBlock, ((uint32_t)h->n_cu - reserve) * per_cu));
  if (!split) return launch_scan_timed(kern, blocks, kPreWavesG, lds, st, src, p);
  // the split scan: one bracket of the timing ring around all three launches (vers_ivf_scan_times keeps meaning "the list scan")
  HeadParams hp;
  hp.rows_h8 = h->rows_h8.as<int8_t>(); hp.q8 = W->head_q8.as<int8_t>(); hp.qhead = W->head_q.as<float>(); hp.prune_tab = p.prune_tab; hp.xnorm = p.xnorm;
  hp.bounds32 = p.bounds32; hp.misc = h->pre_misc.as<uint32_t>(); hp.H = H; hp.n_steps = n_steps; hp.kp = kp; hp.om = p.prune_om;
  hp.last = quad_ctr + 5;  // (zeroed with the hand-out counters)
  hp.tot = h->head_ctr.as<unsigned long long>();
  hp.done = quad_ctr + 8;
  hp.prune_last = p.prune_last; hp.prune_tot = p.prune_tot;
  hp.watch = h->head_watch;
  hp.surv = nullptr; hp.n_surv = nullptr;
  W->head_last = quad_ctr + 5;
  const uint32_t fblocks = std::max<uint32_t>(1u, std::min<uint32_t>((items_bound + 3u) / 4u, ((uint32_t)h->n_cu - reserve) * 2u));  // (two blocks per compute unit: the kernel is compiled for two waves per SIMD)
  BallParams bp;
  if (balls) {
    bp.cent = h->ball_cent.as<uint16_t>(); bp.ballf = h->ball_f.as<float>(); bp.ball_cnt = h->ball_cnt.as<uint32_t>(); bp.ball_off = h->ball_off.as<uint32_t>();
    bp.qh16 = W->ball_qh.as<uint16_t>(); bp.qball = W->ball_q.as<float>(); bp.bounds32 = p.bounds32;
    bp.ld = h->ld; bp.kp = kp; bp.n_steps = n_steps;
    // the pass engages when the cold region has at least as many quads as the head's filter has blocks: below that the filter is a single
    // round of blocks, its time one block's latency, which a launch in front of it cannot shorten.  option "pre_ball_min_quads" (> 0)
    // replaces the figure (tests on small indexes).
    const int64_t mq = opt_get("pre_ball_min_quads", 0);
    bp.min_quads = mq > 0 ? (uint32_t)std::min<int64_t>(mq, 0x7FFFFFFF) : ((uint32_t)h->n_cu - reserve) * 2u;
    bp.surv = W->ball_surv.as<uint32_t>();
    bp.n_surv = quad_ctr + 9;  // (the three spare words, zeroed with the hand-out counters: survivors | units tested | units dead)
    bp.last = quad_ctr + 10;
    bp.tot = h->ball_ctr.as<unsigned long long>();
    bp.head_last = hp.last; bp.head_tot = hp.tot; bp.prune_last = p.prune_last; bp.prune_tot = p.prune_tot;
    hp.surv = bp.surv; hp.n_surv = bp.n_surv;
    W->ball_last = quad_ctr + 10;
  }
  if (int32_t rc = scan_prepare_launch(kern, lds)) return rc;
  return timed_scan(st, [&]() -> int32_t {
    PreParams ph = p, pc = p;
    ph.hot_single = kPreHotOnly;
    pc.hot_single = kPreColdOnly;
    pc.next_quad = quad_ctr + 4;  // the cold launch's own counter: starts at zero, counts from the first cold quad
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(kWave * kPreWavesG), lds, st, src, ph);
    // a block per cold quad, striding; how many there are is on the device (GroupTotals): the grid is what the CUs hold at once
    if (balls) {  // a block per cold quad, striding: four blocks per compute unit at most
      const uint32_t bblocks = std::max<uint32_t>(1u, std::min<uint32_t>((items_bound + 3u) / 4u, ((uint32_t)h->n_cu - reserve) * 4u));
      hipLaunchKernelGGL((ball_filter_kernel<NQ, IvfSrc<NQ>>), dim3(bblocks), dim3(kWave * kBallWaves), 0, st, src, bp);
    }
    hipLaunchKernelGGL((head_filter_kernel<NQ, IvfSrc<NQ>>), dim3(fblocks), dim3(kWave * kHeadWaves), 0, st, src, hp);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(kWave * kPreWavesG), lds, st, src, pc);
    VERS_HIP_TRY(hipGetLastError());
    return VERS_OK;
  });
}

// The ordered-chain passes of a planned search: 64 result ranks per pass (one pass for top_k <= 64) -- the previous pass's slots and pruning
// bounds reset, `scan(lower)` (this pass's list scan, the caller's: unfiltered records / items, or the filtered kernel), ivf_merge_kernel.
// unfiltered: the call that may run in the reference's own mode (a merge group per (query, list)), publishes a host-pointer single query's
// status with its last merge and starts a noted look-ahead behind its first scan; a filtered call does none of the three.
template <class Scan>
int32_t run_chain_passes(vers_ivf* h, const SearchPlan& s, uint32_t b, uint32_t top_k, uint64_t* out_ids, float* out_dist, uint32_t* out_count, uint64_t* out_keys,
                         bool unfiltered, hipStream_t st, Scan&& scan) {
  const int ref_mode = unfiltered ? s.ref_mode : 0;
  for (uint32_t pass = 0; pass < s.n_pass; ++pass) {
    const uint64_t* lower = pass ? W->lower.as<uint64_t>() : nullptr;
    if (pass) VERS_HIP_TRY(hipMemsetAsync(W->partials.p, 0xFF, s.part_bytes, st));  // slots and pruning bounds of the previous pass
    MergeArgs ma;
    ma.partials = W->partials.as<uint64_t>(); ma.P = s.P; ma.S_max = s.S_max; ma.k_keep = s.k_keep; ma.ref_mode = ref_mode; ma.np = s.np;
    ma.pj_list = s.pj_list; ma.pj_pref = s.pj_pref; ma.pj_take = s.pj_take; ma.list_off = h->slot_off.as<uint32_t>(); ma.row_ids = h->row_ids.as<uint32_t>();
    ma.top_k = top_k; ma.rank0 = pass * (uint32_t)kMaxTopK; ma.out_ids = out_ids; ma.out_dist = out_dist; ma.out_count = out_count; ma.out_keys = out_keys;
    ma.lower_out = s.n_pass > 1 ? W->lower.as<uint64_t>() : (uint64_t*)nullptr;
    if (unfiltered && W->st_host && pass + 1 == s.n_pass) { ma.st_word = W->st_word(); ma.st_host = W->st_host; }
    if (int32_t rc = scan(lower)) return rc;
    if (unfiltered && pass == 0)
      if (int32_t rc = start_pending_ahead(h, st)) return rc;
    // four waves while a wave can hold its share of the slots' heads in registers (4096 slots of a merge group: two tree levels
    // instead of four; same box, single query: 94.2 -> 91.6 us, reference mode 59.0 -> 55.3), sixteen beyond
    const uint64_t slots_per_group = ref_mode ? s.S_max : (uint64_t)s.P * s.S_max;
    if (slots_per_group <= 4096) hipLaunchKernelGGL(ivf_merge_kernel<4>, dim3(b), dim3(kWave * 4), 0, st, ma);
    else hipLaunchKernelGGL(ivf_merge_kernel<kMergeWaves>, dim3(b), dim3(kWave * kMergeWaves), 0, st, ma);
    VERS_HIP_TRY(hipGetLastError());
  }
  return VERS_OK;
}

// search_approximate for b queries.  nprobe == 0: the reference's own semantics (nearest list,
// spill while short; results concatenated per list).  nprobe >= 1: extension, global top-k
// over the nprobe nearest lists.
int32_t search_dev_locked(vers_ivf* h, const float* q_dev, uint64_t ldq_in, uint32_t b, uint32_t top_k, uint32_t nprobe,
                          uint64_t* out_ids, float* out_dist, uint32_t* out_count, uint64_t* out_keys, hipStream_t st) {
  if (b == 0) return VERS_OK;
  if (top_k == 0) {
    VERS_HIP_TRY(hipMemsetAsync(out_count, 0, sizeof(uint32_t) * b, st));
    return VERS_OK;
  }
  if (h->k == 0) return fail(VERS_ERR_INSUFFICIENT, "search on an index without centroids (reference: index out of bounds, ivfflat.rs:169)");
  // The reference's own mode (nprobe = 0: the nearest list, spilling into the next ones while the result is short, ivfflat.rs:166-195) IS
  // nprobe = 1 whenever no list is shorter than top_k -- nothing can spill: the nearest list's top_k by (distance, list position) either
  // way.  The handle knows its shortest list (lists_that_always_suffice: add() only lengthens lists, remove_batch recomputes it), so a BATCH in that mode takes
  // the nprobe path: the matrix-core scan of the fp16 shadow + exact finish instead of the ordered chains over the f32 rows (half the
  // bytes: 1.52 -> 0.7 ms per 1024 queries at cfg3).  Single queries keep the f32 tile-per-block scan (scan1t_kernel: one list is
  // latency-bound, the exact finish would cost more than it saves).  option "ref_as_nprobe1" = 0: the ordered chains (A/B runs).
  const bool ref_as_np1 = opt_get("ref_as_nprobe1", 1) != 0;
  if (nprobe == 0 && ref_as_np1 && out_keys == nullptr && h->world == 1 && b >= pre_min_batch_ref().load(std::memory_order_relaxed) && top_k + kPreMinSlack <= kPreMaxKp &&
      knobs().pre_mode != 0 && h->lists_that_always_suffice(top_k) == 1)
    nprobe = 1;
  // Batches below the matrix-core scan's smallest (2 or 3 queries by default) went to one ordered-chain scan of the f32 rows per (query,
  // list) pair: 204 / 272 us at cfg3.  Since round 5 a single query on the shadow is 66 us: such a batch is its queries one after
  // the other on the stream (the per-call tables are reused in stream order, like consecutive calls on one stream).  Same results.
  if (b > 1 && b < pre_min_batch_ref().load(std::memory_order_relaxed) && nprobe != 0 && std::min<uint32_t>(nprobe, h->k) <= (uint32_t)kMaxTopK &&
      top_k + kPreMinSlack <= kPreMaxKp && knobs().pre_mode != 0 && single_shadow_ref().load(std::memory_order_relaxed) != 0 && shadow_mode() != 0 &&
      !h->shadow_off && h->shadow_valid && h->rows_bf.p != nullptr) {
    int32_t rc = VERS_OK;  // (timed -- scan_events 2 -- like single queries: not at all; two event records per query would be 11 us of a batch of 2)
    for (uint32_t qi = 0; qi < b && rc == VERS_OK; ++qi)
      rc = search_dev_locked(h, q_dev + (uint64_t)qi * ldq_in, ldq_in, 1, top_k, nprobe, out_ids + (uint64_t)qi * top_k, out_dist + (uint64_t)qi * top_k,
                             out_count + qi, out_keys ? out_keys + (uint64_t)qi * top_k : nullptr, st);
    return rc;
  }
  SearchPlan s;
  if (int32_t rc = plan_search(h, q_dev, ldq_in, b, top_k, nprobe, st, s)) return rc;
  const uint32_t P = s.P, kp = s.kp, k_keep = s.k_keep, S_max = s.S_max;
  const int ref_mode = s.ref_mode, QG = s.QG, pre_mode = s.pre_mode;
  const bool one1 = s.one1, one1_pre = s.one1_pre, use_pre = s.use_pre, use_shadow = s.use_shadow, hi_only = s.pre_hi_only && !s.one1_pre;
  const uint64_t items_bound = s.items_bound;
  uint32_t *const pj_list = s.pj_list, *const pj_pref = s.pj_pref, *const pj_nq = s.pj_nq, *const quad_ctr = s.quad_ctr;
  uint32_t *const fail_list = s.fail_list, *const qflags = s.qflags;
  GroupTotals* const tot = s.tot;
  const float* const qp = s.qp;
  SearchWs::CoarseAhead* const took = s.took;
  const uint32_t bound_per_pair = ref_mode ? 1u : 0u;
  if (use_pre) {
    // partial lists of the exact re-scan (fail_list [b] + its count, qflags [n_pj]: in the zeroed zone above)
    uint32_t fb_blocks = kFallbackBlocks;  // (a power of two; fewer when P x top_k is large: at most 32 MB of partial lists)
    if (b == 1) fb_blocks = 32;  // (a single query: the launch that almost always finds nothing to do costs 4.3 us with 128 blocks of 16 waves to dispatch; a list per block when it does)
    while (fb_blocks > 16 && fallback_part_keys(fb_blocks, P, top_k) * sizeof(uint64_t) > (size_t(32) << 20)) fb_blocks /= 2;
    if (int32_t rc2 = W->fb_part.reserve(fallback_part_keys(fb_blocks, P, top_k) * sizeof(uint64_t))) return rc2;
    if (!W->fb_ctr.p) {  // group counters of fallback_kernel: zero once, the kernel leaves them zero
      if (int32_t rc2 = W->fb_ctr.reserve((2 * kFallbackBlocks + 1) * sizeof(uint32_t))) return rc2;
      VERS_HIP_TRY(hipMemsetAsync(W->fb_ctr.p, 0, (2 * kFallbackBlocks + 1) * sizeof(uint32_t), st));
    }
    if (one1_pre) {  // a single query: its records (plan1_block) against the shadow, a block each
      Scan1hArgs sa;
      sa.rows_h = h->rows_bf.as<uint16_t>(); sa.xnorm = h->xnorm.as<float>(); sa.recs = W->items.as<Item1Rec>(); sa.n_items_dev = &tot->n_items; sa.qp = qp;
      sa.partials = W->partials.as<uint64_t>(); sa.qflags = qflags; sa.ld = h->ld; sa.kp = kp; sa.metric = (uint32_t)h->metric;
      if (int32_t rc2 = launch_scan1h(h, sa, (uint32_t)items_bound, st)) return rc2;
    } else {
      // (plan_search chose QG: 64 queries per block on the shadow with the query block as fp16 hi only, 16 where rows are too long for a 32-query block)
      if (int32_t rc2 = with_qg<kPreQWide, kPreQNarrow, kPreQ>(QG, [&](auto qg) -> int32_t {
            return launch_prescan(h, make_ivf_src<decltype(qg)::value>(h, s, bound_per_pair), (uint32_t)items_bound, kp, qflags, quad_ctr, use_shadow, hi_only, b, st);
          })) return rc2;
    }
    if (int32_t rc2 = start_pending_ahead(h, st)) return rc2;  // the next batch's coarse quantiser: under this batch's exact finish
    RescoreArgs a;
    a.partials = W->partials.as<uint64_t>(); a.P = P; a.S_max = S_max; a.kp = kp; a.top_k = top_k; a.d_pad = h->ld;
    a.pj_list = pj_list; a.pj_pref = pj_pref; a.pj_nq = pj_nq; a.list_off = h->slot_off.as<uint32_t>(); a.row_ids = h->row_ids.as<uint32_t>();
    a.rows = h->rows.as<float>(); a.rows_rm = h->rows_rm.as<float>(); a.ld = h->ld; a.qp = qp; a.ldq = h->ldq; a.xmax2_bits = h->pre_misc.as<uint32_t>();
    a.qflags = qflags; a.metric = h->metric; a.force_fail = pre_mode == 2; a.shadow = use_shadow ? (hi_only ? 2 : 1) : 0; a.debug = scan_debug_flags(); a.fail_list = fail_list; a.stats = h->pre_misc.as<uint32_t>() + 1;  // (shadow: scan1h_kernel multiplies by the f32 query itself -- no split remainder to charge; code 1 is held to that value by value in tests/test_certificate_single_gpu.py, derivation in single.hip.h)
    a.status = W->st_word(); a.out_ids = out_ids; a.out_dist = out_dist; a.out_count = out_count; a.out_keys = out_keys;
    a.stamps = (scan_debug_flags() & 16u) && W->stamps.p ? W->stamps.as<unsigned long long>() : nullptr;
    if (W->st_host) { a.st_word = W->st_word(); a.st_host = W->st_host; }  // (host-pointer single-query call: the finish publishes when it certifies)
    const int rs_waves = one1_pre ? kRescoreWaves1 : kRescoreWaves;  // (one query: sixteen waves merge its ~250 slots and walk its survivors' chains in one pass)
    const int stage_rows = rescore_lds_bytes(h->ld, true, rs_waves) <= 144u * 1024u ? 1 : 0;
    const size_t rs_lds = rescore_lds_bytes(h->ld, stage_rows != 0, rs_waves);
    if (kp > kPreMaxKp) {  // wide candidate lists (results of 49 .. 200 keys): four keys per lane through the finish (finish_wide.hip.h)
      const size_t w_lds = rescore_wide_lds_bytes(h->ld);
      if (int32_t rc2 = scan_prepare_launch(ivf_rescore_wide_kernel, w_lds)) return rc2;
      hipLaunchKernelGGL(ivf_rescore_wide_kernel, dim3(b), dim3(kWave * kWideWaves), w_lds, st, a);
    } else if (one1_pre) {
      if (int32_t rc2 = scan_prepare_launch(ivf_rescore_kernel<kRescoreWaves1>, rs_lds)) return rc2;
      hipLaunchKernelGGL(ivf_rescore_kernel<kRescoreWaves1>, dim3(b), dim3(kWave * kRescoreWaves1), rs_lds, st, a, stage_rows);
    } else {
      if (int32_t rc2 = scan_prepare_launch(ivf_rescore_kernel<kRescoreWaves>, rs_lds)) return rc2;
      hipLaunchKernelGGL(ivf_rescore_kernel<kRescoreWaves>, dim3(b), dim3(kWave * kRescoreWaves), rs_lds, st, a, stage_rows);
    }
    VERS_HIP_TRY(hipGetLastError());
    if (W->ev_on) {  // (measurement hook vers_ivf_last_finish_ms: from the scan's end record to here)
      VERS_HIP_TRY(hipEventRecord(W->evf, st));
      W->evf_valid = true;
      W->evf_slot = (uint32_t)((W->ev_count - 1) % SearchWs::kEvRing);
    }
    hipLaunchKernelGGL(fallback_kernel, dim3(fb_blocks), dim3(kWave * kFbWaves), 0, st, a, (const uint32_t*)h->slot_len.as<uint32_t>(),
                       (const uint32_t*)fail_list, (const uint32_t*)(fail_list + b), W->fb_part.as<uint64_t>(), W->fb_ctr.as<uint32_t>(),
                       use_shadow ? h->fail_watch : (uint32_t*)nullptr, (const uint32_t*)W->st_word(), W->st_host);  // (st_host: host-pointer single-query call)
    VERS_HIP_TRY(hipGetLastError());
    W->last_pre.valid = true; W->last_pre.b = b; W->last_pre.P = P; W->last_pre.S_max = S_max; W->last_pre.kp = kp; W->last_pre.top_k = top_k;
    W->last_pre.qp = qp; W->last_pre.shadow = use_shadow ? (hi_only ? 2 : 1) : 0;
    if (use_shadow) h->shadow_queries += b;  // (fallback_kernel writes the running failure count to the pinned watch word)
    h->pre_batches += 1;
    W->tot_valid = true;
    if (took) { VERS_HIP_TRY(hipEventRecord(took->freed, st)); took->freed_rec = true; }
    return VERS_OK;
  }
  if (int32_t rc = run_chain_passes(h, s, b, top_k, out_ids, out_dist, out_count, out_keys, /*unfiltered=*/true, st, [&](const uint64_t* lower) -> int32_t {
        if (one1) {  // the single query's items are records (plan1_block)
          Scan1Args sa;
          sa.rows = h->rows.as<float>(); sa.recs = W->items.as<Item1Rec>(); sa.n_items_dev = &tot->n_items; sa.qp = qp;
          sa.partials = W->partials.as<uint64_t>(); sa.k_keep = k_keep; sa.S_max = S_max; sa.bound_per_pair = bound_per_pair;
          const bool few_tiles = ref_mode || (uint64_t)P * (h->n_total / std::max<uint32_t>(1, h->k)) / kWave <= 2ull * (uint64_t)h->n_cu;
          return launch_scan1(h, sa, (uint32_t)items_bound, st, lower, few_tiles);
        }
        return with_qg<1, 8, 16>(QG, [&](auto qg) -> int32_t {
          return launch_ivf_scan(h, make_ivf_src<decltype(qg)::value>(h, s, bound_per_pair), (uint32_t)items_bound, st, lower);
        });
      })) return rc;
  W->tot_valid = true;
  if (took) { VERS_HIP_TRY(hipEventRecord(took->freed, st)); took->freed_rec = true; }
  return VERS_OK;
}

// ---- filtered top-k search (filter.hip.h): a bitmap of allowed vec ids per call = a virtual removal of the others -------------------
// the call's zeroed counters, for either filtered kernel: the call's four | a slot of four words per wave a filtered scan can launch
static int32_t filter_counters_begin(vers_ivf* h, hipStream_t st, unsigned long long*& stats, unsigned long long*& wave_slots) {
  { const int ev = scan_events_ref().load(); W->ev_on = ev == 1 || ev == 2; }
  const size_t stat_words = kFltStats + filter_wave_slots(h) * 4;
  if (int32_t rc = W->flt_stats.reserve(stat_words * sizeof(unsigned long long))) return rc;
  {
    std::lock_guard<std::mutex> lk(h->flt_mu);
    if (!h->flt_total.p) {
      if (int32_t rc = h->flt_total.reserve(kFltStats * sizeof(unsigned long long))) return rc;
      VERS_HIP_TRY(hipMemset(h->flt_total.p, 0, kFltStats * sizeof(unsigned long long)));
    }
  }
  VERS_HIP_TRY(hipMemsetAsync(W->flt_stats.p, 0, stat_words * sizeof(unsigned long long), st));
  stats = W->flt_stats.as<unsigned long long>();
  wave_slots = stats + kFltStats;
  return VERS_OK;
}

// ---- prepared filters (filter_prepared.hip.h): whose arrays a filtered call reads ----
// A full build of the forms asked for into the object's arrays, on `st`: the mask kernels and the count kernel of the per-call path.  recount:
// allowed_len and the total are rebuilt with them (a stale object); else a form is built BESIDE a fresh one (a one-bitmap object's second
// form), whose counts hold already -- the mask kernel's count then goes to the spare counters, so that a search on another stream never
// reads a total in the making.
static int32_t prepared_build(vers_ivf* h, vers_filter* o, bool one, bool multi, bool recount, uint64_t n_rows, hipStream_t st) {
  const uint64_t n_tiles = (n_rows + kWave - 1) / kWave;
  const size_t tile_bytes = std::max<size_t>(1, n_tiles) * sizeof(uint64_t), row_bytes = tile_bytes * kWave;
  if (one)
    if (int32_t rc = o->tile_mask.reserve(tile_bytes)) return rc;
  if (multi) {
    if (int32_t rc = o->tile_sets.reserve(tile_bytes)) return rc;
    if (int32_t rc = o->row_sets.reserve(row_bytes)) return rc;
  }
  if (int32_t rc = o->stats.reserve(2 * kFltStats * sizeof(unsigned long long))) return rc;
  if (recount)
    if (int32_t rc = o->alen.reserve(std::max<size_t>(1, (size_t)o->n_filters * h->k) * sizeof(uint32_t))) return rc;
  unsigned long long* const sink = o->stats.as<unsigned long long>() + (recount ? 0 : kFltStats);
  const bool empty = o->n_bits == 0 || n_tiles == 0;  // nothing is allowed
  const uint64_t blocks = std::min<uint64_t>((uint64_t)h->n_cu, (n_tiles + kFltMaskThreads / kWave - 1) / (kFltMaskThreads / kWave));
  if (one) {
    VERS_HIP_TRY(hipMemsetAsync(sink, 0, kFltStats * sizeof(unsigned long long), st));
    if (empty) VERS_HIP_TRY(hipMemsetAsync(o->tile_mask.p, 0, tile_bytes, st));
    else
      hipLaunchKernelGGL(filter_tile_mask_kernel, dim3((unsigned)blocks), dim3(kFltMaskThreads), 0, st, (const uint32_t*)h->row_ids.as<uint32_t>(), n_rows,
                         (const uint64_t*)o->bits.as<uint64_t>(), o->n_bits, o->tile_mask.as<uint64_t>(), sink);
    VERS_HIP_TRY(hipGetLastError());
  }
  if (multi) {
    VERS_HIP_TRY(hipMemsetAsync(sink, 0, kFltStats * sizeof(unsigned long long), st));  // (both forms of one bitmap count the same rows)
    if (empty) {
      VERS_HIP_TRY(hipMemsetAsync(o->tile_sets.p, 0, tile_bytes, st));
      VERS_HIP_TRY(hipMemsetAsync(o->row_sets.p, 0, row_bytes, st));
    } else {
      hipLaunchKernelGGL(filter_multi_mask_kernel, dim3((unsigned)blocks), dim3(kFltMaskThreads), 0, st, (const uint32_t*)h->row_ids.as<uint32_t>(), n_rows,
                         (const uint64_t*)o->bits.as<uint64_t>(), o->words, o->n_filters, o->n_bits, o->row_sets.as<uint64_t>(), o->tile_sets.as<uint64_t>(), sink);
      VERS_HIP_TRY(hipGetLastError());
    }
  }
  if (recount && h->k != 0) {
    const uint32_t cblocks = (h->k + kAdpThreads / kWave - 1) / (kAdpThreads / kWave);
    const uint8_t* owner = h->world > 1 ? h->owner.as<uint8_t>() : (const uint8_t*)nullptr;
    if (multi)
      hipLaunchKernelGGL(filter_multi_allowed_len_kernel, dim3(cblocks), dim3(kAdpThreads), 0, st, (const uint64_t*)o->row_sets.as<uint64_t>(),
                         (const uint64_t*)o->tile_sets.as<uint64_t>(), (const uint32_t*)h->list_off.as<uint32_t>(), (const uint32_t*)h->list_len.as<uint32_t>(), h->k,
                         o->n_filters, o->alen.as<uint32_t>(), owner, h->rank);
    else
      hipLaunchKernelGGL(filter_allowed_len_kernel, dim3(cblocks), dim3(kAdpThreads), 0, st, (const uint64_t*)o->tile_mask.as<uint64_t>(),
                         (const uint32_t*)h->list_off.as<uint32_t>(), (const uint32_t*)h->list_len.as<uint32_t>(), h->k, o->alen.as<uint32_t>(), owner, h->rank);
    VERS_HIP_TRY(hipGetLastError());
  }
  return VERS_OK;
}

// The object brought up to date against the handle on `st`, under the handle's shared lock (the caller's) and the object's mutex (taken here):
// "check, enqueue, record the event" is one critical section.  want: 0 the per-call form, 1 the per-query form, -1 whatever the object holds
// (vers_ivf_filter_refresh).  A rebuild or a tail refresh leaves ONE record in the scan-timing ring of the leased workspace; a call served
// from fresh masks leaves none, and is counted as a hit when it is a search's.
static int32_t prepared_sync(vers_ivf* h, vers_filter* o, int want, bool search, hipStream_t st) {
  std::lock_guard<std::mutex> lk(o->mu);
  const uint64_t n_rows = (h->k == 0 || h->up.open) ? 0 : h->cap_rows;
  // Work queued for the object on ANOTHER stream (a rebuild, a tail refresh, a form's first build) may still be running: whatever this call
  // reads or writes of the object comes behind it, on the device.  Before anything below records `ready` anew.
  if (o->pending && o->ready_stream != st) {
    const hipError_t q = hipEventQuery(o->ready);
    if (q == hipSuccess) o->pending = false;
    else {
      if (q == hipErrorNotReady) (void)hipGetLastError();  // (no error: the query's answer)
      VERS_HIP_TRY(hipStreamWaitEvent(st, o->ready, 0));
    }
  }
  bool stale = !o->built || o->seen_moved != h->flt_moved;
  // A form's first build beside held ones, after in-place appends the object has not seen: the new form would hold the appended rows'
  // bits while allowed_len and the total do not count them yet, and the tail refresh takes its corrections from the words that were there.
  // Rare (a one-bitmap object's second form): everything is rebuilt and recounted, as if rows had moved.
  if (!stale && o->seen_appended != h->flt_appended && ((want == 0 && !o->have_one) || (want == 1 && !o->have_multi))) stale = true;
  const bool one = want == 0 ? (stale || !o->have_one) : (stale && o->have_one);
  const bool multi = want == 1 ? (stale || !o->have_multi) : (stale && o->have_multi);
  auto snapshot = [&]() {
    o->seen_moved = h->flt_moved; o->seen_appended = h->flt_appended; o->snap_n_total = h->n_total;
    o->snap_len.assign(h->h_len.begin(), h->h_len.begin() + std::min<size_t>(h->h_len.size(), h->k));
  };
  auto record = [&]() -> int32_t {
    VERS_HIP_TRY(hipEventRecord(o->ready, st));
    o->ready_stream = st;
    o->pending = true;
    return VERS_OK;
  };
  if (one || multi) {
    if (stale) o->built = false;
    if (int32_t rc = timed_scan(st, [&]() -> int32_t { return prepared_build(h, o, one, multi, stale, n_rows, st); })) {
      if (one) o->have_one = false;
      if (multi) o->have_multi = false;
      return rc;
    }
    o->have_one = o->have_one || one; o->have_multi = o->have_multi || multi;
    if (stale) { snapshot(); o->built = true; }
    o->builds += 1;
    return record();
  }
  if (stale) { snapshot(); o->built = true; }  // (an object that holds no form yet: nothing to rebuild)
  if (o->seen_appended != h->flt_appended) {
    std::vector<TailItem> items;
    if (o->have_one || o->have_multi)
      (void)filter_tail_plan(o->snap_len.data(), h->h_len.data(), h->world > 1 ? h->h_owner.data() : (const uint8_t*)nullptr, h->rank, h->k, o->snap_n_total, o->n_bits, items);
    if (!items.empty()) {
      if (int32_t rc = o->work.reserve(items.size() * sizeof(TailItem))) return rc;
      VERS_HIP_TRY(hipMemcpyAsync(o->work.p, items.data(), items.size() * sizeof(TailItem), hipMemcpyHostToDevice, st));  // (pageable source: copied before the call returns)
      TailArgs a;
      a.items = o->work.as<TailItem>(); a.n_items = (uint32_t)items.size();
      a.row_ids = h->row_ids.as<uint32_t>(); a.list_off = h->list_off.as<uint32_t>(); a.cap_rows = n_rows;
      a.bits = o->bits.as<uint64_t>(); a.stride_words = o->words; a.n_bits = o->n_bits; a.n_filters = o->n_filters;
      a.tile_mask = o->have_one ? o->tile_mask.as<uint64_t>() : (uint64_t*)nullptr;
      a.row_sets = o->have_multi ? o->row_sets.as<uint64_t>() : (uint64_t*)nullptr;
      a.tile_sets = o->have_multi ? o->tile_sets.as<uint64_t>() : (uint64_t*)nullptr;
      a.allowed_len = o->alen.as<uint32_t>(); a.k_lists = h->k;
      a.total = o->stats.as<unsigned long long>() + kFltRowsAllowed;
      if (int32_t rc = timed_scan(st, [&]() -> int32_t {
            hipLaunchKernelGGL(filter_tail_refresh_kernel, dim3((a.n_items + kTailThreads / kWave - 1) / (kTailThreads / kWave)), dim3(kTailThreads), 0, st, a);
            VERS_HIP_TRY(hipGetLastError());
            return VERS_OK;
          })) {
        o->built = false;  // (what the kernel did is not known: the next call rebuilds)
        return rc;
      }
      snapshot();
      o->tails += 1;
      return record();
    }
    snapshot();  // no new row can be allowed, and a slack row's bits were 0 already
  }
  if (search) o->hits += 1;
  return VERS_OK;
}

// The filter of a call, on the device -- what every filtered *_dev_locked function takes: n_filters bitmaps `stride_words` apart, one n_bits for
// all.  filter_of == NULL: ONE bitmap for the batch and the per-call kernels (filter.hip.h, filter_range.hip.h); else the batch's filter_of and
// the per-query kernels (filter_multi.hip.h, filter_range_multi.hip.h).  prep: a prepared call -- the object the bitmaps above are; its masks
// serve the call and no mask kernel runs.
struct FilterArg {
  const uint64_t* filters; uint64_t stride_words; uint32_t n_filters; uint64_t n_bits; const uint32_t* filter_of;
  vers_filter* prep = nullptr;
  // (several bitmaps without a filter_of: vers_ivf_filter_allowed_len_dev, which counts every bitmap and has no batch; the searches refuse that)
  bool multi() const { return filter_of != nullptr || n_filters > 1; }
  uint32_t n_sets() const { return multi() ? n_filters : 1u; }
};
// the per-call entry points' filter: one bitmap of n_bits bits
static FilterArg per_call_filter(const uint64_t* bits, uint64_t n_bits) { return FilterArg{bits, (n_bits + 63) / 64, 1u, n_bits, nullptr}; }
// the prepared calls' filter: the object's own packed copy of the bitmaps, and the object
static FilterArg prepared_filter(const vers_filter* f, const uint32_t* filter_of_dev) {
  return FilterArg{f->bits.as<uint64_t>(), f->words, f->n_filters, f->n_bits, filter_of_dev, const_cast<vers_filter*>(f)};
}

// What filter_begin fills for the kernels of the call: the per-call mask's parameters or the per-query sets', and which of the two.
struct FilterMasks {
  FilterParams one;
  FilterMultiParams multi;
  bool per_query = false;
  FilterChoice choice() const { return per_query ? FilterChoice{nullptr, &multi} : FilterChoice{&one, nullptr}; }
};

// the begin of a prepared call: the object's arrays in the workspace's place, the allowed total from the object
static int32_t prepared_begin(vers_ivf* h, vers_filter* o, bool multi, hipStream_t st, unsigned long long* stats) {
  if (int32_t rc = prepared_sync(h, o, multi ? 1 : 0, true, st)) return rc;
  VERS_HIP_TRY(hipMemcpyAsync(stats + kFltRowsAllowed, o->stats.as<unsigned long long>() + kFltRowsAllowed, sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
  return VERS_OK;
}

// The tile mask of the call over `n_rows` storage rows + its zeroed counters.  The mask kernel is bracketed by a record of the scan-timing
// ring (vers_ivf_scan_times: a filtered call leaves the mask kernel's record, then one per scan pass).
static int32_t filter_one_begin(vers_ivf* h, const FilterArg& a, uint64_t n_rows, hipStream_t st, FilterParams& f) {
  const uint64_t* const bits_dev = a.filters;
  const uint64_t n_bits = a.n_bits;
  const uint64_t n_tiles = (n_rows + kWave - 1) / kWave;
  if (a.prep) {  // a prepared call: no mask kernel, the object's mask
    if (int32_t rc = filter_counters_begin(h, st, f.stats, f.wave_slots)) return rc;
    if (int32_t rc = prepared_begin(h, a.prep, false, st, f.stats)) return rc;
    f.tile_mask = a.prep->tile_mask.as<uint64_t>();
    return VERS_OK;
  }
  if (int32_t rc = W->flt_mask.reserve(std::max<size_t>(1, n_tiles) * sizeof(uint64_t))) return rc;
  if (int32_t rc = filter_counters_begin(h, st, f.stats, f.wave_slots)) return rc;
  f.tile_mask = W->flt_mask.as<uint64_t>();
  return timed_scan(st, [&]() -> int32_t {
    if (n_bits == 0 || n_tiles == 0) {  // the empty filter: nothing is allowed
      VERS_HIP_TRY(hipMemsetAsync(W->flt_mask.p, 0, std::max<size_t>(1, n_tiles) * sizeof(uint64_t), st));
      return VERS_OK;
    }
    const uint64_t blocks = std::min<uint64_t>((uint64_t)h->n_cu, (n_tiles + kFltMaskThreads / kWave - 1) / (kFltMaskThreads / kWave));
    hipLaunchKernelGGL(filter_tile_mask_kernel, dim3((unsigned)blocks), dim3(kFltMaskThreads), 0, st, (const uint32_t*)h->row_ids.as<uint32_t>(), n_rows, bits_dev, n_bits,
                       W->flt_mask.as<uint64_t>(), f.stats);
    VERS_HIP_TRY(hipGetLastError());
    return VERS_OK;
  });
}

// An adaptive call's own arguments (filter_adaptive.hip.h), `on` for the calls that are: the call's nprobe is nprobe_max; out_nprobe is where
// the call's other outputs are (host or device), nullable.
// On a handle sharded by cluster a rank counts the allowed rows of the lists it stores only, and the depth needs every list's:
//   allowed_len  a partial call: the GLOBAL counts [n_filters or 1][k], the caller's (vers_ivf_filter_allowed_len_dev on every rank, summed);
//                the count kernel is not run
//   reduce       a sharded call: told this rank's counts (n words, on `st`), it exchanges them and names the global ones
struct AdaptiveSpec {
  bool on = false;
  uint32_t nprobe_min = 0, min_allowed = 0;
  uint32_t* out_nprobe = nullptr;
  const uint32_t* allowed_len = nullptr;
  std::function<int32_t(const uint32_t* local, size_t n, const uint32_t*& global, hipStream_t st)> reduce;
};
static AdaptiveSpec adaptive_spec(uint32_t nprobe_min, uint32_t min_allowed, uint32_t* out_nprobe, const uint32_t* allowed_len = nullptr) {
  AdaptiveSpec as;
  as.on = true; as.nprobe_min = nprobe_min; as.min_allowed = min_allowed; as.out_nprobe = out_nprobe; as.allowed_len = allowed_len;
  return as;
}
static AdaptiveSpec adaptive_spec(const vers_adaptive_t* ad) {  // (NULL: plain depth)
  return ad ? adaptive_spec(ad->nprobe_min, ad->min_allowed, ad->out_nprobe_dev, ad->allowed_len_dev) : AdaptiveSpec{};
}

// allowed_len[f * k + L] of the call's mask(s) into `out` ([n_sets][k]): a record of the scan-timing ring of its own.  On a sharded handle the
// lists this rank stores, 0 for the others (filter_adaptive.hip.h).
static int32_t filter_count_allowed(vers_ivf* h, const FilterMasks& m, uint32_t n_sets, uint32_t* out, hipStream_t st) {
  return timed_scan(st, [&]() -> int32_t {
    if (h->k == 0) return VERS_OK;
    const uint32_t blocks = (h->k + kAdpThreads / kWave - 1) / (kAdpThreads / kWave);
    const uint8_t* owner = h->world > 1 ? h->owner.as<uint8_t>() : (const uint8_t*)nullptr;
    if (m.per_query)
      hipLaunchKernelGGL(filter_multi_allowed_len_kernel, dim3(blocks), dim3(kAdpThreads), 0, st, m.multi.row_sets, m.multi.tile_sets, (const uint32_t*)h->list_off.as<uint32_t>(),
                         (const uint32_t*)h->list_len.as<uint32_t>(), h->k, n_sets, out, owner, h->rank);
    else
      hipLaunchKernelGGL(filter_allowed_len_kernel, dim3(blocks), dim3(kAdpThreads), 0, st, m.one.tile_mask, (const uint32_t*)h->list_off.as<uint32_t>(),
                         (const uint32_t*)h->list_len.as<uint32_t>(), h->k, out, owner, h->rank);
    VERS_HIP_TRY(hipGetLastError());
    return VERS_OK;
  });
}

// filter_one_begin's twin for a filter per query: row_sets (8 bytes per storage row, whole tiles) and tile_sets (in the per-call mask's buffer)
// over `n_rows` storage rows + the zeroed counters; the mask kernel inside the same bracket of the scan-timing ring.
static int32_t filter_multi_begin(vers_ivf* h, const FilterArg& ms, uint64_t n_rows, hipStream_t st, FilterMultiParams& f) {
  const uint64_t* const filters_dev = ms.filters;
  const uint64_t n_bits = ms.n_bits;
  const uint64_t n_tiles = (n_rows + kWave - 1) / kWave;
  const size_t tile_bytes = std::max<size_t>(1, n_tiles) * sizeof(uint64_t), row_bytes = tile_bytes * kWave;
  if (ms.prep) {  // a prepared call: no mask kernel, the object's sets
    if (int32_t rc = filter_counters_begin(h, st, f.stats, f.wave_slots)) return rc;
    if (int32_t rc = prepared_begin(h, ms.prep, true, st, f.stats)) return rc;
    f.tile_sets = ms.prep->tile_sets.as<uint64_t>();
    f.row_sets = ms.prep->row_sets.as<uint64_t>();
    f.filter_of = ms.filter_of;
    f.n_filters = ms.n_filters;
    return VERS_OK;
  }
  if (int32_t rc = W->flt_mask.reserve(tile_bytes)) return rc;
  if (int32_t rc = W->flt_rows.reserve(row_bytes)) return rc;
  if (int32_t rc = filter_counters_begin(h, st, f.stats, f.wave_slots)) return rc;
  f.tile_sets = W->flt_mask.as<uint64_t>();
  f.row_sets = W->flt_rows.as<uint64_t>();
  f.filter_of = ms.filter_of;
  f.n_filters = ms.n_filters;
  return timed_scan(st, [&]() -> int32_t {
    if (n_bits == 0 || n_tiles == 0) {  // every filter is empty: nothing is allowed
      VERS_HIP_TRY(hipMemsetAsync(W->flt_mask.p, 0, tile_bytes, st));
      VERS_HIP_TRY(hipMemsetAsync(W->flt_rows.p, 0, row_bytes, st));
      return VERS_OK;
    }
    const uint64_t blocks = std::min<uint64_t>((uint64_t)h->n_cu, (n_tiles + kFltMaskThreads / kWave - 1) / (kFltMaskThreads / kWave));
    hipLaunchKernelGGL(filter_multi_mask_kernel, dim3((unsigned)blocks), dim3(kFltMaskThreads), 0, st, (const uint32_t*)h->row_ids.as<uint32_t>(), n_rows, filters_dev,
                       ms.stride_words, ms.n_filters, n_bits, W->flt_rows.as<uint64_t>(), W->flt_mask.as<uint64_t>(), f.stats);
    VERS_HIP_TRY(hipGetLastError());
    return VERS_OK;
  });
}

// the masks of the call's filter over `n_rows` storage rows, in the form the filter asks for
static int32_t filter_begin(vers_ivf* h, const FilterArg& a, uint64_t n_rows, hipStream_t st, FilterMasks& m) {
  m.per_query = a.multi();
  return m.per_query ? filter_multi_begin(h, a, n_rows, st, m.multi) : filter_one_begin(h, a, n_rows, st, m.one);
}
// the rows an exhaustive filtered scan covers: none on an index without centroids (a streamed upload in progress included)
static uint64_t stored_rows(const vers_ivf* h) { return (h->k == 0 || h->up.open) ? 0 : h->cap_rows; }

// the call's counters into the handle's totals, and the workspace noted for vers_ivf_filter_stats
static int32_t filter_end(vers_ivf* h, hipStream_t st) {
  hipLaunchKernelGGL(filter_stats_fold_kernel, dim3(1), dim3(kFltFoldThreads), 0, st, (const unsigned long long*)(W->flt_stats.as<unsigned long long>() + kFltStats),
                     (uint32_t)filter_wave_slots(h), W->flt_stats.as<unsigned long long>(), h->flt_total.as<unsigned long long>());
  VERS_HIP_TRY(hipGetLastError());
  std::lock_guard<std::mutex> lk(h->pool_mu);
  h->flt_last = W;
  return VERS_OK;
}

// launch_seg_scan's filtered twin -- no bounds, no counter either -- but timed through the scan-timing ring, and no more waves than counter slots
template <int QG>
int32_t launch_filter_seg_scan(vers_ivf* h, const SegSrc<QG, true>& src, uint32_t n_items, int metric, FilterChoice f, hipStream_t st,
                               const uint64_t* lower) {
  const ScanParams p = ivf_scan_params(h, src.k, lower);
  const uint32_t blocks = scan_grid(h->n_cu, QG, h->ld, n_items, (uint32_t)(filter_wave_slots(h) / kWavesPerBlock));
  return with_metric(metric, [&](auto m) -> int32_t {
    if (f.multi)
      return launch_scan_timed(filter_multi_scan_kernel<QG, decltype(m)::value, SegSrc<QG, true>>, blocks, kWavesPerBlock, scan_lds_bytes(QG, h->ld), st, src, p, *f.multi);
    return launch_scan_timed(filter_scan_kernel<QG, decltype(m)::value, SegSrc<QG, true>>, blocks, kWavesPerBlock, scan_lds_bytes(QG, h->ld), st, src, p, *f.one);
  });
}

// The exhaustive top-k scan (utils.rs:68-82 on the stored rows) of the first `n_rows` storage rows: queries staged by group, segment items,
// per pass of 64 result ranks the segment scan and seg_merge_kernel (seq == vec id already).  What its two callers do differently is theirs
// to say:
//   n_rows          the unfiltered call always scans cap_rows; the filtered one scans an index without centroids as zero rows
//   fixed_seg_rows  option "seg_rows", which only the filtered call honours (0: segments sized for one item per resident wave)
//   flt             the filtered kernel, timed; refuses a batch whose slots do not fit 32 bits (the unfiltered call never has); resets the
//                   slots per pass, since a segment without an allowed row writes nothing and its slots must read as empty
static int32_t run_exhaustive_passes(vers_ivf* h, const float* q_dev, uint64_t ldq_in, uint32_t b, uint32_t top_k, uint32_t metric, uint64_t n_rows,
                                     int64_t fixed_seg_rows, FilterChoice flt, uint64_t* out_ids, float* out_dist, uint32_t* out_count, hipStream_t st) {
  const SegPlan sp = seg_plan(n_rows, b, h->ld, h->n_cu, fixed_seg_rows);
  if (int32_t rc = W->qil.reserve((size_t)sp.n_qg * h->ldq * sp.QG * sizeof(float))) return rc;
  if (int32_t rc = launch_stage_queries(q_dev, ldq_in, h->d, W->qil.as<float>(), h->ldq, b, sp.QG, st)) return rc;
  if (flt && sp.too_large) return fail(VERS_ERR_INVALID, "vers_ivf_search_exhaustive_filtered: batch too large (query x segment slots); split the batch");
  const uint32_t k_w = std::min<uint32_t>(top_k, kMaxTopK);  // one key per lane; wider results: 64 ranks per pass (utils.rs:68-82 has no cap)
  const size_t xpart_bytes = (size_t)b * sp.n_segs * k_w * sizeof(uint64_t);
  if (int32_t rc = W->xpart.reserve(xpart_bytes)) return rc;
  if (top_k > (uint32_t)kMaxTopK)
    if (int32_t rc = W->lower.reserve((size_t)b * sizeof(uint64_t))) return rc;
  uint64_t* const lower_out = top_k > (uint32_t)kMaxTopK ? W->lower.as<uint64_t>() : (uint64_t*)nullptr;
  // (a pass past the last stored row finds nothing; 64-bit rank: no wrap near 2^32)
  for (uint64_t rank0 = 0; rank0 < top_k && (rank0 == 0 || rank0 < n_rows); rank0 += kMaxTopK) {
    const uint32_t k_pass = (uint32_t)std::min<uint64_t>(kMaxTopK, top_k - rank0);
    const uint64_t* lower = rank0 ? W->lower.as<uint64_t>() : nullptr;
    if (flt) VERS_HIP_TRY(hipMemsetAsync(W->xpart.p, 0xFF, xpart_bytes, st));
    if (int32_t rc = with_qg<1, 8>(sp.QG, [&](auto qg) -> int32_t {
          using Src = SegSrc<decltype(qg)::value, true>;
          const Src src = make_seg_src<Src>(h->rows.as<float>(), n_rows, h->ld, sp, W->qil.as<float>(), h->ldq, b, W->xpart.as<uint64_t>(), k_pass, h->row_ids.as<uint32_t>());
          return flt ? launch_filter_seg_scan(h, src, sp.n_items, (int)metric, flt, st, lower) : launch_seg_scan(h, src, sp.n_items, (int)metric, st, lower);
        })) return rc;
    hipLaunchKernelGGL(seg_merge_kernel, dim3(b), dim3(kWave * kMergeWaves), 0, st, W->xpart.as<uint64_t>(), sp.n_segs, k_pass, top_k, (uint32_t)rank0, out_ids,
                       out_dist, out_count, lower_out);
    VERS_HIP_TRY(hipGetLastError());
  }
  return VERS_OK;
}

int32_t exhaustive_dev_locked(vers_ivf* h, const float* q_dev, uint64_t ldq_in, uint32_t b, uint32_t top_k, uint32_t metric,
                              uint64_t* out_ids, float* out_dist, uint32_t* out_count, hipStream_t st) {
  if (b == 0) return VERS_OK;
  if (top_k == 0) {
    VERS_HIP_TRY(hipMemsetAsync(out_count, 0, sizeof(uint32_t) * b, st));
    return VERS_OK;
  }
  return run_exhaustive_passes(h, q_dev, ldq_in, b, top_k, metric, h->cap_rows, 0, FilterChoice{}, out_ids, out_dist, out_count, st);
}

// Filtered search over the min(nprobe, k) nearest lists, nprobe >= 1: mask kernel, the plan of the ordered-chain scan (the lists are ranked as
// without a filter: the centroids do not depend on it), per pass the filtered scan, ivf_merge_kernel as it is.  The caller has checked nprobe,
// the handle's sharding and its centroids.  flt says which mask kernel and which scan kernel (FilterArg); everything else is the same.
// adaptive: nprobe is nprobe_max and every query probes to its own depth (filter_adaptive.hip.h) -- behind the mask kernel the allowed rows
// per list are counted (a record of the scan-timing ring of its own, between the mask's and the passes'), and the plan is the adaptive one.
int32_t filtered_dev_locked(vers_ivf* h, const float* q_dev, uint64_t ldq_in, uint32_t b, uint32_t top_k, uint32_t nprobe, const FilterArg& flt, const AdaptiveSpec& adaptive,
                            uint64_t* out_ids, float* out_dist, uint32_t* out_count, hipStream_t st, uint64_t* out_keys = nullptr) {
  // out_keys: a rank's PARTIAL (search_dev_locked's: the merge stores the keys beside the ids, kKeyMax padded); top_k >= 1 then.  The handle
  // may be sharded by cluster: the plan scans the lists this rank stores, sequence numbers run over the global lengths.
  if (b == 0) return VERS_OK;
  if (top_k == 0) {
    VERS_HIP_TRY(hipMemsetAsync(out_count, 0, sizeof(uint32_t) * b, st));
    if (adaptive.on && adaptive.out_nprobe) VERS_HIP_TRY(hipMemsetAsync(adaptive.out_nprobe, 0, sizeof(uint32_t) * b, st));  // (nothing is probed)
    return VERS_OK;
  }
  FilterMasks masks;
  if (int32_t rc = filter_begin(h, flt, h->cap_rows, st, masks)) return rc;
  AdaptiveQ aq;
  if (adaptive.on) {
    const uint32_t n_sets = flt.n_sets();
    aq.p_min = std::min<uint32_t>(adaptive.nprobe_min, h->k); aq.min_allowed = adaptive.min_allowed; aq.allowed_len = adaptive.allowed_len;
    aq.filter_of = flt.filter_of; aq.n_filters = n_sets; aq.out_nprobe = adaptive.out_nprobe;
    if (aq.allowed_len == nullptr) {  // (a partial call brings the global counts: nothing to count)
      const uint32_t* counts = flt.prep ? flt.prep->alen.as<uint32_t>() : (const uint32_t*)nullptr;  // (a prepared call: the object has them, kept with its masks)
      if (counts == nullptr) {
        if (int32_t rc = W->flt_alen.reserve((size_t)n_sets * h->k * sizeof(uint32_t))) return rc;
        if (int32_t rc = filter_count_allowed(h, masks, n_sets, W->flt_alen.as<uint32_t>(), st)) return rc;
        counts = W->flt_alen.as<uint32_t>();
      }
      aq.allowed_len = counts;
      if (adaptive.reduce)
        if (int32_t rc = adaptive.reduce(counts, (size_t)n_sets * h->k, aq.allowed_len, st)) return rc;
    }
  }
  SearchPlan s;
  W->no_ahead = true;
  const int32_t prc = plan_search(h, q_dev, ldq_in, b, top_k, nprobe, st, s, true, adaptive.on ? &aq : nullptr);
  W->no_ahead = false;
  if (prc) return prc;
  { const int ev = scan_events_ref().load(); W->ev_on = ev == 1 || ev == 2; }  // (the plan set it for an unfiltered call)
  W->tot_valid = true;
  if (int32_t rc = run_chain_passes(h, s, b, top_k, out_ids, out_dist, out_count, out_keys, /*unfiltered=*/false, st, [&](const uint64_t* lower) -> int32_t {
        return with_qg<1, 8, 16>(s.QG, [&](auto qg) -> int32_t {
          return launch_ivf_scan(h, make_ivf_src<decltype(qg)::value>(h, s, 0u), (uint32_t)s.items_bound, st, lower, masks.choice());
        });
      })) return rc;
  return filter_end(h, st);
}

// The exhaustive scan with the filtered kernel: every allowed row that is in a list now, ascending (distance, vec id).  Option "seg_rows" fixes
// the segment length here as it does for the chains.  An index without centroids (a streamed upload in progress included) is scanned as zero
// rows: counts 0.
int32_t exhaustive_filtered_dev_locked(vers_ivf* h, const float* q_dev, uint64_t ldq_in, uint32_t b, uint32_t top_k, uint32_t metric, const FilterArg& flt, uint64_t* out_ids,
                                       float* out_dist, uint32_t* out_count, hipStream_t st, uint64_t* out_keys = nullptr, uint64_t* out_key_ids = nullptr) {
  // out_keys / out_key_ids: a rank's PARTIAL as well -- (distance bits << 32) | vec id beside the ids, kKeyMax padded, packed from the local
  // result (out_ids / out_dist / out_count are then the caller's scratch); top_k >= 1 then
  if (b == 0) return VERS_OK;
  if (top_k == 0) {
    VERS_HIP_TRY(hipMemsetAsync(out_count, 0, sizeof(uint32_t) * b, st));
    return VERS_OK;
  }
  const uint64_t n_rows = stored_rows(h);
  FilterMasks masks;
  if (int32_t rc = filter_begin(h, flt, n_rows, st, masks)) return rc;
  if (int32_t rc = run_exhaustive_passes(h, q_dev, ldq_in, b, top_k, metric, n_rows, knobs().seg_rows, masks.choice(), out_ids, out_dist, out_count, st)) return rc;
  if (out_keys != nullptr) {
    const size_t part = (size_t)b * top_k;
    hipLaunchKernelGGL(pack_exhaustive_keys_kernel, dim3((unsigned)((part + 255) / 256)), dim3(256), 0, st, (const uint64_t*)out_ids, (const float*)out_dist,
                       (const uint32_t*)out_count, b, top_k, out_keys, out_key_ids);
    VERS_HIP_TRY(hipGetLastError());
  }
  return filter_end(h, st);
}

// The local part of a whole (not a rank's partial) filtered top-k call: the probed lists, or every stored row under the metric given in place of nprobe.
static int32_t filtered_topk_locked(vers_ivf* h, bool probed, const float* q_dev, uint64_t ldq_in, uint32_t b, uint32_t top_k, uint32_t nprobe_or_metric, const FilterArg& flt,
                                    const AdaptiveSpec& adaptive, uint64_t* out_ids, float* out_dist, uint32_t* out_count, hipStream_t st) {
  if (probed) return filtered_dev_locked(h, q_dev, ldq_in, b, top_k, nprobe_or_metric, flt, adaptive, out_ids, out_dist, out_count, st);
  return exhaustive_filtered_dev_locked(h, q_dev, ldq_in, b, top_k, nprobe_or_metric, flt, out_ids, out_dist, out_count, st);
}

// ---- what the filtered calls refuse before they touch the device: ONE check, told what differs between them ----
//   form         how the call takes its filter: one bitmap (kPerCall); the _multi form, where a NULL filter_of is an error (kMulti); the _multi
//                form of the shard and prepared calls, where a NULL filter_of means one bitmap for the batch and needs n_filters == 1 (kEither)
//   sharded_use  the sentence that names the calls to use on a handle sharded by cluster, which this call then refuses; NULL: the call serves a
//                rank (the _partial, _sharded and _prepared calls).  Such a call has no walk order on stored rows: storage order has no key
//                the ranks share.
// Where several refusals apply the first in this order is reported: flags (and walk order), n_filters == 0, VERS_FILTER_MAX, filter_of,
// stride, NULL bitmap, nprobe, sharded handle, no centroids -- except that the _multi range calls test the flags behind their own four.
// b == 0 passes without bitmaps or filter_of: the top-k calls check before they return for an empty batch.
enum class FilterForm { kPerCall, kMulti, kEither };
struct FilterCheck {
  bool probed, range;
  FilterForm form;
  const char* sharded_use;
};
static const char* const kUseShardedTopk = ": the handle is sharded by cluster; filtered search on a sharded handle is out of scope for this call (use vers_ivf_search_filtered_sharded_dev / vers_ivf_search_exhaustive_filtered_sharded_dev, or the _filtered_partial_dev calls + vers_topk_merge_dev)";
static const char* const kUseShardedRange = ": the handle is sharded by cluster; filtered range search on a sharded handle is out of scope for this call (use vers_ivf_range_search_filtered_sharded_dev / vers_ivf_range_search_exhaustive_filtered_sharded_dev, or the _filtered_partial_dev calls + vers_range_merge_dev)";
static int32_t filtered_check(vers_ivf* h, const char* who, const FilterCheck& c, uint32_t nprobe, uint32_t flags, uint32_t b, const FilterArg& f) {
  auto bad = [&](const char* what) -> int32_t { return fail(VERS_ERR_INVALID, std::string(who) + what); };
  auto flags_ok = [&]() -> int32_t {
    if (flags & ~VERS_RANGE_WALK_ORDER) return bad(": unknown flag bits");
    if (c.sharded_use == nullptr && !c.probed && (flags & VERS_RANGE_WALK_ORDER))
      return bad(": no walk order across ranks (storage order has no key the ranks share); use the default order");
    return VERS_OK;
  };
  const bool flags_late = c.form == FilterForm::kMulti;
  if (c.range && !flags_late)
    if (int32_t rc = flags_ok()) return rc;
  if (c.form != FilterForm::kPerCall) {
    if (b != 0 && f.n_filters == 0) return bad(": n_filters == 0");
    if (f.n_filters > VERS_FILTER_MAX) return bad(": more than VERS_FILTER_MAX bitmaps in one call; split the batch by allowed set");
    if (b != 0 && f.filter_of == nullptr) {
      if (c.form == FilterForm::kMulti) return bad(": NULL filter_of");
      if (f.n_filters != 1) return bad(": a NULL filter_of means one bitmap for the batch: n_filters must be 1");
    }
    if (f.n_bits != 0 && f.stride_words < (f.n_bits + 63) / 64) return bad(": filter_stride_words is smaller than ceil(n_bits / 64)");
  }
  if (c.range && flags_late)
    if (int32_t rc = flags_ok()) return rc;
  if (f.n_bits != 0 && f.filters == nullptr) return bad(c.form == FilterForm::kEither ? ": n_bits > 0 with NULL filters" : ": n_bits > 0 with a NULL bitmap");
  if (c.probed && nprobe == 0)
    return bad(c.range ? ": nprobe must be at least 1 (the reference's spill walk is defined by top_k: it has no range meaning)"
                       : ": nprobe must be at least 1 (the reference's spill walk depends on the filtered list lengths: out of scope)");
  if (h->world > 1 && c.sharded_use != nullptr) return bad(c.sharded_use);
  if (c.probed && h->k == 0)
    return fail(VERS_ERR_INSUFFICIENT, c.range ? "range search on an index without centroids (reference: index out of bounds, ivfflat.rs:169)"
                                               : "search on an index without centroids (reference: index out of bounds, ivfflat.rs:169)");
  return VERS_OK;
}

// What the adaptive calls refuse on top of that (filter_adaptive.hip.h), before the handle is locked.  On a handle sharded by cluster the depth
// needs every rank's counts: a partial must bring them, a sharded (or prepared) call exchanges them itself.
enum class AdaptiveKind { kCall, kPartial, kSharded };
static int32_t adaptive_check(const char* who, const AdaptiveSpec& ad, uint32_t nprobe_max, AdaptiveKind kind) {
  if (!ad.on) return VERS_OK;
  auto bad = [&](const char* what) -> int32_t { return fail(VERS_ERR_INVALID, std::string(who) + what); };
  if (ad.nprobe_min == 0) return bad(": nprobe_min must be at least 1");
  if (nprobe_max < ad.nprobe_min) return bad(kind == AdaptiveKind::kCall ? ": nprobe_max is below nprobe_min" : ": nprobe (the adaptive call's nprobe_max) is below nprobe_min");
  if (kind == AdaptiveKind::kPartial && ad.allowed_len == nullptr)
    return bad(": an adaptive partial needs the GLOBAL allowed counts (vers_ivf_filter_allowed_len_dev on every rank, summed)");
  if (kind == AdaptiveKind::kSharded && ad.allowed_len != nullptr) return bad(": allowed_len_dev must be NULL (the call exchanges the counts itself)");
  return VERS_OK;
}

int32_t ensure_out(vers_ivf* h, size_t need, uint32_t b) {
  if (int32_t rc = W->o_ids.reserve(need * sizeof(uint64_t))) return rc;
  if (int32_t rc = W->o_dist.reserve(need * sizeof(float))) return rc;
  return W->o_cnt.reserve((size_t)b * sizeof(uint32_t));
}

int32_t upload_queries(const float* queries, uint64_t stride_bytes, uint32_t b, uint32_t d, DevBuf& buf) {
  if (int32_t rc = buf.reserve((size_t)b * d * sizeof(float))) return rc;
  VERS_HIP_TRY(hipMemcpy2D(buf.p, (size_t)d * 4, queries, stride_bytes, (size_t)d * 4, b, hipMemcpyHostToDevice));
  return VERS_OK;
}

int32_t download_results(vers_ivf* h, uint32_t b, uint32_t top_k, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  const size_t need = (size_t)b * top_k;
  if (need) {
    VERS_HIP_TRY(hipMemcpy(out_ids, W->o_ids.p, need * sizeof(uint64_t), hipMemcpyDeviceToHost));
    VERS_HIP_TRY(hipMemcpy(out_dist, W->o_dist.p, need * sizeof(float), hipMemcpyDeviceToHost));
  }
  VERS_HIP_TRY(hipMemcpy(out_count, W->o_cnt.p, (size_t)b * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return VERS_OK;
}

// ---- host-pointer calls: staged through pinned memory, one synchronisation -----------------------------
struct HostIo {
  bool direct = false;  // single query: the kernels write ids / distances / count / status straight into the pinned block
  size_t q_bytes, ids_off, dist_off, cnt_off, st_off, out_bytes;
  float* q_dev;
  uint64_t* ids_dev;
  float* dist_dev;
  uint32_t* cnt_dev;
};

int32_t host_io_begin(vers_ivf* h, const float* queries, uint64_t stride_bytes, uint32_t b, uint32_t top_k, HostIo& io, bool direct = false) {
  const size_t need = (size_t)b * std::max<uint32_t>(top_k, 1);
  io.q_bytes = (size_t)b * h->d * sizeof(float);
  io.ids_off = 0;
  io.dist_off = need * sizeof(uint64_t);
  io.cnt_off = io.dist_off + need * sizeof(float);
  io.st_off = io.cnt_off + (size_t)b * sizeof(uint32_t);
  io.out_bytes = io.st_off + 16;
  if (!W->io_stream) VERS_HIP_TRY(hipStreamCreateWithFlags(&W->io_stream, hipStreamNonBlocking));
  if (W->used && W->last_stream != W->io_stream) VERS_HIP_TRY(hipStreamWaitEvent(W->io_stream, W->done, 0));
  if (int32_t rc = W->io_q.reserve(io.q_bytes)) return rc;
  if (int32_t rc = W->io_out.reserve(io.out_bytes)) return rc;
  // (a single query's results are written into the pinned block by the merge launch itself -- no memset, no device-to-device
  // and device-to-host copies behind the search: three stream operations of ~4 us each, 124 -> 112 us per call; the query's bytes
  // and the results do not share pinned bytes then.  Letting coarse1_kernel read the QUERY from the pinned block too instead of
  // the H2D copy measured the same: not kept)
  io.direct = direct;
  const size_t q_pin = (io.q_bytes + 63) & ~(size_t)63;
  const size_t pin_need = io.direct ? q_pin + io.out_bytes : std::max(io.q_bytes, io.out_bytes);
  if (pin_need > W->io_pin_cap) {
    if (W->io_pin) (void)hipHostFree(W->io_pin);
    W->io_pin = nullptr; W->io_pin_cap = 0;
    VERS_HIP_TRY(hipHostMalloc(&W->io_pin, pin_need, hipHostMallocDefault));
    W->io_pin_cap = pin_need;
  }
  char* base = io.direct ? (char*)W->io_pin + q_pin : (char*)W->io_out.p;
  io.q_dev = W->io_q.as<float>();
  io.ids_dev = (uint64_t*)(base + io.ids_off);
  io.dist_dev = (float*)(base + io.dist_off);
  io.cnt_dev = (uint32_t*)(base + io.cnt_off);
  for (uint32_t i = 0; i < b; ++i)
    std::memcpy((char*)W->io_pin + (size_t)i * h->d * 4, (const char*)queries + (size_t)i * stride_bytes, (size_t)h->d * 4);
  VERS_HIP_TRY(hipMemcpyAsync(io.q_dev, W->io_pin, io.q_bytes, hipMemcpyHostToDevice, W->io_stream));
  return VERS_OK;
}

// copies results + status word back, waits once, maps the status; *out_status_rc carries kRetrySpill etc.
int32_t host_io_end(vers_ivf* h, const HostIo& io, uint32_t b, uint32_t top_k, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  const char* pin = (const char*)W->io_pin;
  if (io.direct) {
    pin = (const char*)io.ids_dev - io.ids_off;
    // The result block is pinned and its status word is the call's LAST store (system scope, behind a release fence): spin on it for
    // up to 2 ms -- a single query takes ~90 us -- instead of sleeping in hipStreamSynchronize, whose wake-up costs the call several
    // microseconds; a word that stays "not yet" (an error path that launched no merge, a very slow call) falls back to the synchronisation.
    const volatile uint32_t* flag = reinterpret_cast<const volatile uint32_t*>(pin + io.st_off);
    const auto t0 = std::chrono::steady_clock::now();
    bool seen = false;
    for (uint32_t spins = 0; host_spin_ref().load(std::memory_order_relaxed) != 0; ++spins) {
      if (*flag != kStNotYet) { seen = true; break; }
      if ((spins & 255u) == 255u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
      __builtin_ia32_pause();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (!seen) VERS_HIP_TRY(hipStreamSynchronize(W->io_stream));
  } else {
    char* base = (char*)W->io_out.p;
    VERS_HIP_TRY(hipMemcpyAsync(base + io.st_off, W->st_word(), sizeof(uint32_t), hipMemcpyDeviceToDevice, W->io_stream));
    VERS_HIP_TRY(hipMemcpyAsync(W->io_pin, base, io.out_bytes, hipMemcpyDeviceToHost, W->io_stream));
    VERS_HIP_TRY(hipStreamSynchronize(W->io_stream));
  }
  uint32_t s = 0;
  std::memcpy(&s, pin + io.st_off, sizeof(s));
  if (int32_t rc = status_to_rc(h, s, W->st_slot)) return rc;
  const size_t need = (size_t)b * top_k;
  if (need) {
    std::memcpy(out_ids, pin + io.ids_off, need * sizeof(uint64_t));
    std::memcpy(out_dist, pin + io.dist_off, need * sizeof(float));
  }
  std::memcpy(out_count, pin + io.cnt_off, (size_t)b * sizeof(uint32_t));
  return VERS_OK;
}

// ---- range search (range.hip.h) ---------------------------------------------------------------------------------------
constexpr int kRangePhases = 8;
static std::mutex g_rg_mu;
static double g_rg[kRangePhases] = {};  // vers_range_phases: calls, queries, results, plan, count, prefix + total, fill, sort + decode (ms)
}  // namespace ivf
void range_phases_add(uint32_t b, uint64_t total, const float* ms5) {  // (the flat handle's range calls are counted here too: flat.hip)
  std::lock_guard<std::mutex> lk(ivf::g_rg_mu);
  ivf::g_rg[0] += 1.0; ivf::g_rg[1] += (double)b; ivf::g_rg[2] += (double)total;
  for (int i = 0; i < 5; ++i) ivf::g_rg[3 + i] += (double)ms5[i];
}
namespace ivf {

// What the range protocol (range_driver.hip.h: range_search_run) walks on the index.  The caller holds the index shared, a leased workspace
// and status word 1 (HostStatusSlot: the call synchronises and consumes its status itself); a host-pointer call's ids / distances go to the
// workspace's o_ids / o_dist.  The status word maps as every search's does, except that a spill past the ranked lists has no range meaning.
struct IvfRangeSource {
  vers_ivf* h;
  uint32_t ld() const { return h->ld; }
  uint32_t* status() const { return W->st_word(); }
  const uint32_t* row_ids() const { return h->row_ids.as<uint32_t>(); }
  int32_t status_rc(uint32_t word) const {
    const int32_t rc = status_to_rc(h, word, W->st_slot);
    return rc == kRetrySpill ? VERS_ERR_INVALID : rc;
  }
  int32_t own_out(uint64_t total, uint64_t*& ids, float*& dist) const {
    if (int32_t rc = W->o_ids.reserve((size_t)total * sizeof(uint64_t))) return rc;
    if (int32_t rc = W->o_dist.reserve((size_t)total * sizeof(float))) return rc;
    ids = W->o_ids.as<uint64_t>(); dist = W->o_dist.as<float>();
    return VERS_OK;
  }
};

// the rows of the min(nprobe, k) nearest lists: the plan of the ordered-chain scan (IvfSrc<QG> items, slot = pair * S_max + segment).  A partial
// keeps walk order when asked to: ascending sequence number (a sharded rank walks its probes in rank order).
struct ProbedRangeSource : IvfRangeSource {
  static constexpr bool kKeyIds = false, kPartials = true;
  const char* who;
  const float* q_dev; uint64_t ldq_in; uint32_t b, nprobe;
  SearchPlan s;
  bool planned = false;
  ProbedRangeSource(vers_ivf* hh, const char* w, const float* q, uint64_t ldq, uint32_t bb, uint32_t np) : IvfRangeSource{hh}, who(w), q_dev(q), ldq_in(ldq), b(bb), nprobe(np) {}
  hipStream_t st_ = nullptr;
  ~ProbedRangeSource() {  // a look-ahead slot the plan consumed is free again behind whatever the call queued, on EVERY way out
    if (planned && s.took && hipEventRecord(s.took->freed, st_) == hipSuccess) s.took->freed_rec = true;
  }
  int32_t prepare(hipStream_t st, uint64_t& slots_per_query) {
    if (int32_t rc = plan_search(h, q_dev, ldq_in, b, 1, nprobe, st, s, true)) return rc;  // (top_k = 1: the partial slots no kernel here reads stay small)
    planned = true; st_ = st;
    W->tot_valid = true;
    slots_per_query = (uint64_t)s.P * s.S_max;
    if ((uint64_t)b * slots_per_query >= 0xFFFFFFFFull) return fail(VERS_ERR_INVALID, "vers_ivf_range_search: batch too large (query x probe x segment slots); split the batch");
    return VERS_OK;
  }
  bool walk_order(uint32_t flags, bool) const { return (flags & VERS_RANGE_WALK_ORDER) != 0; }
  // one pass: pass(query-group tag, metric, the items, how many) launches it over the plan's items.  Hand-out counter as launch_ivf_scan's; no
  // pruning: every row within the radius counts
  template <class Pass>
  int32_t with_items(RangeParams& p, hipStream_t st, Pass&& pass) const {
    return with_qg<1, 8, 16>(s.QG, [&](auto qg) -> int32_t {
      constexpr int QG = decltype(qg)::value;
      if (QG != 1)
        if (int32_t rc = fresh_quad_counter(st, &p.next_quad)) return rc;
      return pass(qg, h->metric, make_ivf_src<QG>(h, s, 0u), (uint32_t)s.items_bound);
    });
  }
  template <class Fill>
  int32_t launch(Fill, RangeParams p, hipStream_t st) const {
    return with_items(p, st, [&](auto qg, int metric, const auto& src, uint32_t items) -> int32_t {
      return launch_range_pass<decltype(qg)::value, Fill::value>(h->n_cu, h->ld, metric, src, items, p, st);
    });
  }
};

// every row that is in a list NOW, over the storage rows (SegSrc<QG, true>: the exhaustive top-k scan's items, cut as option "seg_rows" says when
// set).  An index without centroids (a streamed upload in progress included) is scanned as zero rows: total 0, every limit 0, the radii still
// checked -- what the exhaustive top-k search makes of it.  A partial has no walk order: storage order across ranks has no key (its entry
// points refuse the flag).
struct StoredRangeSource : IvfRangeSource {
  static constexpr bool kKeyIds = true, kPartials = true;
  const char* who;
  const float* q_dev; uint64_t ldq_in; uint32_t b, metric;
  uint64_t n_rows = 0;
  SegPlan sp{};
  StoredRangeSource(vers_ivf* hh, const char* w, const float* q, uint64_t ldq, uint32_t bb, uint32_t m) : IvfRangeSource{hh}, who(w), q_dev(q), ldq_in(ldq), b(bb), metric(m) {}
  int32_t prepare(hipStream_t st, uint64_t& slots_per_query) {
    n_rows = stored_rows(h);
    sp = seg_plan(n_rows, b, h->ld, h->n_cu, knobs().seg_rows);
    if (int32_t rc = W->qil.reserve((size_t)sp.n_qg * h->ldq * sp.QG * sizeof(float))) return rc;
    if (int32_t rc = launch_stage_queries(q_dev, ldq_in, h->d, W->qil.as<float>(), h->ldq, b, sp.QG, st)) return rc;
    if (sp.too_large) return fail(VERS_ERR_INVALID, "vers_ivf_range_search_exhaustive: batch too large (query x segment slots); split the batch");
    slots_per_query = sp.n_segs;
    return VERS_OK;
  }
  bool walk_order(uint32_t flags, bool partial) const { return (flags & VERS_RANGE_WALK_ORDER) != 0 && !partial; }
  void launch_key_ids(const uint64_t* keys, uint64_t n, uint64_t* ids, hipStream_t st) const {
    hipLaunchKernelGGL(range_key_ids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, keys, n, ids);
  }
  template <class Pass>
  int32_t with_items(RangeParams&, hipStream_t, Pass&& pass) const {  // (ProbedRangeSource::with_items over the segment items)
    return with_qg<1, 8>(sp.QG, [&](auto qg) -> int32_t {
      using Src = SegSrc<decltype(qg)::value, true>;
      return pass(qg, (int)metric, make_seg_src<Src>(h->rows.as<float>(), n_rows, h->ld, sp, W->qil.as<float>(), h->ldq, b, nullptr, 0, h->row_ids.as<uint32_t>()), sp.n_items);
    });
  }
  template <class Fill>
  int32_t launch(Fill, RangeParams p, hipStream_t st) const {
    return with_items(p, st, [&](auto qg, int metric, const auto& src, uint32_t items) -> int32_t {
      return launch_range_pass<decltype(qg)::value, Fill::value>(h->n_cu, h->ld, metric, src, items, p, st);
    });
  }
};

// A range search on the index, on `st`: over the probed lists, or (probed = false) over every stored row under the metric given in place of
// nprobe.  own_out / part: range_search_run.  who: the name the source reports under (the unfiltered calls all report as the host-pointer call).
int32_t range_dev_locked(vers_ivf* h, const char* who, bool probed, const float* q_dev, uint64_t ldq_in, uint32_t b, const float* radius_dev, uint32_t nprobe_or_metric,
                         uint32_t flags, uint64_t* lims_dev, uint64_t* ids_dev, float* dist_dev, uint64_t cap, bool own_out, uint64_t* out_total, hipStream_t st,
                         RangePartial* part = nullptr) {
  if (probed) {
    ProbedRangeSource src(h, who, q_dev, ldq_in, b, nprobe_or_metric);
    return range_search_run(src, W->rg, b, radius_dev, flags, lims_dev, ids_dev, dist_dev, cap, own_out, out_total, st, part);
  }
  StoredRangeSource src(h, who, q_dev, ldq_in, b, nprobe_or_metric);
  return range_search_run(src, W->rg, b, radius_dev, flags, lims_dev, ids_dev, dist_dev, cap, own_out, out_total, st, part);
}
static const char* range_name(bool probed) { return probed ? "vers_ivf_range_search" : "vers_ivf_range_search_exhaustive"; }

// ---- filtered range search (filter_range.hip.h, filter_range_multi.hip.h): the range protocol over the allowed rows ---------------------------
// one pass of the filtered range walk, with the kernel of the call's masks; not timed by the scan-timing ring (no range pass is), and no more
// waves than counter slots (filter_begin)
template <int QG, bool FILL, class Src>
static int32_t launch_filter_range_pass(vers_ivf* h, int metric, const Src& src, uint32_t items, const RangeParams& p, FilterChoice f, hipStream_t st) {
  const uint32_t blocks = scan_grid(h->n_cu, QG, h->ld, items, (uint32_t)(filter_wave_slots(h) / kWavesPerBlock));
  return with_metric(metric, [&](auto m) -> int32_t {
    if (f.multi) return launch_scan(filter_range_multi_scan_kernel<QG, decltype(m)::value, FILL, Src>, blocks, kWavesPerBlock, scan_lds_bytes(QG, h->ld), st, src, p, *f.multi);
    return launch_scan(filter_range_scan_kernel<QG, decltype(m)::value, FILL, Src>, blocks, kWavesPerBlock, scan_lds_bytes(QG, h->ld), st, src, p, *f.one);
  });
}

// A range source behind a filter, Base one of ProbedRangeSource and StoredRangeSource: the mask kernel (with its record in the scan-timing ring)
// opens the first phase, over the rows the scan covers (none on an index without centroids for the stored rows); both passes run the filtered
// kernel over the base's items.  The probed plan is the unfiltered one (the lists are ranked as without a filter) but neither consumes nor
// starts a look-ahead.  Serves a rank's partial of the _filtered_partial / _filtered_sharded calls too.
template <class Base>
struct Filtered : Base {
  static constexpr bool kProbed = std::is_same<Base, ProbedRangeSource>::value;
  FilterArg flt;
  FilterMasks masks{};
  Filtered(vers_ivf* hh, const char* w, const float* q, uint64_t ldq, uint32_t bb, uint32_t nprobe_or_metric, const FilterArg& f) : Base(hh, w, q, ldq, bb, nprobe_or_metric), flt(f) {}
  int32_t prepare(hipStream_t st, uint64_t& slots_per_query) {
    vers_ivf* const h = this->h;
    if (int32_t rc = filter_begin(h, flt, kProbed ? h->cap_rows : stored_rows(h), st, masks)) return rc;
    if (kProbed) W->no_ahead = true;
    const int32_t rc = Base::prepare(st, slots_per_query);
    if (kProbed) W->no_ahead = false;
    return rc;
  }
  template <class Fill>
  int32_t launch(Fill, RangeParams p, hipStream_t st) const {
    return this->with_items(p, st, [&](auto qg, int metric, const auto& src, uint32_t items) -> int32_t {
      return launch_filter_range_pass<decltype(qg)::value, Fill::value>(this->h, metric, src, items, p, masks.choice(), st);
    });
  }
};

// A filtered range search on the index, on `st`: mask kernel + counters, the range protocol, the counters folded.  A call that fails leaves
// vers_ivf_filter_stats where it was.  part: a rank's partial ((key, id) pairs, range_search_run); who: the name the source reports under.
int32_t range_filtered_dev_locked(vers_ivf* h, const char* who, bool probed, const float* q_dev, uint64_t ldq_in, uint32_t b, const float* radius_dev, uint32_t nprobe_or_metric,
                                  uint32_t flags, const FilterArg& flt, uint64_t* lims_dev, uint64_t* ids_dev, float* dist_dev, uint64_t cap, bool own_out, uint64_t* out_total,
                                  hipStream_t st, RangePartial* part = nullptr) {
  auto run = [&](auto&& src) -> int32_t {
    if (int32_t rc = range_search_run(src, W->rg, b, radius_dev, flags, lims_dev, ids_dev, dist_dev, cap, own_out, out_total, st, part)) return rc;
    return filter_end(h, st);
  };
  if (probed) return run(Filtered<ProbedRangeSource>(h, who, q_dev, ldq_in, b, nprobe_or_metric, flt));
  return run(Filtered<StoredRangeSource>(h, who, q_dev, ldq_in, b, nprobe_or_metric, flt));
}

// what both exhaustive entry points refuse before they touch the device
static int32_t range_exhaustive_check(vers_ivf* h, const char* who, uint32_t flags, bool partial = false) {
  if (flags & ~VERS_RANGE_WALK_ORDER) return fail(VERS_ERR_INVALID, std::string(who) + ": unknown flag bits");
  if (partial && (flags & VERS_RANGE_WALK_ORDER))
    return fail(VERS_ERR_INVALID, std::string(who) + ": no walk order across ranks (storage order has no key the ranks share); use the default order");
  if (h->world > 1 && !partial)
    return fail(VERS_ERR_INVALID, std::string(who) + ": the handle is sharded by cluster; use vers_ivf_range_search_exhaustive_sharded_dev (or the partial call + vers_range_merge_dev)");
  return VERS_OK;
}

// what both entry points refuse before they touch the device
static int32_t range_check(vers_ivf* h, const char* who, uint32_t nprobe, uint32_t flags, bool partial = false) {
  if (flags & ~VERS_RANGE_WALK_ORDER) return fail(VERS_ERR_INVALID, std::string(who) + ": unknown flag bits");
  if (nprobe == 0) return fail(VERS_ERR_INVALID, std::string(who) + ": nprobe must be at least 1 (the reference's spill walk is defined by top_k: it has no range meaning)");
  if (h->world > 1 && !partial)
    return fail(VERS_ERR_INVALID, std::string(who) + ": the handle is sharded by cluster; use vers_ivf_range_search_sharded_dev (or the partial call + vers_range_merge_dev)");
  if (h->k == 0) return fail(VERS_ERR_INSUFFICIENT, "range search on an index without centroids (reference: index out of bounds, ivfflat.rs:169)");
  return VERS_OK;
}

// ---- the entry scaffolds of the filtered calls and of the range calls: what follows a call's own argument tests --------------------------------
// A device-pointer call: the handle locked shared, check() (what the call refuses from its arguments and the locked handle), nothing more for
// an empty batch, then a workspace leased for `stream` and ordered on it, and body(st).  status_slot: the call synchronises and consumes its
// status itself (the range calls: HostStatusSlot).  A call that returns for b == 0 BEFORE its checks (the range calls) does so itself.
template <class Check, class Body>
static int32_t dev_call(vers_ivf* h, uint32_t b, bool status_slot, void* stream, Check&& check, Body&& body) {
  std::shared_lock<std::shared_mutex> lk(h->index);
  if (int32_t rc = check()) return rc;
  if (b == 0) return VERS_OK;
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)stream;
  WsLease lease(h, true, st);
  if (lease.rc) return lease.rc;
  if (int32_t rc = lease.order_on(st)) return rc;
  std::optional<HostStatusSlot> slot;
  if (status_slot) slot.emplace(h);
  return body(st);
}

// A host-pointer call: the same, with the queries through the pinned staging of every host-pointer call onto the workspace's own stream, and
// body(io).  A body that fails may have queued staging copies that still read the caller's memory: the stream is waited for before the error
// goes back.
template <class Check, class Body>
static int32_t host_call(vers_ivf* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, uint32_t top_k, Check&& check, Body&& body) {
  std::shared_lock<std::shared_mutex> lk(h->index);
  if (int32_t rc = check()) return rc;
  if (b == 0) return VERS_OK;
  DeviceGuard g(h->device);
  WsLease lease(h);
  if (lease.rc) return lease.rc;
  HostStatusSlot slot(h);
  HostIo io;
  if (int32_t rc = host_io_begin(h, queries, q_stride_bytes, b, top_k, io)) return rc;
  lease.st = W->io_stream;
  const int32_t rc = body(io);
  if (rc) (void)hipStreamSynchronize(W->io_stream);
  return rc;
}

// A host call's filter onto the device, on the workspace's stream: the bitmaps packed to ceil(n_bits / 64) words each in W->flt_bits -- one
// bitmap a plain copy, the _multi form a pitched one -- and filter_of beside them in W->flt_of.  An entry of filter_of at or beyond n_filters is
// refused here, where it can be read.  dev: the filter as the device sees it.
static int32_t stage_filter(vers_ivf* h, const char* who, const FilterArg& host, uint32_t b, FilterArg& dev) {
  for (uint32_t q = 0; host.filter_of != nullptr && q < b; ++q)
    if (host.filter_of[q] >= host.n_filters) return fail(VERS_ERR_INVALID, std::string(who) + ": filter_of[" + std::to_string(q) + "] is not below n_filters");
  const size_t words = (size_t)((host.n_bits + 63) / 64), bit_bytes = words * sizeof(uint64_t);
  if (int32_t rc = W->flt_bits.reserve(std::max<size_t>(8, bit_bytes * host.n_filters))) return rc;
  if (host.filter_of != nullptr)
    if (int32_t rc = W->flt_of.reserve((size_t)b * sizeof(uint32_t))) return rc;
  if (bit_bytes && host.filter_of == nullptr && hipMemcpyAsync(W->flt_bits.p, host.filters, bit_bytes, hipMemcpyHostToDevice, W->io_stream) != hipSuccess)
    return fail(VERS_ERR_HIP, std::string(who) + ": staging the bitmap failed");
  if (bit_bytes && host.filter_of != nullptr &&
      hipMemcpy2DAsync(W->flt_bits.p, bit_bytes, host.filters, (size_t)host.stride_words * sizeof(uint64_t), bit_bytes, host.n_filters, hipMemcpyHostToDevice, W->io_stream) != hipSuccess)
    return fail(VERS_ERR_HIP, std::string(who) + ": staging the bitmaps failed");
  if (host.filter_of != nullptr && hipMemcpyAsync(W->flt_of.p, host.filter_of, (size_t)b * sizeof(uint32_t), hipMemcpyHostToDevice, W->io_stream) != hipSuccess)
    return fail(VERS_ERR_HIP, std::string(who) + ": staging filter_of failed");
  dev = FilterArg{W->flt_bits.as<uint64_t>(), (uint64_t)words, host.n_filters, host.n_bits, host.filter_of != nullptr ? W->flt_of.as<uint32_t>() : (const uint32_t*)nullptr};
  return VERS_OK;
}

// A host range call's radii: a NaN among them is refused before the handle is locked ...
static int32_t radii_check(const char* who, const float* radius, uint32_t b) {
  for (uint32_t i = 0; i < b; ++i)
    if (radius[i] != radius[i]) return fail(VERS_ERR_INVALID, std::string(who) + ": NaN radius");
  return VERS_OK;
}
// ... and they go to W->rg_rad on the workspace's stream, with W->rg_lims reserved for the limits
static int32_t stage_radii(vers_ivf* h, const float* radius, uint32_t b) {
  if (int32_t rc = W->rg_rad.reserve((size_t)b * sizeof(float))) return rc;
  if (int32_t rc = W->rg_lims.reserve(((size_t)b + 1) * sizeof(uint64_t))) return rc;
  VERS_HIP_TRY(hipMemcpyAsync(W->rg_rad.p, radius, (size_t)b * sizeof(float), hipMemcpyHostToDevice, W->io_stream));
  return VERS_OK;
}

// a host range call's result out of the workspace (the call has synchronised): the limits and the total always, ids and distances when they fit
static int32_t range_download(vers_ivf* h, uint32_t b, uint64_t total, uint64_t cap, uint64_t* out_lims, uint64_t* out_ids, float* out_dist, uint64_t* out_total) {
  VERS_HIP_TRY(hipMemcpy(out_lims, W->rg_lims.p, ((size_t)b + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
  *out_total = total;
  if (total == 0 || total > cap) return VERS_OK;
  VERS_HIP_TRY(hipMemcpy(out_ids, W->o_ids.p, (size_t)total * sizeof(uint64_t), hipMemcpyDeviceToHost));
  VERS_HIP_TRY(hipMemcpy(out_dist, W->o_dist.p, (size_t)total * sizeof(float), hipMemcpyDeviceToHost));
  return VERS_OK;
}

}  // namespace ivf
}  // namespace vers

namespace vers {

// ---- the flat index's shadow (flat_shadow.hpp): derive, gate, search ------------------------------------------------------------
namespace {
__global__ void flat_row_ids_kernel(uint32_t* ids, uint64_t n, uint64_t n_pad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_pad) ids[i] = i < n ? (uint32_t)i : 0xFFFFFFFFu;
}
constexpr uint32_t kFsTables = 8;  // misc[8 ..]: pj_list | pj_pref | pj_nq | list_off | list_len | qflags | fail_list | fail count
constexpr uint32_t kFsSlotKeys = 64;
}  // namespace

void FlatShadow::release() {
  for (void* p : {(void*)rows_h, (void*)xnorm, (void*)row_ids, (void*)misc, (void*)slots, (void*)fb_part, (void*)fb_ctr})
    if (p) (void)hipFree(p);
  if (bytes) dev_mem_account(-(int64_t)bytes);
  *this = FlatShadow();
}

int32_t flat_shadow_derive(FlatShadow& s, const float* rows_blocked, uint64_t n, uint32_t ld, int n_cu) {
  s.release();
  if (n == 0 || shadow_mode() == 0) return VERS_OK;
  const uint64_t n_pad = (n + 63) / 64 * 64;
  const size_t b_rows = n_pad * (size_t)ld * sizeof(uint16_t), b_norm = n_pad * sizeof(float), b_ids = n_pad * sizeof(uint32_t);
  if (b_rows >= (size_t(1) << 32)) return VERS_OK;  // (flat1h_kernel addresses the shadow through one buffer descriptor)
  s.n_slots = 2u * (uint32_t)n_cu;
  const uint32_t fb_blocks = kFallbackBlocks;
  const size_t b_slots = (size_t)s.n_slots * kFsSlotKeys * sizeof(uint64_t), b_fb = fallback_part_keys(fb_blocks, 1, kMaxTopK) * sizeof(uint64_t),
               b_ctr = (2 * kFallbackBlocks + 1) * sizeof(uint32_t);
  // optional memory: without it the f32 ordered-chain scan stays in charge
  size_t free_b = 0, total_b = 0;
  (void)hipMemGetInfo(&free_b, &total_b);
  const size_t need = b_rows + b_norm + b_ids + b_slots + b_fb + b_ctr + 256;
  bool ok = need + (size_t(1) << 30) <= free_b;
  ok = ok && hipMalloc((void**)&s.rows_h, b_rows) == hipSuccess && hipMalloc((void**)&s.xnorm, b_norm) == hipSuccess &&
       hipMalloc((void**)&s.row_ids, b_ids) == hipSuccess && hipMalloc((void**)&s.misc, 256) == hipSuccess &&
       hipMalloc((void**)&s.slots, b_slots) == hipSuccess && hipMalloc((void**)&s.fb_part, b_fb) == hipSuccess &&
       hipMalloc((void**)&s.fb_ctr, b_ctr) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    s.release();
    return VERS_OK;
  }
  s.bytes = need;
  dev_mem_account((int64_t)s.bytes);
  uint32_t host_misc[64] = {};
  host_misc[kFsTables + 2] = s.n_slots;  // pj_nq: every slot is written by every search
  host_misc[kFsTables + 4] = (uint32_t)n;  // list_len
  VERS_HIP_TRY(hipMemcpy(s.misc, host_misc, sizeof(host_misc), hipMemcpyHostToDevice));
  VERS_HIP_TRY(hipMemset(s.fb_ctr, 0, b_ctr));
  VERS_HIP_TRY(hipMemset(s.slots, 0xFF, b_slots));
  hipLaunchKernelGGL(flat_row_ids_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, 0, s.row_ids, n, n_pad);
  const uint64_t work = n_pad * (ld / 8);
  hipLaunchKernelGGL(rows_to_f16_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, 0, rows_blocked, ld, (uint64_t)0, n_pad, s.rows_h);
  hipLaunchKernelGGL(shadow_residual_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, 0, rows_blocked, ld, (const uint32_t*)s.row_ids, (uint64_t)0, n_pad, s.misc + 2);
  hipLaunchKernelGGL(blocked_row_norms_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, 0, rows_blocked, ld, (const uint32_t*)s.row_ids, (uint64_t)0, n_pad, s.xnorm, s.misc);
  VERS_HIP_TRY(hipGetLastError());
  VERS_HIP_TRY(hipDeviceSynchronize());
  uint32_t r2 = 0;
  VERS_HIP_TRY(hipMemcpy(&r2, s.misc + 2, sizeof(r2), hipMemcpyDeviceToHost));
  float r2f;
  std::memcpy(&r2f, &r2, sizeof(r2f));
  if (!(r2f < std::numeric_limits<float>::infinity())) {  // an element overflows fp16: no certificate would hold
    s.release();
    return VERS_OK;
  }
  s.rows_built = n;
  return VERS_OK;
}

bool flat_shadow_usable(const FlatShadow& s, uint64_t n, uint32_t ld, uint32_t top_k) {
  return s.rows_built == n && n != 0 && s.rows_h != nullptr && shadow_mode() != 0 && single_shadow_ref().load(std::memory_order_relaxed) != 0 &&
         knobs().pre_mode != 0 && top_k >= 1 && top_k + kPreMinSlack <= kPreMaxKp && scan1h_lds_bytes(ld) <= 64u * 1024u;
}

int32_t flat_shadow_search1(FlatShadow& s, const float* rows_blocked, uint64_t n, uint32_t ld, int n_cu, const float* q_padded, uint32_t top_k,
                            uint32_t metric, uint32_t* status, uint64_t* out_ids, float* out_dist, uint32_t* out_count, hipStream_t st,
                            hipEvent_t ev0, hipEvent_t ev1) {
  const uint32_t kp = std::min<uint32_t>(kPreMaxKp, top_k + std::max<uint32_t>(24, top_k));  // (the inverted lists' slack on the shadow: ivf_plan.hip)
  uint32_t* const tb = s.misc + kFsTables;
  const uint32_t n_tiles = (uint32_t)((n + 63) / 64);
  const uint32_t blocks = std::min<uint32_t>(s.n_slots, (n_tiles + kS1hWaves - 1) / kS1hWaves);
  Flat1hArgs fa;
  fa.rows_h = s.rows_h; fa.xnorm = s.xnorm; fa.qp = q_padded; fa.partials = s.slots; fa.qflags = tb + 5; fa.ld = ld; fa.kp = kp; fa.metric = metric; fa.n_rows = (uint32_t)n;
  const size_t lds = scan1h_lds_bytes(ld);
  if (int32_t rc = scan_prepare_launch(flat1h_kernel, lds)) return rc;
  if (blocks < s.n_slots)  // (a small corpus: the slots no block writes must read as empty; kp may differ from the last call's)
    VERS_HIP_TRY(hipMemsetAsync(s.slots, 0xFF, (size_t)s.n_slots * kFsSlotKeys * sizeof(uint64_t), st));
  if (ev0) VERS_HIP_TRY(hipEventRecord(ev0, st));
  hipLaunchKernelGGL(flat1h_kernel, dim3(blocks), dim3(kWave * kS1hWaves), lds, st, fa);
  VERS_HIP_TRY(hipGetLastError());
  if (ev1) VERS_HIP_TRY(hipEventRecord(ev1, st));
  RescoreArgs a;
  a.partials = s.slots; a.P = 1; a.S_max = s.n_slots; a.kp = kp; a.top_k = top_k; a.d_pad = ld;
  a.pj_list = tb + 0; a.pj_pref = tb + 1; a.pj_nq = tb + 2; a.list_off = tb + 3; a.row_ids = s.row_ids;
  a.rows = rows_blocked; a.rows_rm = nullptr; a.ld = ld; a.qp = q_padded; a.ldq = ld; a.xmax2_bits = s.misc;
  a.qflags = tb + 5; a.metric = (int)metric; a.force_fail = knobs().pre_mode == 2; a.shadow = 1; a.debug = 0; a.fail_list = tb + 6; a.stats = s.misc + 1;
  a.status = status; a.out_ids = out_ids; a.out_dist = out_dist; a.out_count = out_count; a.out_keys = nullptr; a.stamps = nullptr;
  a.reset_flag = tb + 5; a.reset_count = tb + 7;
  const int stage_rows = rescore_lds_bytes(ld, true, kRescoreWaves1) <= 144u * 1024u ? 1 : 0;
  const size_t rs_lds = rescore_lds_bytes(ld, stage_rows != 0, kRescoreWaves1);
  if (int32_t rc = scan_prepare_launch(ivf_rescore_kernel<kRescoreWaves1>, rs_lds)) return rc;
  hipLaunchKernelGGL(ivf_rescore_kernel<kRescoreWaves1>, dim3(1), dim3(kWave * kRescoreWaves1), rs_lds, st, a, stage_rows);
  VERS_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(fallback_kernel, dim3(kFallbackBlocks), dim3(kWave * kFbWaves), 0, st, a, (const uint32_t*)(tb + 4), (const uint32_t*)(tb + 6),
                     (const uint32_t*)(tb + 7), s.fb_part, s.fb_ctr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr);
  VERS_HIP_TRY(hipGetLastError());
  return VERS_OK;
}

}  // namespace vers

extern "C" {

int32_t vers_ivf_search_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k,
                            uint32_t nprobe, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev, void* stream) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (b && (!queries_dev || ldq_floats < h->d || !out_count_dev || (top_k && (!out_ids_dev || !out_dist_dev))))
    return fail(VERS_ERR_INVALID, "vers_ivf_search_dev: bad arguments");
  std::shared_lock<std::shared_mutex> lk(h->index);
  DeviceGuard g(h->device);
  WsLease lease(h, true, (hipStream_t)stream);
  if (lease.rc) return lease.rc;
  if (int32_t rc = lease.order_on((hipStream_t)stream)) return rc;
  return search_dev_locked(h, queries_dev, ldq_floats, b, top_k, nprobe, out_ids_dev, out_dist_dev, out_count_dev, nullptr,
                           (hipStream_t)stream);
}

int32_t vers_ivf_search_partial_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k,
                                    uint32_t nprobe, uint64_t* out_keys_dev, uint64_t* out_ids_dev, void* stream) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (top_k == 0) return fail(VERS_ERR_INVALID, "vers_ivf_search_partial_dev: top_k must be at least 1");
  if (b && (!queries_dev || ldq_floats < h->d || !out_keys_dev || !out_ids_dev))
    return fail(VERS_ERR_INVALID, "vers_ivf_search_partial_dev: bad arguments");
  std::shared_lock<std::shared_mutex> lk(h->index);
  DeviceGuard g(h->device);
  WsLease lease(h, true, (hipStream_t)stream);
  if (lease.rc) return lease.rc;
  if (int32_t rc = lease.order_on((hipStream_t)stream)) return rc;
  // distances and counts of the local part are scratch here: the cross-GPU merge recomputes them
  if (int32_t rc = ensure_out(h, (size_t)b * top_k, b)) return rc;
  return search_dev_locked(h, queries_dev, ldq_floats, b, top_k, nprobe, out_ids_dev, W->o_dist.as<float>(), W->o_cnt.as<uint32_t>(),
                           out_keys_dev, (hipStream_t)stream);
}

// A sharded top-k call, all on `stream` (vers_hip.h: vers_gather_t): the local part -> the one exchange -> merge.  What differs between the
// calls is theirs to say:
//   check    under the handle's shared lock, before anything is reserved or exchanged: what the call refuses from its arguments and the handle
//   local    this rank's partial -- keys | ids, [b * top_k] each, kKeyMax padded -- written on `st` by whatever search the call is
//   count_words != 0: an ADAPTIVE filtered call, which exchanges twice.  Its local part hands `reduce` this rank's allowed counts (count_words
//            u32, on the device) between its count kernel and its plan: they are all-gathered on the stream, summed over the ranks on the device
//            and the global counts named.  A rank that fails locally before that point still joins the first gather, with zeros.
using ShardReduce = std::function<int32_t(const uint32_t* local, size_t n, const uint32_t*& global, hipStream_t st)>;
extern "C++" {  // (a template has no C linkage)
template <class Check, class Local>
static int32_t sharded_topk_run(vers_ivf_t* h, const char* who, const vers_gather_t* g, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k, int ref_mode,
                                const size_t& count_words /* read behind check(), which may set it from the locked handle */, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev, void* stream, Check&& check, Local&& local) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (top_k == 0) return fail(VERS_ERR_INVALID, std::string(who) + ": top_k must be at least 1");
  if (b && (!queries_dev || ldq_floats < h->d || !out_ids_dev || !out_dist_dev || !out_count_dev))
    return fail(VERS_ERR_INVALID, std::string(who) + ": bad arguments");
  const uint32_t world = g ? g->world : 1u;
  if (g && (g->world == 0 || g->rank >= g->world || (g->world > 1 && !g->all_gather_async))) return fail(VERS_ERR_INVALID, std::string(who) + ": incomplete vers_gather_t");
  if (b == 0) return VERS_OK;
  std::shared_lock<std::shared_mutex> lk(h->index);
  if (world != h->world || (g && world > 1 && g->rank != h->rank))
    return fail(VERS_ERR_INVALID, std::string(who) + ": the handle is sharded as rank " + std::to_string(h->rank) + " of " + std::to_string(h->world) + ", the exchange says otherwise");
  if (int32_t rc = check()) return rc;
  DeviceGuard gd(h->device);
  hipStream_t st = (hipStream_t)stream;
  WsLease lease(h, true, st);
  if (lease.rc) return lease.rc;
  if (int32_t rc = lease.order_on(st)) return rc;
  const size_t part = (size_t)b * top_k;  // keys | ids of one rank
  // The exchange buffers FIRST.  Up to here a local failure (no workspace, no exchange buffer) leaves this rank unable to take part
  // in the batch's all-gather at all: the peers have queued theirs and wait -- the host must abort the communicator
  // (vers_rccl_abort) when a rank returns from here, there is nothing the library can send.
  const bool exchange = g != nullptr && g->all_gather_async != nullptr;
  {
    int32_t rc = W->g_send.reserve(2 * part * sizeof(uint64_t));
    if (!rc) rc = W->g_recv.reserve((size_t)world * 2 * part * sizeof(uint64_t));
    if (!rc && count_words) rc = W->g_cnt.reserve(((size_t)world + 2) * count_words * sizeof(uint32_t));  // this rank's | the world's | their sum
    if (rc) {
      if (exchange && world > 1)
        fail(rc, std::string(who) + ": the exchange buffers could not be reserved -- this rank cannot join the batch's all-gather; abort the communicator (" + vers_last_error() + ")");
      return rc;
    }
  }
  // (no exchange -- g == nullptr, a single process: the partial is the gathered buffer.  A one-rank communicator still gathers:
  // the call is the same code path as with peers, which is how the RCCL leg is tested on a one-GPU box)
  uint64_t* mine = exchange ? W->g_send.as<uint64_t>() : W->g_recv.as<uint64_t>();
  // The adaptive call's first exchange: exactly once per call, on every way through it.
  bool counted = false;
  int32_t gather_rc = VERS_OK;  // a callback that failed: nothing more is exchanged
  ShardReduce reduce = [&](const uint32_t* counts, size_t n, const uint32_t*& global, hipStream_t) -> int32_t {
    counted = true;
    uint32_t* send = W->g_cnt.as<uint32_t>();
    uint32_t* recv = send + count_words;
    uint32_t* sum = recv + (size_t)world * count_words;
    if (counts != nullptr && n == count_words) VERS_HIP_TRY(hipMemcpyAsync(exchange ? send : recv, counts, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    else VERS_HIP_TRY(hipMemsetAsync(exchange ? send : recv, 0, count_words * sizeof(uint32_t), st));  // (a rank that failed: it adds nothing)
    if (exchange)
      if (int32_t rc = g->all_gather_async(g->ctx, send, recv, count_words * sizeof(uint32_t), stream)) {
        gather_rc = rc;
        return fail(VERS_ERR_COMM, "vers_gather_t::all_gather_async reported failure (status " + std::to_string(rc) + ")");
      }
    hipLaunchKernelGGL(allowed_len_rank_sum_kernel, dim3((unsigned)((count_words + kAdpThreads - 1) / kAdpThreads)), dim3(kAdpThreads), 0, st, (const uint32_t*)recv, world,
                       (uint64_t)count_words, sum);
    VERS_HIP_TRY(hipGetLastError());
    global = sum;
    return VERS_OK;
  };
  // From here on a LOCAL failure (scratch reservation, a failed launch) must not skip the batch's collectives: the peers have
  // already queued their ncclAllGather and would block forever, and every later collective on the communicator would be
  // mismatched.  The rank answers with a POISONED partial instead -- every key kKeyMax (it contributes nothing), first id word
  // kPoisonId -- so that the gather completes everywhere; every rank's merge sees the mark and latches kStPeerFailed in its
  // stream's status word (vers_ivf_poll -> VERS_ERR_COMM); this rank also returns its own error from the call.
  int32_t local_rc = VERS_OK;
  if (W->g_poisoned) {  // (this workspace's send buffer carried the poison mark once: a partial whose first query finds nothing leaves the word as it is)
    (void)hipMemsetAsync(mine + part, 0, sizeof(uint64_t), st);
    W->g_poisoned = false;
  }
  if (test_fail_sharded_ref().load() > 0 && test_fail_sharded_ref().fetch_sub(1) > 0) local_rc = fail(VERS_ERR_HIP, std::string(who) + ": injected local failure (test hook)");
  if (!local_rc) local_rc = local(mine, mine + part, reduce, st);
  if (count_words && !counted && exchange) {  // the local part did not get as far as its counts: zeros, so that the peers' first gather completes
    const std::string why = local_rc ? std::string(vers_last_error()) : std::string();
    const uint32_t* unused = nullptr;
    const int32_t crc = reduce(nullptr, 0, unused, st);
    if (local_rc) fail(local_rc, why);
    else local_rc = crc;
  }
  if (gather_rc) return local_rc;
  if (local_rc && !exchange) return local_rc;
  if (local_rc) {  // (stream order: behind whatever the failed search had already queued into `mine`)
    const std::string why = vers_last_error();
    const uint64_t mark = kPoisonId;
    (void)hipMemsetAsync(mine, 0xFF, 2 * part * sizeof(uint64_t), st);
    (void)hipMemcpyAsync(mine + part, &mark, sizeof(mark), hipMemcpyHostToDevice, st);  // (pageable source: copied before the call returns)
    W->g_poisoned = true;
    (void)hipGetLastError();
    fail(local_rc, why + " [this rank joined the batch's all-gather with a poisoned partial]");
  }
  if (exchange) {
    if (int32_t rc = g->all_gather_async(g->ctx, W->g_send.p, W->g_recv.p, 2 * part * sizeof(uint64_t), stream))
      return local_rc ? local_rc : fail(VERS_ERR_COMM, "vers_gather_t::all_gather_async reported failure (status " + std::to_string(rc) + ")");
  }
  hipLaunchKernelGGL(rank_merge_kernel, dim3(b), dim3(kWave), 0, st, (const uint64_t*)W->g_recv.as<uint64_t>(), (const uint64_t*)W->g_recv.as<uint64_t>() + part,
                     (uint64_t)(2 * part), world, b, top_k, ref_mode, out_ids_dev, out_dist_dev, out_count_dev,
                     exchange ? W->st_word() : (uint32_t*)nullptr);
  if (local_rc) { (void)hipGetLastError(); return local_rc; }
  VERS_HIP_TRY(hipGetLastError());
  return VERS_OK;
}

}  // extern "C++"

// the two unfiltered sharded calls: the local part is the partial search / the partial exhaustive scan
static int32_t sharded_common(vers_ivf_t* h, const vers_gather_t* g, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k,
                              uint32_t nprobe, int exhaustive_metric, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev, void* stream) {
  const char* who = exhaustive_metric >= 0 ? "vers_ivf_search_exhaustive_sharded_dev" : "vers_ivf_search_sharded_dev";
  if (exhaustive_metric > (int)VERS_METRIC_COSDIST) return fail(VERS_ERR_INVALID, "unknown metric");
  const size_t part = (size_t)b * top_k;
  const size_t no_counts = 0;
  return sharded_topk_run(
      h, who, g, queries_dev, ldq_floats, b, top_k, (exhaustive_metric < 0 && nprobe == 0) ? 1 : 0, no_counts, out_ids_dev, out_dist_dev, out_count_dev, stream,
      []() -> int32_t { return VERS_OK; },
      [&](uint64_t* keys, uint64_t* ids, const ShardReduce&, hipStream_t st) -> int32_t {
        if (int32_t rc = ensure_out(h, part, b)) return rc;
        if (exhaustive_metric >= 0) {
          if (int32_t rc = exhaustive_dev_locked(h, queries_dev, ldq_floats, b, top_k, (uint32_t)exhaustive_metric, W->o_ids.as<uint64_t>(), W->o_dist.as<float>(),
                                                 W->o_cnt.as<uint32_t>(), st)) return rc;
          hipLaunchKernelGGL(pack_exhaustive_keys_kernel, dim3((unsigned)((part + 255) / 256)), dim3(256), 0, st, (const uint64_t*)W->o_ids.as<uint64_t>(),
                             (const float*)W->o_dist.as<float>(), (const uint32_t*)W->o_cnt.as<uint32_t>(), b, top_k, keys, ids);
          VERS_HIP_TRY(hipGetLastError());
          return VERS_OK;
        }
        return search_dev_locked(h, queries_dev, ldq_floats, b, top_k, nprobe, ids, W->o_dist.as<float>(), W->o_cnt.as<uint32_t>(), keys, st);
      });
}

int32_t vers_ivf_search_sharded_dev(vers_ivf_t* h, const vers_gather_t* g, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k,
                                    uint32_t nprobe, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev, void* stream) {
  return sharded_common(h, g, queries_dev, ldq_floats, b, top_k, nprobe, -1, out_ids_dev, out_dist_dev, out_count_dev, stream);
}

int32_t vers_ivf_search_exhaustive_sharded_dev(vers_ivf_t* h, const vers_gather_t* g, const float* queries_dev, uint64_t ldq_floats, uint32_t b,
                                               uint32_t top_k, uint32_t metric, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev,
                                               void* stream) {
  if (metric > VERS_METRIC_COSDIST) return fail(VERS_ERR_INVALID, "unknown metric");
  return sharded_common(h, g, queries_dev, ldq_floats, b, top_k, 1, (int)metric, out_ids_dev, out_dist_dev, out_count_dev, stream);
}

int32_t vers_ivf_coarse_ahead_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t nprobe, void* stream) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (b && (!queries_dev || ldq_floats < h->d)) return fail(VERS_ERR_INVALID, "vers_ivf_coarse_ahead_dev: bad arguments");
  std::lock_guard<std::mutex> lk(h->pool_mu);
  (void)stream;  // (the look-ahead is ordered behind the list scan of the NEXT search on this handle, on that search's stream)
  h->pending.set = b != 0 && nprobe != 0;
  h->pending.q_dev = queries_dev; h->pending.ldq_in = ldq_floats; h->pending.b = b; h->pending.nprobe = nprobe;
  return VERS_OK;
}

int32_t vers_topk_merge_dev(const uint64_t* keys_dev, const uint64_t* ids_dev, uint64_t rank_stride, uint32_t world, uint32_t b,
                            uint32_t top_k, uint32_t nprobe, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev,
                            void* stream) {
  if (rank_stride < (uint64_t)b * top_k) return fail(VERS_ERR_INVALID, "vers_topk_merge_dev: rank_stride < b * top_k");
  if (world == 0 || top_k == 0 || (b && (!keys_dev || !ids_dev || !out_ids_dev || !out_dist_dev || !out_count_dev)))
    return fail(VERS_ERR_INVALID, "vers_topk_merge_dev: bad arguments");
  if (b == 0) return VERS_OK;
  hipLaunchKernelGGL(rank_merge_kernel, dim3(b), dim3(kWave), 0, (hipStream_t)stream, keys_dev, ids_dev, rank_stride, world, b, top_k,
                     nprobe == 0 ? 1 : 0, out_ids_dev, out_dist_dev, out_count_dev);
  VERS_HIP_TRY(hipGetLastError());
  return VERS_OK;
}

int32_t vers_ivf_search(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, uint32_t top_k,
                        uint32_t nprobe, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (b && (!queries || q_stride_bytes < (uint64_t)h->d * 4 || q_stride_bytes % 4 || !out_count || (top_k && (!out_ids || !out_dist))))
    return fail(VERS_ERR_INVALID, "vers_ivf_search: bad arguments");
  if (b == 0) return VERS_OK;
  std::shared_lock<std::shared_mutex> lk(h->index);
  DeviceGuard g(h->device);
  WsLease lease(h);
  if (lease.rc) return lease.rc;
  HostStatusSlot slot(h);
  HostIo io;
  if (int32_t rc = host_io_begin(h, queries, q_stride_bytes, b, top_k, io, b == 1 && top_k > 0)) return rc;
  lease.st = W->io_stream;
  // Reference mode ranks only as many lists as the spill may need: 16 first (the merge of the coarse partial lists
  // and the plan are what a single-query call waits for), then 48, then 64 with the exact coarse quantiser, and as
  // the last resort ALL of them (ivfflat.rs:166-195 walks the ranked lists as far as it must -- many empty lists with
  // zero centroids make that real); the batch then goes in slices so that the (query, list) tables stay small.
  int32_t rc = VERS_OK;
  for (int attempt = nprobe == 0 ? 0 : 1; attempt < 4; ++attempt) {
    W->ref_shallow = attempt == 0;
    W->ref_deep = attempt == 2;
    W->ref_all = attempt == 3;
    // every attempt starts from zeros: entries past a query's count must not carry a previous attempt's values
    if (io.direct) {  // (no kernel of this workspace that WRITES is in flight: the previous call ended with its published status or a synchronisation;
                      // a fallback_kernel launch of that call may still be queued -- it returns before its first store when nothing was queued for it:
                      // the publisher invariant in finish.hip.h)
      std::memset((char*)io.ids_dev - io.ids_off, 0, io.out_bytes);
      W->st_host = (uint32_t*)((char*)io.ids_dev - io.ids_off + io.st_off);
      *reinterpret_cast<volatile uint32_t*>(W->st_host) = kStNotYet;  // (the last merge launch overwrites it with the status: host_io_end spins on it)
    } else {
      VERS_HIP_TRY(hipMemsetAsync(W->io_out.p, 0, io.out_bytes, W->io_stream));
    }
    const uint32_t slice = attempt == 3 ? std::max<uint32_t>(1u, 65536u / std::max<uint32_t>(1u, h->k)) : b;
    rc = VERS_OK;
    for (uint32_t q0 = 0; q0 < b && rc == VERS_OK; q0 += slice) {
      const uint32_t bq = std::min(slice, b - q0);
      rc = search_dev_locked(h, io.q_dev + (size_t)q0 * h->d, h->d, bq, top_k, nprobe, io.ids_dev + (size_t)q0 * top_k,
                             io.dist_dev + (size_t)q0 * top_k, io.cnt_dev + q0, nullptr, W->io_stream);
    }
    W->ref_shallow = W->ref_deep = W->ref_all = false;
    W->st_host = nullptr;
    if (rc) return rc;
    rc = host_io_end(h, io, b, top_k, out_ids, out_dist, out_count);
    if (rc != kRetrySpill) break;
    if ((attempt == 0 && h->k <= 16) || (attempt == 1 && h->k <= 48) || (attempt == 2 && h->k <= 64)) break;  // every list was ranked already
  }
  return rc == kRetrySpill ? VERS_ERR_INVALID : rc;
}

int32_t vers_ivf_search_exhaustive_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k,
                                       uint32_t metric, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev,
                                       void* stream) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (metric > VERS_METRIC_COSDIST) return fail(VERS_ERR_INVALID, "unknown metric");
  if (b && (!queries_dev || ldq_floats < h->d || !out_count_dev || (top_k && (!out_ids_dev || !out_dist_dev))))
    return fail(VERS_ERR_INVALID, "vers_ivf_search_exhaustive_dev: bad arguments");
  std::shared_lock<std::shared_mutex> lk(h->index);
  DeviceGuard g(h->device);
  WsLease lease(h, true, (hipStream_t)stream);
  if (lease.rc) return lease.rc;
  if (int32_t rc = lease.order_on((hipStream_t)stream)) return rc;
  return exhaustive_dev_locked(h, queries_dev, ldq_floats, b, top_k, metric, out_ids_dev, out_dist_dev, out_count_dev,
                               (hipStream_t)stream);
}

int32_t vers_ivf_search_exhaustive_partial_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k,
                                               uint32_t metric, uint64_t* out_keys_dev, uint64_t* out_ids_dev, void* stream) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (top_k == 0 || metric > VERS_METRIC_COSDIST) return fail(VERS_ERR_INVALID, "unsupported top_k / metric");
  if (b && (!queries_dev || ldq_floats < h->d || !out_keys_dev || !out_ids_dev))
    return fail(VERS_ERR_INVALID, "vers_ivf_search_exhaustive_partial_dev: bad arguments");
  if (b == 0) return VERS_OK;
  std::shared_lock<std::shared_mutex> lk(h->index);
  DeviceGuard g(h->device);
  WsLease lease(h, true, (hipStream_t)stream);
  if (lease.rc) return lease.rc;
  if (int32_t rc = lease.order_on((hipStream_t)stream)) return rc;
  if (int32_t rc = ensure_out(h, (size_t)b * top_k, b)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int32_t rc = exhaustive_dev_locked(h, queries_dev, ldq_floats, b, top_k, metric, W->o_ids.as<uint64_t>(), W->o_dist.as<float>(),
                                         W->o_cnt.as<uint32_t>(), st)) return rc;
  hipLaunchKernelGGL(pack_exhaustive_keys_kernel, dim3((b * top_k + 255) / 256), dim3(256), 0, st, (const uint64_t*)W->o_ids.as<uint64_t>(),
                     (const float*)W->o_dist.as<float>(), (const uint32_t*)W->o_cnt.as<uint32_t>(), b, top_k, out_keys_dev, out_ids_dev);
  VERS_HIP_TRY(hipGetLastError());
  return VERS_OK;
}

int32_t vers_ivf_search_exhaustive(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, uint32_t top_k,
                                   uint32_t metric, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (metric > VERS_METRIC_COSDIST) return fail(VERS_ERR_INVALID, "unknown metric");
  if (b && (!queries || q_stride_bytes < (uint64_t)h->d * 4 || q_stride_bytes % 4 || !out_count || (top_k && (!out_ids || !out_dist))))
    return fail(VERS_ERR_INVALID, "vers_ivf_search_exhaustive: bad arguments");
  if (b == 0) return VERS_OK;
  std::shared_lock<std::shared_mutex> lk(h->index);
  DeviceGuard g(h->device);
  WsLease lease(h);
  if (lease.rc) return lease.rc;
  HostStatusSlot slot(h);
  HostIo io;
  if (int32_t rc = host_io_begin(h, queries, q_stride_bytes, b, top_k, io)) return rc;
  lease.st = W->io_stream;
  VERS_HIP_TRY(hipMemsetAsync(W->io_out.p, 0, io.out_bytes, W->io_stream));  // entries past a query's count come back as zeros
  if (int32_t rc = exhaustive_dev_locked(h, io.q_dev, h->d, b, top_k, metric, io.ids_dev, io.dist_dev, io.cnt_dev, W->io_stream)) return rc;
  const int32_t rc = host_io_end(h, io, b, top_k, out_ids, out_dist, out_count);
  return rc == kRetrySpill ? VERS_ERR_INVALID : rc;
}

// ---- filtered top-k search (filter.hip.h, filter_multi.hip.h, filter_adaptive.hip.h) ----
// The device-pointer calls: the probed lists or (probed = false) every stored row under the metric given in place of nprobe; one bitmap or the
// _multi form (form); ad: the adaptive call's arguments, nprobe then being nprobe_max.
static int32_t filtered_dev_common(vers_ivf_t* h, const char* who, bool probed, FilterForm form, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k,
                                   uint32_t nprobe_or_metric, const FilterArg& flt, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev, void* stream,
                                   const AdaptiveSpec& ad = {}) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (!probed && nprobe_or_metric > VERS_METRIC_COSDIST) return fail(VERS_ERR_INVALID, "unknown metric");
  if (b && (!queries_dev || ldq_floats < h->d || !out_count_dev || (top_k && (!out_ids_dev || !out_dist_dev))))
    return fail(VERS_ERR_INVALID, std::string(who) + ": bad arguments");
  if (int32_t rc = adaptive_check(who, ad, nprobe_or_metric, AdaptiveKind::kCall)) return rc;
  return dev_call(
      h, b, false, stream, [&]() -> int32_t { return filtered_check(h, who, FilterCheck{probed, false, form, kUseShardedTopk}, nprobe_or_metric, 0, b, flt); },
      [&](hipStream_t st) -> int32_t {
        return filtered_topk_locked(h, probed, queries_dev, ldq_floats, b, top_k, nprobe_or_metric, flt, ad, out_ids_dev, out_dist_dev, out_count_dev, st);
      });
}

// The host-pointer calls: the filter through the workspace (stage_filter), one synchronisation.  ad.out_nprobe is the caller's host array.
static int32_t filtered_host_common(vers_ivf_t* h, const char* who, bool probed, FilterForm form, const float* queries, uint64_t q_stride_bytes, uint32_t b, uint32_t top_k,
                                    uint32_t nprobe_or_metric, const FilterArg& flt, uint64_t* out_ids, float* out_dist, uint32_t* out_count, const AdaptiveSpec& ad = {}) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (!probed && nprobe_or_metric > VERS_METRIC_COSDIST) return fail(VERS_ERR_INVALID, "unknown metric");
  if (b && (!queries || q_stride_bytes < (uint64_t)h->d * 4 || q_stride_bytes % 4 || !out_count || (top_k && (!out_ids || !out_dist))))
    return fail(VERS_ERR_INVALID, std::string(who) + ": bad arguments");
  if (int32_t rc = adaptive_check(who, ad, nprobe_or_metric, AdaptiveKind::kCall)) return rc;
  return host_call(
      h, queries, q_stride_bytes, b, top_k,
      [&]() -> int32_t { return filtered_check(h, who, FilterCheck{probed, false, form, kUseShardedTopk}, nprobe_or_metric, 0, b, flt); },
      [&](const HostIo& io) -> int32_t {
        FilterArg flt_dev;
        if (int32_t rc = stage_filter(h, who, flt, b, flt_dev)) return rc;
        if (hipMemsetAsync(W->io_out.p, 0, io.out_bytes, W->io_stream) != hipSuccess) return fail(VERS_ERR_HIP, std::string(who) + ": hipMemsetAsync failed");  // entries past a query's count come back as zeros
        AdaptiveSpec ad_dev = ad;
        const bool want_np = ad.on && ad.out_nprobe;
        if (want_np) {
          if (int32_t rc = W->flt_np.reserve((size_t)b * sizeof(uint32_t))) return rc;
          ad_dev.out_nprobe = W->flt_np.as<uint32_t>();
        }
        if (int32_t rc = filtered_topk_locked(h, probed, io.q_dev, h->d, b, top_k, nprobe_or_metric, flt_dev, ad_dev, io.ids_dev, io.dist_dev, io.cnt_dev, W->io_stream)) return rc;
        const int32_t rc = host_io_end(h, io, b, top_k, out_ids, out_dist, out_count);
        if (!rc && want_np) VERS_HIP_TRY(hipMemcpy(ad.out_nprobe, W->flt_np.p, (size_t)b * sizeof(uint32_t), hipMemcpyDeviceToHost));  // (the stream has been waited for)
        return rc == kRetrySpill ? VERS_ERR_INVALID : rc;
      });
}

int32_t vers_ivf_search_filtered_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k, uint32_t nprobe,
                                     const uint64_t* allowed_bits_dev, uint64_t n_bits, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev,
                                     void* stream) {
  return filtered_dev_common(h, "vers_ivf_search_filtered_dev", true, FilterForm::kPerCall, queries_dev, ldq_floats, b, top_k, nprobe, per_call_filter(allowed_bits_dev, n_bits),
                             out_ids_dev, out_dist_dev, out_count_dev, stream);
}

int32_t vers_ivf_search_filtered_adaptive_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k, uint32_t nprobe_min,
                                              uint32_t nprobe_max, uint32_t min_allowed, const uint64_t* allowed_bits_dev, uint64_t n_bits, uint64_t* out_ids_dev,
                                              float* out_dist_dev, uint32_t* out_count_dev, uint32_t* out_nprobe_dev, void* stream) {
  return filtered_dev_common(h, "vers_ivf_search_filtered_adaptive_dev", true, FilterForm::kPerCall, queries_dev, ldq_floats, b, top_k, nprobe_max,
                             per_call_filter(allowed_bits_dev, n_bits), out_ids_dev, out_dist_dev, out_count_dev, stream, adaptive_spec(nprobe_min, min_allowed, out_nprobe_dev));
}

int32_t vers_ivf_search_exhaustive_filtered_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k, uint32_t metric,
                                                const uint64_t* allowed_bits_dev, uint64_t n_bits, uint64_t* out_ids_dev, float* out_dist_dev,
                                                uint32_t* out_count_dev, void* stream) {
  return filtered_dev_common(h, "vers_ivf_search_exhaustive_filtered_dev", false, FilterForm::kPerCall, queries_dev, ldq_floats, b, top_k, metric,
                             per_call_filter(allowed_bits_dev, n_bits), out_ids_dev, out_dist_dev, out_count_dev, stream);
}

int32_t vers_ivf_search_filtered(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, uint32_t top_k, uint32_t nprobe,
                                 const uint64_t* allowed_bits, uint64_t n_bits, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  return filtered_host_common(h, "vers_ivf_search_filtered", true, FilterForm::kPerCall, queries, q_stride_bytes, b, top_k, nprobe, per_call_filter(allowed_bits, n_bits), out_ids,
                              out_dist, out_count);
}

int32_t vers_ivf_search_filtered_adaptive(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, uint32_t top_k, uint32_t nprobe_min,
                                          uint32_t nprobe_max, uint32_t min_allowed, const uint64_t* allowed_bits, uint64_t n_bits, uint64_t* out_ids, float* out_dist,
                                          uint32_t* out_count, uint32_t* out_nprobe) {
  return filtered_host_common(h, "vers_ivf_search_filtered_adaptive", true, FilterForm::kPerCall, queries, q_stride_bytes, b, top_k, nprobe_max,
                              per_call_filter(allowed_bits, n_bits), out_ids, out_dist, out_count, adaptive_spec(nprobe_min, min_allowed, out_nprobe));
}

int32_t vers_ivf_search_exhaustive_filtered(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, uint32_t top_k, uint32_t metric,
                                            const uint64_t* allowed_bits, uint64_t n_bits, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  return filtered_host_common(h, "vers_ivf_search_exhaustive_filtered", false, FilterForm::kPerCall, queries, q_stride_bytes, b, top_k, metric,
                              per_call_filter(allowed_bits, n_bits), out_ids, out_dist, out_count);
}

// ---- with a filter per query: the same two paths, the filter in the _multi form ----
int32_t vers_ivf_search_filtered_multi_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k, uint32_t nprobe,
                                           const uint64_t* filters_dev, uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits,
                                           const uint32_t* filter_of_dev, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev, void* stream) {
  return filtered_dev_common(h, "vers_ivf_search_filtered_multi_dev", true, FilterForm::kMulti, queries_dev, ldq_floats, b, top_k, nprobe,
                             FilterArg{filters_dev, filter_stride_words, n_filters, n_bits, filter_of_dev}, out_ids_dev, out_dist_dev, out_count_dev, stream);
}

int32_t vers_ivf_search_filtered_multi_adaptive_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k, uint32_t nprobe_min,
                                                    uint32_t nprobe_max, uint32_t min_allowed, const uint64_t* filters_dev, uint64_t filter_stride_words,
                                                    uint32_t n_filters, uint64_t n_bits, const uint32_t* filter_of_dev, uint64_t* out_ids_dev, float* out_dist_dev,
                                                    uint32_t* out_count_dev, uint32_t* out_nprobe_dev, void* stream) {
  return filtered_dev_common(h, "vers_ivf_search_filtered_multi_adaptive_dev", true, FilterForm::kMulti, queries_dev, ldq_floats, b, top_k, nprobe_max,
                             FilterArg{filters_dev, filter_stride_words, n_filters, n_bits, filter_of_dev}, out_ids_dev, out_dist_dev, out_count_dev, stream,
                             adaptive_spec(nprobe_min, min_allowed, out_nprobe_dev));
}

int32_t vers_ivf_search_exhaustive_filtered_multi_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k, uint32_t metric,
                                                      const uint64_t* filters_dev, uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits,
                                                      const uint32_t* filter_of_dev, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev,
                                                      void* stream) {
  return filtered_dev_common(h, "vers_ivf_search_exhaustive_filtered_multi_dev", false, FilterForm::kMulti, queries_dev, ldq_floats, b, top_k, metric,
                             FilterArg{filters_dev, filter_stride_words, n_filters, n_bits, filter_of_dev}, out_ids_dev, out_dist_dev, out_count_dev, stream);
}

int32_t vers_ivf_search_filtered_multi(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, uint32_t top_k, uint32_t nprobe,
                                       const uint64_t* filters, uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits, const uint32_t* filter_of,
                                       uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  return filtered_host_common(h, "vers_ivf_search_filtered_multi", true, FilterForm::kMulti, queries, q_stride_bytes, b, top_k, nprobe,
                              FilterArg{filters, filter_stride_words, n_filters, n_bits, filter_of}, out_ids, out_dist, out_count);
}

int32_t vers_ivf_search_filtered_multi_adaptive(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, uint32_t top_k, uint32_t nprobe_min,
                                                uint32_t nprobe_max, uint32_t min_allowed, const uint64_t* filters, uint64_t filter_stride_words, uint32_t n_filters,
                                                uint64_t n_bits, const uint32_t* filter_of, uint64_t* out_ids, float* out_dist, uint32_t* out_count,
                                                uint32_t* out_nprobe) {
  return filtered_host_common(h, "vers_ivf_search_filtered_multi_adaptive", true, FilterForm::kMulti, queries, q_stride_bytes, b, top_k, nprobe_max,
                              FilterArg{filters, filter_stride_words, n_filters, n_bits, filter_of}, out_ids, out_dist, out_count,
                              adaptive_spec(nprobe_min, min_allowed, out_nprobe));
}

int32_t vers_ivf_search_exhaustive_filtered_multi(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, uint32_t top_k, uint32_t metric,
                                                  const uint64_t* filters, uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits,
                                                  const uint32_t* filter_of, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  return filtered_host_common(h, "vers_ivf_search_exhaustive_filtered_multi", false, FilterForm::kMulti, queries, q_stride_bytes, b, top_k, metric,
                              FilterArg{filters, filter_stride_words, n_filters, n_bits, filter_of}, out_ids, out_dist, out_count);
}

int32_t vers_ivf_filter_stats(vers_ivf_t* h, uint64_t* out4, uint64_t* out4_total) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  DeviceGuard g(h->device);
  unsigned long long last[kFltStats] = {}, tot[kFltStats] = {};
  SearchWs* ws = nullptr;
  {
    std::lock_guard<std::mutex> lk(h->pool_mu);
    ws = h->flt_last;
  }
  if (ws && ws->flt_stats.p) {  // (a measurement hook: the caller has stopped issuing filtered calls)
    if (ws->used && ws->done) VERS_HIP_TRY(hipEventSynchronize(ws->done));
    VERS_HIP_TRY(hipMemcpy(last, ws->flt_stats.p, sizeof(last), hipMemcpyDeviceToHost));
  }
  {
    std::lock_guard<std::mutex> lk(h->flt_mu);
    if (h->flt_total.p) VERS_HIP_TRY(hipMemcpy(tot, h->flt_total.p, sizeof(tot), hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < kFltStats; ++i) {
    if (out4) out4[i] = last[i];
    if (out4_total) out4_total[i] = tot[i];
  }
  return VERS_OK;
}

// The four device-pointer range entries: the probed lists or (probed = false) every stored row under the metric given in place of nprobe; the
// full result (ids + distances) or, with keys_dev in place of dist_dev, a rank's partial (keys + ids).
static int32_t range_dev_common(vers_ivf_t* h, const char* who, bool probed, bool partial, const float* queries_dev, uint64_t ldq_floats, uint32_t b,
                                const float* radius_dev, uint32_t nprobe_or_metric, uint32_t flags, uint64_t* out_lims_dev, uint64_t* out_keys_dev, uint64_t* out_ids_dev,
                                float* out_dist_dev, uint64_t cap, uint64_t* out_total, void* stream) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (!out_total) return fail(VERS_ERR_INVALID, std::string(who) + ": out_total is required");
  *out_total = 0;
  if (!probed && nprobe_or_metric > VERS_METRIC_COSDIST) return fail(VERS_ERR_INVALID, "unknown metric");
  if (b && (!queries_dev || ldq_floats < h->d || !radius_dev || !out_lims_dev || (cap && (!out_ids_dev || (partial ? !out_keys_dev : !out_dist_dev)))))
    return fail(VERS_ERR_INVALID, std::string(who) + ": bad arguments");
  if (b == 0) return VERS_OK;
  return dev_call(
      h, b, true, stream, [&]() -> int32_t { return probed ? range_check(h, who, nprobe_or_metric, flags, partial) : range_exhaustive_check(h, who, flags, partial); },
      [&](hipStream_t st) -> int32_t {
        RangePartial part;
        part.keys = out_keys_dev;
        return range_dev_locked(h, range_name(probed), probed, queries_dev, ldq_floats, b, radius_dev, nprobe_or_metric, flags, out_lims_dev, out_ids_dev, out_dist_dev, cap, false,
                                out_total, st, partial ? &part : nullptr);
      });
}

int32_t vers_ivf_range_search_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev, uint32_t nprobe,
                                  uint32_t flags, uint64_t* out_lims_dev, uint64_t* out_ids_dev, float* out_dist_dev, uint64_t cap, uint64_t* out_total,
                                  void* stream) {
  return range_dev_common(h, "vers_ivf_range_search_dev", true, false, queries_dev, ldq_floats, b, radius_dev, nprobe, flags, out_lims_dev, nullptr, out_ids_dev,
                          out_dist_dev, cap, out_total, stream);
}

int32_t vers_ivf_range_search_exhaustive_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev,
                                             uint32_t metric, uint32_t flags, uint64_t* out_lims_dev, uint64_t* out_ids_dev, float* out_dist_dev,
                                             uint64_t cap, uint64_t* out_total, void* stream) {
  return range_dev_common(h, "vers_ivf_range_search_exhaustive_dev", false, false, queries_dev, ldq_floats, b, radius_dev, metric, flags, out_lims_dev, nullptr,
                          out_ids_dev, out_dist_dev, cap, out_total, stream);
}

// ---- sharded range search: a rank's partial, the cross-rank merge, and the two exchanges around them (vers_hip.h) ----
int32_t vers_ivf_range_search_partial_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev, uint32_t nprobe,
                                          uint32_t flags, uint64_t* out_lims_dev, uint64_t* out_keys_dev, uint64_t* out_ids_dev, uint64_t cap, uint64_t* out_total,
                                          void* stream) {
  return range_dev_common(h, "vers_ivf_range_search_partial_dev", true, true, queries_dev, ldq_floats, b, radius_dev, nprobe, flags, out_lims_dev, out_keys_dev,
                          out_ids_dev, nullptr, cap, out_total, stream);
}

int32_t vers_ivf_range_search_exhaustive_partial_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev,
                                                     uint32_t metric, uint32_t flags, uint64_t* out_lims_dev, uint64_t* out_keys_dev, uint64_t* out_ids_dev,
                                                     uint64_t cap, uint64_t* out_total, void* stream) {
  return range_dev_common(h, "vers_ivf_range_search_exhaustive_partial_dev", false, true, queries_dev, ldq_floats, b, radius_dev, metric, flags, out_lims_dev,
                          out_keys_dev, out_ids_dev, nullptr, cap, out_total, stream);
}

// the two host-pointer range entries: queries through the pinned staging of every host-pointer call, radii and limits through the workspace
static int32_t range_host_common(vers_ivf_t* h, const char* who, bool probed, const float* queries, uint64_t q_stride_bytes, uint32_t b, const float* radius,
                                 uint32_t nprobe_or_metric, uint32_t flags, uint64_t* out_lims, uint64_t* out_ids, float* out_dist, uint64_t cap, uint64_t* out_total) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (!out_total) return fail(VERS_ERR_INVALID, std::string(who) + ": out_total is required");
  *out_total = 0;
  if (!probed && nprobe_or_metric > VERS_METRIC_COSDIST) return fail(VERS_ERR_INVALID, "unknown metric");
  if (b && (!queries || q_stride_bytes < (uint64_t)h->d * 4 || q_stride_bytes % 4 || !radius || !out_lims || (cap && (!out_ids || !out_dist))))
    return fail(VERS_ERR_INVALID, std::string(who) + ": bad arguments");
  if (b == 0) return VERS_OK;
  if (int32_t rc = radii_check(who, radius, b)) return rc;
  std::shared_lock<std::shared_mutex> lk(h->index);
  if (int32_t rc = probed ? range_check(h, who, nprobe_or_metric, flags) : range_exhaustive_check(h, who, flags)) return rc;
  DeviceGuard g(h->device);
  WsLease lease(h);
  if (lease.rc) return lease.rc;
  HostStatusSlot slot(h);
  HostIo io;
  if (int32_t rc = host_io_begin(h, queries, q_stride_bytes, b, 0, io)) return rc;  // (the pinned query staging of every host-pointer call)
  lease.st = W->io_stream;
  if (int32_t rc = stage_radii(h, radius, b)) return rc;
  uint64_t total = 0;
  if (int32_t rc = range_dev_locked(h, who, probed, io.q_dev, h->d, b, W->rg_rad.as<float>(), nprobe_or_metric, flags, W->rg_lims.as<uint64_t>(), nullptr, nullptr, cap, true,
                                    &total, W->io_stream)) return rc;
  return range_download(h, b, total, cap, out_lims, out_ids, out_dist, out_total);
}

int32_t vers_ivf_range_search(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, const float* radius, uint32_t nprobe, uint32_t flags,
                              uint64_t* out_lims, uint64_t* out_ids, float* out_dist, uint64_t cap, uint64_t* out_total) {
  return range_host_common(h, "vers_ivf_range_search", true, queries, q_stride_bytes, b, radius, nprobe, flags, out_lims, out_ids, out_dist, cap, out_total);
}

int32_t vers_ivf_range_search_exhaustive(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, const float* radius, uint32_t metric,
                                         uint32_t flags, uint64_t* out_lims, uint64_t* out_ids, float* out_dist, uint64_t cap, uint64_t* out_total) {
  return range_host_common(h, "vers_ivf_range_search_exhaustive", false, queries, q_stride_bytes, b, radius, metric, flags, out_lims, out_ids, out_dist, cap, out_total);
}

// ---- filtered range search (filter_range.hip.h, filter_range_multi.hip.h): the probed lists or (probed = false) every stored row under the metric
// given in place of nprobe; one bitmap, the _multi form, or (a rank's partial: out_keys_dev in place of out_dist_dev) either ----
// The device-pointer calls.  who: the entry point; src_who: the name its range source reports under (the host-pointer call's for the whole calls).
static int32_t range_filtered_dev_common(vers_ivf_t* h, const char* who, const char* src_who, bool probed, FilterForm form, const float* queries_dev, uint64_t ldq_floats,
                                         uint32_t b, const float* radius_dev, uint32_t nprobe_or_metric, uint32_t flags, const FilterArg& flt, uint64_t* out_lims_dev,
                                         uint64_t* out_keys_dev, uint64_t* out_ids_dev, float* out_dist_dev, uint64_t cap, uint64_t* out_total, void* stream) {
  const bool partial = form == FilterForm::kEither;
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (!out_total) return fail(VERS_ERR_INVALID, std::string(who) + ": out_total is required");
  *out_total = 0;
  if (!probed && nprobe_or_metric > VERS_METRIC_COSDIST) return fail(VERS_ERR_INVALID, "unknown metric");
  if (b && (!queries_dev || ldq_floats < h->d || !radius_dev || !out_lims_dev || (cap && (!out_ids_dev || (partial ? !out_keys_dev : !out_dist_dev)))))
    return fail(VERS_ERR_INVALID, std::string(who) + ": bad arguments");
  if (b == 0) return VERS_OK;
  return dev_call(
      h, b, true, stream,
      [&]() -> int32_t { return filtered_check(h, who, FilterCheck{probed, true, form, partial ? nullptr : kUseShardedRange}, nprobe_or_metric, flags, b, flt); },
      [&](hipStream_t st) -> int32_t {
        RangePartial part;
        part.keys = out_keys_dev;
        return range_filtered_dev_locked(h, src_who, probed, queries_dev, ldq_floats, b, radius_dev, nprobe_or_metric, flags, flt, out_lims_dev, out_ids_dev, out_dist_dev, cap,
                                         false, out_total, st, partial ? &part : nullptr);
      });
}

// The host-pointer calls: radii and limits through the workspace (stage_radii), the filter beside them (stage_filter).
static int32_t range_filtered_host_common(vers_ivf_t* h, const char* who, bool probed, FilterForm form, const float* queries, uint64_t q_stride_bytes, uint32_t b,
                                          const float* radius, uint32_t nprobe_or_metric, uint32_t flags, const FilterArg& flt, uint64_t* out_lims, uint64_t* out_ids,
                                          float* out_dist, uint64_t cap, uint64_t* out_total) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (!out_total) return fail(VERS_ERR_INVALID, std::string(who) + ": out_total is required");
  *out_total = 0;
  if (!probed && nprobe_or_metric > VERS_METRIC_COSDIST) return fail(VERS_ERR_INVALID, "unknown metric");
  if (b && (!queries || q_stride_bytes < (uint64_t)h->d * 4 || q_stride_bytes % 4 || !radius || !out_lims || (cap && (!out_ids || !out_dist))))
    return fail(VERS_ERR_INVALID, std::string(who) + ": bad arguments");
  if (b == 0) return VERS_OK;
  if (int32_t rc = radii_check(who, radius, b)) return rc;
  return host_call(
      h, queries, q_stride_bytes, b, 0,
      [&]() -> int32_t { return filtered_check(h, who, FilterCheck{probed, true, form, kUseShardedRange}, nprobe_or_metric, flags, b, flt); },
      [&](const HostIo& io) -> int32_t {
        FilterArg flt_dev;
        if (int32_t rc = stage_radii(h, radius, b)) return rc;
        if (int32_t rc = stage_filter(h, who, flt, b, flt_dev)) return rc;
        uint64_t total = 0;
        if (int32_t rc = range_filtered_dev_locked(h, who, probed, io.q_dev, h->d, b, W->rg_rad.as<float>(), nprobe_or_metric, flags, flt_dev, W->rg_lims.as<uint64_t>(), nullptr,
                                                   nullptr, cap, true, &total, W->io_stream)) return rc;
        return range_download(h, b, total, cap, out_lims, out_ids, out_dist, out_total);
      });
}

int32_t vers_ivf_range_search_filtered_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev, uint32_t nprobe,
                                           uint32_t flags, const uint64_t* allowed_bits_dev, uint64_t n_bits, uint64_t* out_lims_dev, uint64_t* out_ids_dev,
                                           float* out_dist_dev, uint64_t cap, uint64_t* out_total, void* stream) {
  return range_filtered_dev_common(h, "vers_ivf_range_search_filtered_dev", "vers_ivf_range_search_filtered", true, FilterForm::kPerCall, queries_dev, ldq_floats, b, radius_dev,
                                   nprobe, flags, per_call_filter(allowed_bits_dev, n_bits), out_lims_dev, nullptr, out_ids_dev, out_dist_dev, cap, out_total, stream);
}

int32_t vers_ivf_range_search_exhaustive_filtered_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev,
                                                      uint32_t metric, uint32_t flags, const uint64_t* allowed_bits_dev, uint64_t n_bits, uint64_t* out_lims_dev,
                                                      uint64_t* out_ids_dev, float* out_dist_dev, uint64_t cap, uint64_t* out_total, void* stream) {
  return range_filtered_dev_common(h, "vers_ivf_range_search_exhaustive_filtered_dev", "vers_ivf_range_search_exhaustive_filtered", false, FilterForm::kPerCall, queries_dev,
                                   ldq_floats, b, radius_dev, metric, flags, per_call_filter(allowed_bits_dev, n_bits), out_lims_dev, nullptr, out_ids_dev, out_dist_dev, cap,
                                   out_total, stream);
}

int32_t vers_ivf_range_search_filtered(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, const float* radius, uint32_t nprobe, uint32_t flags,
                                       const uint64_t* allowed_bits, uint64_t n_bits, uint64_t* out_lims, uint64_t* out_ids, float* out_dist, uint64_t cap,
                                       uint64_t* out_total) {
  return range_filtered_host_common(h, "vers_ivf_range_search_filtered", true, FilterForm::kPerCall, queries, q_stride_bytes, b, radius, nprobe, flags,
                                    per_call_filter(allowed_bits, n_bits), out_lims, out_ids, out_dist, cap, out_total);
}

int32_t vers_ivf_range_search_exhaustive_filtered(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, const float* radius, uint32_t metric,
                                                  uint32_t flags, const uint64_t* allowed_bits, uint64_t n_bits, uint64_t* out_lims, uint64_t* out_ids, float* out_dist,
                                                  uint64_t cap, uint64_t* out_total) {
  return range_filtered_host_common(h, "vers_ivf_range_search_exhaustive_filtered", false, FilterForm::kPerCall, queries, q_stride_bytes, b, radius, metric, flags,
                                    per_call_filter(allowed_bits, n_bits), out_lims, out_ids, out_dist, cap, out_total);
}

int32_t vers_ivf_range_search_filtered_multi_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev, uint32_t nprobe,
                                                 uint32_t flags, const uint64_t* filters_dev, uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits,
                                                 const uint32_t* filter_of_dev, uint64_t* out_lims_dev, uint64_t* out_ids_dev, float* out_dist_dev, uint64_t cap,
                                                 uint64_t* out_total, void* stream) {
  return range_filtered_dev_common(h, "vers_ivf_range_search_filtered_multi_dev", "vers_ivf_range_search_filtered_multi", true, FilterForm::kMulti, queries_dev, ldq_floats, b,
                                   radius_dev, nprobe, flags, FilterArg{filters_dev, filter_stride_words, n_filters, n_bits, filter_of_dev}, out_lims_dev, nullptr, out_ids_dev,
                                   out_dist_dev, cap, out_total, stream);
}

int32_t vers_ivf_range_search_exhaustive_filtered_multi_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev,
                                                            uint32_t metric, uint32_t flags, const uint64_t* filters_dev, uint64_t filter_stride_words,
                                                            uint32_t n_filters, uint64_t n_bits, const uint32_t* filter_of_dev, uint64_t* out_lims_dev,
                                                            uint64_t* out_ids_dev, float* out_dist_dev, uint64_t cap, uint64_t* out_total, void* stream) {
  return range_filtered_dev_common(h, "vers_ivf_range_search_exhaustive_filtered_multi_dev", "vers_ivf_range_search_exhaustive_filtered_multi", false, FilterForm::kMulti,
                                   queries_dev, ldq_floats, b, radius_dev, metric, flags, FilterArg{filters_dev, filter_stride_words, n_filters, n_bits, filter_of_dev},
                                   out_lims_dev, nullptr, out_ids_dev, out_dist_dev, cap, out_total, stream);
}

int32_t vers_ivf_range_search_filtered_multi(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, const float* radius, uint32_t nprobe,
                                             uint32_t flags, const uint64_t* filters, uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits,
                                             const uint32_t* filter_of, uint64_t* out_lims, uint64_t* out_ids, float* out_dist, uint64_t cap, uint64_t* out_total) {
  return range_filtered_host_common(h, "vers_ivf_range_search_filtered_multi", true, FilterForm::kMulti, queries, q_stride_bytes, b, radius, nprobe, flags,
                                    FilterArg{filters, filter_stride_words, n_filters, n_bits, filter_of}, out_lims, out_ids, out_dist, cap, out_total);
}

int32_t vers_ivf_range_search_exhaustive_filtered_multi(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, const float* radius, uint32_t metric,
                                                        uint32_t flags, const uint64_t* filters, uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits,
                                                        const uint32_t* filter_of, uint64_t* out_lims, uint64_t* out_ids, float* out_dist, uint64_t cap,
                                                        uint64_t* out_total) {
  return range_filtered_host_common(h, "vers_ivf_range_search_exhaustive_filtered_multi", false, FilterForm::kMulti, queries, q_stride_bytes, b, radius, metric, flags,
                                    FilterArg{filters, filter_stride_words, n_filters, n_bits, filter_of}, out_lims, out_ids, out_dist, cap, out_total);
}

int32_t vers_range_merge_dev(const uint64_t* keys_dev, const uint64_t* ids_dev, uint64_t rank_stride, const uint64_t* rank_lims_dev, uint32_t world, uint32_t b,
                             uint32_t flags, uint64_t* out_lims_dev, uint64_t* out_ids_dev, float* out_dist_dev, void* stream) {
  if (world == 0 || world > 65535u) return fail(VERS_ERR_INVALID, "vers_range_merge_dev: world must be 1 .. 65535");
  if (flags & ~VERS_RANGE_WALK_ORDER) return fail(VERS_ERR_INVALID, "vers_range_merge_dev: unknown flag bits");
  if (b && (!rank_lims_dev || !out_lims_dev || (rank_stride && (!keys_dev || !ids_dev || !out_ids_dev || !out_dist_dev))))
    return fail(VERS_ERR_INVALID, "vers_range_merge_dev: bad arguments");
  if (b == 0) return VERS_OK;
  if (int32_t rc = launch_range_merge(keys_dev, ids_dev, rank_stride, rank_lims_dev, world, b, (flags & VERS_RANGE_WALK_ORDER) != 0, out_lims_dev, out_ids_dev,
                                      out_dist_dev, (hipStream_t)stream))
    return fail(rc, "vers_range_merge_dev: launch failed");
  return VERS_OK;
}

// local count -> exchange 1 (counts + status: the agreement round) -> local fill into the send buffer -> exchange 2 (keys | ids, padded to
// the largest rank) -> merge.  What differs between the sharded range calls is theirs to say:
//   key_ids  the sort key's low word is the vec id (the exhaustive calls: keys alone are sorted) -- sizes the sort's scratch
//   check    under the handle's shared lock, before any exchange: what the call refuses from its arguments and the handle
//   local    the rank's partial range call (range_search_run with `part`): count pass, part->decide, fill pass, on `st`
extern "C++" {  // (a template has no C linkage)
template <class Check, class Local>
static int32_t range_sharded_run(vers_ivf_t* h, const char* who_c, const vers_comm_t* comm, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev,
                                 bool key_ids, uint32_t flags, uint64_t* out_lims_dev, uint64_t* out_ids_dev, float* out_dist_dev, uint64_t cap, uint64_t* out_total,
                                 void* stream, Check&& check, Local&& local) {
  const std::string who = who_c;
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (!out_total) return fail(VERS_ERR_INVALID, who + ": out_total is required");
  *out_total = 0;
  if (b && (!queries_dev || ldq_floats < h->d || !radius_dev || !out_lims_dev || (cap && (!out_ids_dev || !out_dist_dev)))) return fail(VERS_ERR_INVALID, who + ": bad arguments");
  if (comm && (comm->world == 0 || comm->rank >= comm->world || comm->world > 65535u || !comm->all_gather)) return fail(VERS_ERR_INVALID, who + ": incomplete vers_comm_t");
  if (b == 0) return VERS_OK;
  std::shared_lock<std::shared_mutex> lk(h->index);
  const uint32_t world = comm ? comm->world : 1u;
  if (world != h->world || (comm && world > 1 && comm->rank != h->rank))
    return fail(VERS_ERR_INVALID, who + ": the handle is sharded as rank " + std::to_string(h->rank) + " of " + std::to_string(h->world) + ", the communicator says otherwise");
  if (int32_t rc = check()) return rc;
  DeviceGuard gd(h->device);
  hipStream_t st = (hipStream_t)stream;
  WsLease lease(h, true, st);
  if (lease.rc) return lease.rc;
  if (int32_t rc = lease.order_on(st)) return rc;
  HostStatusSlot slot(h);
  const uint32_t me = comm ? comm->rank : 0u;
  const size_t nw = (size_t)b + 1;  // words of exchange 1 per rank: b counts | the status
  std::vector<uint64_t> all((size_t)world * nw, 0), rank_lims((size_t)world * nw, 0), lims(nw, 0);
  uint64_t g_total = 0, t_max = 0;
  bool agreed = false;
  // Exchange 1.  EVERY way out of the local count leads here exactly once -- a rank that failed (a NaN distance, a NaN radius, scratch that
  // did not fit, the injected failure) enters with zero counts and its status, so that nobody waits for it and everybody leaves with the
  // same verdict: the first failing rank's status, in rank order.
  auto exchange1 = [&](int32_t local_rc, bool have_lims) -> int32_t {
    agreed = true;
    const std::string local_why = local_rc ? std::string(vers_last_error()) : std::string();
    uint64_t* mine = all.data() + (size_t)me * nw;
    if (!local_rc && have_lims) {
      if (hipMemcpy(lims.data(), W->rg_lims.p, nw * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) local_rc = fail(VERS_ERR_HIP, who + ": reading the local limits failed");
      else
        for (uint32_t q = 0; q < b; ++q) mine[q] = lims[q + 1] - lims[q];
    }
    mine[b] = (uint64_t)(uint32_t)local_rc;
    if (comm) {
      int32_t rc = W->g_send.reserve(nw * sizeof(uint64_t));
      if (!rc) rc = W->g_recv.reserve((size_t)world * nw * sizeof(uint64_t));
      if (!rc && hipMemcpy(W->g_send.p, mine, nw * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess) rc = VERS_ERR_HIP;
      if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = VERS_ERR_HIP;
      if (rc)  // (nothing the library can send: the host aborts the group on a non-zero return, as for the sharded build)
        return local_rc ? local_rc : fail(rc, who + ": the exchange buffers could not be set up -- this rank cannot join the agreement round; abort the group");
      if (int32_t crc = comm->all_gather(comm->ctx, W->g_send.p, W->g_recv.p, nw * sizeof(uint64_t)))
        return local_rc ? local_rc : fail(VERS_ERR_COMM, "vers_comm_t::all_gather reported failure (status " + std::to_string(crc) + ")");
      if (hipMemcpy(all.data(), W->g_recv.p, (size_t)world * nw * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess)
        return local_rc ? local_rc : fail(VERS_ERR_HIP, who + ": reading the gathered counts failed");
    }
    for (uint32_t r = 0; r < world; ++r) {
      const int32_t s = (int32_t)(uint32_t)all[(size_t)r * nw + b];
      if (s == 0) continue;
      if (r == me) return fail(s, local_why);
      return fail(s, who + ": rank " + std::to_string(r) + " reported status " + std::to_string(s) + "; no rank wrote a result");
    }
    for (uint32_t r = 0; r < world; ++r) {
      uint64_t* rl = rank_lims.data() + (size_t)r * nw;
      rl[0] = 0;
      for (uint32_t q = 0; q < b; ++q) rl[q + 1] = rl[q] + all[(size_t)r * nw + q];
      t_max = std::max(t_max, rl[b]);
    }
    for (uint32_t q = 0; q <= b; ++q) {
      uint64_t sum = 0;
      for (uint32_t r = 0; r < world; ++r) sum += rank_lims[(size_t)r * nw + q];
      lims[q] = sum;
    }
    g_total = lims[b];
    if (g_total > 0xFFFFFFFFull) return fail(VERS_ERR_INVALID, who + ": more than 2^32 - 1 results in one call; split the batch");
    VERS_HIP_TRY(hipMemcpy(out_lims_dev, lims.data(), nw * sizeof(uint64_t), hipMemcpyHostToDevice));
    *out_total = g_total;
    return VERS_OK;
  };
  uint64_t local_total = 0;
  bool gather = false;  // 0 < global total <= cap: exchange 2 and the merge follow
  RangePartial part;
  part.decide = [&](uint64_t total, uint64_t*& keys, uint64_t*& ids, bool& go) -> int32_t {
    local_total = total;
    int32_t lrc = VERS_OK;
    if (total != 0 && total <= cap) {  // the fill's staging BEFORE the agreement: scratch that does not fit is a status the peers learn
      lrc = W->rg.stage.reserve(2 * (size_t)total * sizeof(uint64_t));
      if (!lrc && !(flags & VERS_RANGE_WALK_ORDER))
        lrc = W->rg.tmp.reserve(key_ids ? range_sort_keys_temp_bytes((uint32_t)total, b) : range_sort_temp_bytes((uint32_t)total, b));
    }
    if (int32_t rc = exchange1(lrc, true)) return rc;
    go = false;
    gather = g_total != 0 && g_total <= cap;
    if (!gather) return VERS_OK;
    // (past the agreement a local failure has no round left to be told in: the host aborts the group on a non-zero return)
    if (int32_t rc = W->g_recv.reserve((size_t)world * 2 * t_max * sizeof(uint64_t))) return rc;
    if (comm)
      if (int32_t rc = W->g_send.reserve(2 * (size_t)t_max * sizeof(uint64_t))) return rc;
    uint64_t* mine = comm ? W->g_send.as<uint64_t>() : W->g_recv.as<uint64_t>();
    VERS_HIP_TRY(hipMemsetAsync(mine, 0xFF, 2 * (size_t)t_max * sizeof(uint64_t), st));  // the padding behind a shorter rank: defined bytes, never read by the merge
    keys = mine; ids = mine + t_max;
    go = total != 0;
    return VERS_OK;
  };
  int32_t rc = VERS_OK;
  if (test_fail_sharded_ref().load() > 0 && test_fail_sharded_ref().fetch_sub(1) > 0) rc = fail(VERS_ERR_HIP, who + ": injected local failure (test hook)");
  if (!rc) {
    rc = W->rg_lims.reserve(nw * sizeof(uint64_t));
    if (!rc) rc = local(W->rg_lims.as<uint64_t>(), &local_total, st, &part);
  }
  if (!agreed) {  // the local count did not get as far as the agreement: enter it with the failure
    const int32_t arc = exchange1(rc ? rc : fail(VERS_ERR_HIP, who + ": the local count ended without a verdict"), false);
    *out_total = 0;
    return arc;
  }
  if (rc) { *out_total = 0; return rc; }
  *out_total = g_total;  // (the local call left its own total there)
  if (!gather) return VERS_OK;
  VERS_HIP_TRY(hipStreamSynchronize(st));  // (the callbacks are synchronous: the partial is in place)
  if (comm) {
    if (int32_t crc = comm->all_gather(comm->ctx, W->g_send.p, W->g_recv.p, 2 * t_max * sizeof(uint64_t)))
      return fail(VERS_ERR_COMM, "vers_comm_t::all_gather reported failure (status " + std::to_string(crc) + ")");
  }
  if (int32_t rrc = W->rg_rlims.reserve((size_t)world * nw * sizeof(uint64_t))) return rrc;
  VERS_HIP_TRY(hipMemcpy(W->rg_rlims.p, rank_lims.data(), (size_t)world * nw * sizeof(uint64_t), hipMemcpyHostToDevice));
  if (int32_t mrc = launch_range_merge(W->g_recv.as<uint64_t>(), W->g_recv.as<uint64_t>() + t_max, 2 * t_max, W->rg_rlims.as<uint64_t>(), world, b,
                                       (flags & VERS_RANGE_WALK_ORDER) != 0, out_lims_dev, out_ids_dev, out_dist_dev, st))
    return fail(mrc, who + ": the merge could not be launched");
  VERS_HIP_TRY(hipStreamSynchronize(st));
  return VERS_OK;
}

}  // extern "C++"

// the two unfiltered sharded range calls: the local part is the partial range call.  exhaustive_metric < 0: the probed lists.
static int32_t range_sharded_common(vers_ivf_t* h, const vers_comm_t* comm, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev,
                                    uint32_t nprobe, int exhaustive_metric, uint32_t flags, uint64_t* out_lims_dev, uint64_t* out_ids_dev, float* out_dist_dev,
                                    uint64_t cap, uint64_t* out_total, void* stream) {
  const char* who = exhaustive_metric >= 0 ? "vers_ivf_range_search_exhaustive_sharded_dev" : "vers_ivf_range_search_sharded_dev";
  if (h && out_total && exhaustive_metric > (int)VERS_METRIC_COSDIST) { *out_total = 0; return fail(VERS_ERR_INVALID, "unknown metric"); }
  return range_sharded_run(
      h, who, comm, queries_dev, ldq_floats, b, radius_dev, exhaustive_metric >= 0, flags, out_lims_dev, out_ids_dev, out_dist_dev, cap, out_total, stream,
      [&]() -> int32_t { return exhaustive_metric >= 0 ? range_exhaustive_check(h, who, flags, true) : range_check(h, who, nprobe, flags, true); },
      [&](uint64_t* lims, uint64_t* local_total, hipStream_t st, RangePartial* part) -> int32_t {
        return range_dev_locked(h, range_name(exhaustive_metric < 0), exhaustive_metric < 0, queries_dev, ldq_floats, b, radius_dev,
                                exhaustive_metric >= 0 ? (uint32_t)exhaustive_metric : nprobe, flags, lims, nullptr, nullptr, cap, false, local_total, st, part);
      });
}

int32_t vers_ivf_range_search_sharded_dev(vers_ivf_t* h, const vers_comm_t* comm, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev,
                                          uint32_t nprobe, uint32_t flags, uint64_t* out_lims_dev, uint64_t* out_ids_dev, float* out_dist_dev, uint64_t cap,
                                          uint64_t* out_total, void* stream) {
  return range_sharded_common(h, comm, queries_dev, ldq_floats, b, radius_dev, nprobe, -1, flags, out_lims_dev, out_ids_dev, out_dist_dev, cap, out_total, stream);
}

int32_t vers_ivf_range_search_exhaustive_sharded_dev(vers_ivf_t* h, const vers_comm_t* comm, const float* queries_dev, uint64_t ldq_floats, uint32_t b,
                                                     const float* radius_dev, uint32_t metric, uint32_t flags, uint64_t* out_lims_dev, uint64_t* out_ids_dev,
                                                     float* out_dist_dev, uint64_t cap, uint64_t* out_total, void* stream) {
  if (metric > VERS_METRIC_COSDIST) return fail(VERS_ERR_INVALID, "unknown metric");
  return range_sharded_common(h, comm, queries_dev, ldq_floats, b, radius_dev, 1, (int)metric, flags, out_lims_dev, out_ids_dev, out_dist_dev, cap, out_total, stream);
}

// ---- filtered search on handles sharded by cluster (vers_hip.h): a rank's partial of every filtered call, and the calls end to end ----
// The filters of these calls come in the _multi form, a NULL filter_of meaning one bitmap for the batch (FilterForm::kEither).
namespace {
// the local part of the top-k partial, sharded and prepared calls: this rank's partial into keys / ids.  The workspace's o_* buffers take what a partial has no use for.
int32_t shard_filtered_local(vers_ivf* h, bool probed, const float* q_dev, uint64_t ldq, uint32_t b, uint32_t top_k, uint32_t nprobe_or_metric, const FilterArg& f,
                             const AdaptiveSpec& as, uint64_t* keys, uint64_t* ids, hipStream_t st) {
  if (int32_t rc = ensure_out(h, (size_t)b * top_k, b)) return rc;
  if (probed) return filtered_dev_locked(h, q_dev, ldq, b, top_k, nprobe_or_metric, f, as, ids, W->o_dist.as<float>(), W->o_cnt.as<uint32_t>(), st, keys);
  return exhaustive_filtered_dev_locked(h, q_dev, ldq, b, top_k, nprobe_or_metric, f, W->o_ids.as<uint64_t>(), W->o_dist.as<float>(), W->o_cnt.as<uint32_t>(), st, keys, ids);
}

int32_t filtered_partial_common(vers_ivf_t* h, const char* who, bool probed, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k, uint32_t nprobe_or_metric,
                                const FilterArg& f, const vers_adaptive_t* adaptive, uint64_t* out_keys_dev, uint64_t* out_ids_dev, void* stream) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (top_k == 0) return fail(VERS_ERR_INVALID, std::string(who) + ": top_k must be at least 1");
  if (!probed && nprobe_or_metric > VERS_METRIC_COSDIST) return fail(VERS_ERR_INVALID, "unknown metric");
  if (b && (!queries_dev || ldq_floats < h->d || !out_keys_dev || !out_ids_dev)) return fail(VERS_ERR_INVALID, std::string(who) + ": bad arguments");
  const AdaptiveSpec as = adaptive_spec(adaptive);
  if (int32_t rc = adaptive_check(who, as, nprobe_or_metric, AdaptiveKind::kPartial)) return rc;
  return dev_call(
      h, b, false, stream, [&]() -> int32_t { return filtered_check(h, who, FilterCheck{probed, false, FilterForm::kEither, nullptr}, nprobe_or_metric, 0, b, f); },
      [&](hipStream_t st) -> int32_t { return shard_filtered_local(h, probed, queries_dev, ldq_floats, b, top_k, nprobe_or_metric, f, as, out_keys_dev, out_ids_dev, st); });
}

int32_t filtered_sharded_common(vers_ivf_t* h, const char* who, bool probed, const vers_gather_t* g, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k,
                                uint32_t nprobe_or_metric, const FilterArg& f, const vers_adaptive_t* adaptive, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev,
                                void* stream) {
  if (h && !probed && nprobe_or_metric > VERS_METRIC_COSDIST) return fail(VERS_ERR_INVALID, "unknown metric");
  AdaptiveSpec as = adaptive_spec(adaptive);
  if (h)
    if (int32_t rc = adaptive_check(who, as, nprobe_or_metric, AdaptiveKind::kSharded)) return rc;
  size_t count_words = 0;
  return sharded_topk_run(
      h, who, g, queries_dev, ldq_floats, b, top_k, 0, count_words, out_ids_dev, out_dist_dev, out_count_dev, stream,
      [&]() -> int32_t {
        if (int32_t rc = filtered_check(h, who, FilterCheck{probed, false, FilterForm::kEither, nullptr}, nprobe_or_metric, 0, b, f)) return rc;
        if (as.on) count_words = (size_t)f.n_sets() * h->k;
        return VERS_OK;
      },
      [&](uint64_t* keys, uint64_t* ids, const ShardReduce& reduce, hipStream_t st) -> int32_t {
        if (as.on) as.reduce = reduce;
        return shard_filtered_local(h, probed, queries_dev, ldq_floats, b, top_k, nprobe_or_metric, f, as, keys, ids, st);
      });
}

int32_t range_filtered_sharded_common(vers_ivf_t* h, const char* who, bool probed, const vers_comm_t* comm, const float* queries_dev, uint64_t ldq_floats, uint32_t b,
                                      const float* radius_dev, uint32_t nprobe_or_metric, uint32_t flags, const FilterArg& f, uint64_t* out_lims_dev, uint64_t* out_ids_dev,
                                      float* out_dist_dev, uint64_t cap, uint64_t* out_total, void* stream) {
  if (h && out_total && !probed && nprobe_or_metric > VERS_METRIC_COSDIST) { *out_total = 0; return fail(VERS_ERR_INVALID, "unknown metric"); }
  return range_sharded_run(
      h, who, comm, queries_dev, ldq_floats, b, radius_dev, !probed, flags, out_lims_dev, out_ids_dev, out_dist_dev, cap, out_total, stream,
      [&]() -> int32_t { return filtered_check(h, who, FilterCheck{probed, true, FilterForm::kEither, nullptr}, nprobe_or_metric, flags, b, f); },
      [&](uint64_t* lims, uint64_t* local_total, hipStream_t st, RangePartial* part) -> int32_t {
        return range_filtered_dev_locked(h, who, probed, queries_dev, ldq_floats, b, radius_dev, nprobe_or_metric, flags, f, lims, nullptr, nullptr, cap, false, local_total, st, part);
      });
}
}  // namespace

int32_t vers_ivf_filter_allowed_len_dev(vers_ivf_t* h, const uint64_t* filters_dev, uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits, uint32_t* out_len_dev,
                                        void* stream) {
  const char* who = "vers_ivf_filter_allowed_len_dev";
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (n_filters == 0) return fail(VERS_ERR_INVALID, std::string(who) + ": n_filters == 0");
  if (n_filters > VERS_FILTER_MAX) return fail(VERS_ERR_INVALID, std::string(who) + ": more than VERS_FILTER_MAX bitmaps in one call");
  if (n_bits != 0 && filter_stride_words < (n_bits + 63) / 64) return fail(VERS_ERR_INVALID, std::string(who) + ": filter_stride_words is smaller than ceil(n_bits / 64)");
  if (n_bits != 0 && filters_dev == nullptr) return fail(VERS_ERR_INVALID, std::string(who) + ": n_bits > 0 with NULL filters");
  std::shared_lock<std::shared_mutex> lk(h->index);
  if (h->k == 0) return VERS_OK;  // (no list: nothing to write)
  if (!out_len_dev) return fail(VERS_ERR_INVALID, std::string(who) + ": NULL out_len_dev");
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)stream;
  WsLease lease(h, true, st);
  if (lease.rc) return lease.rc;
  if (int32_t rc = lease.order_on(st)) return rc;
  FilterMasks masks;  // (one bitmap: the per-call mask; several: the per-query sets, every bitmap counted)
  if (int32_t rc = filter_begin(h, FilterArg{filters_dev, filter_stride_words, n_filters, n_bits, nullptr}, h->cap_rows, st, masks)) return rc;
  if (int32_t rc = filter_count_allowed(h, masks, n_filters, out_len_dev, st)) return rc;
  return filter_end(h, st);
}

int32_t vers_ivf_search_filtered_partial_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k, uint32_t nprobe,
                                             const uint64_t* filters_dev, uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits, const uint32_t* filter_of_dev,
                                             const vers_adaptive_t* adaptive, uint64_t* out_keys_dev, uint64_t* out_ids_dev, void* stream) {
  return filtered_partial_common(h, "vers_ivf_search_filtered_partial_dev", true, queries_dev, ldq_floats, b, top_k, nprobe,
                                 FilterArg{filters_dev, filter_stride_words, n_filters, n_bits, filter_of_dev}, adaptive, out_keys_dev, out_ids_dev, stream);
}

int32_t vers_ivf_search_exhaustive_filtered_partial_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k, uint32_t metric,
                                                        const uint64_t* filters_dev, uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits,
                                                        const uint32_t* filter_of_dev, uint64_t* out_keys_dev, uint64_t* out_ids_dev, void* stream) {
  return filtered_partial_common(h, "vers_ivf_search_exhaustive_filtered_partial_dev", false, queries_dev, ldq_floats, b, top_k, metric,
                                 FilterArg{filters_dev, filter_stride_words, n_filters, n_bits, filter_of_dev}, nullptr, out_keys_dev, out_ids_dev, stream);
}

int32_t vers_ivf_search_filtered_sharded_dev(vers_ivf_t* h, const vers_gather_t* g, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k, uint32_t nprobe,
                                             const uint64_t* filters_dev, uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits, const uint32_t* filter_of_dev,
                                             const vers_adaptive_t* adaptive, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev, void* stream) {
  return filtered_sharded_common(h, "vers_ivf_search_filtered_sharded_dev", true, g, queries_dev, ldq_floats, b, top_k, nprobe,
                                 FilterArg{filters_dev, filter_stride_words, n_filters, n_bits, filter_of_dev}, adaptive, out_ids_dev, out_dist_dev, out_count_dev, stream);
}

int32_t vers_ivf_search_exhaustive_filtered_sharded_dev(vers_ivf_t* h, const vers_gather_t* g, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k,
                                                        uint32_t metric, const uint64_t* filters_dev, uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits,
                                                        const uint32_t* filter_of_dev, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev, void* stream) {
  return filtered_sharded_common(h, "vers_ivf_search_exhaustive_filtered_sharded_dev", false, g, queries_dev, ldq_floats, b, top_k, metric,
                                 FilterArg{filters_dev, filter_stride_words, n_filters, n_bits, filter_of_dev}, nullptr, out_ids_dev, out_dist_dev, out_count_dev, stream);
}

int32_t vers_ivf_range_search_filtered_partial_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev, uint32_t nprobe,
                                                   uint32_t flags, const uint64_t* filters_dev, uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits,
                                                   const uint32_t* filter_of_dev, uint64_t* out_lims_dev, uint64_t* out_keys_dev, uint64_t* out_ids_dev, uint64_t cap,
                                                   uint64_t* out_total, void* stream) {
  const char* who = "vers_ivf_range_search_filtered_partial_dev";
  return range_filtered_dev_common(h, who, who, true, FilterForm::kEither, queries_dev, ldq_floats, b, radius_dev, nprobe, flags,
                                   FilterArg{filters_dev, filter_stride_words, n_filters, n_bits, filter_of_dev}, out_lims_dev, out_keys_dev, out_ids_dev, nullptr, cap, out_total,
                                   stream);
}

int32_t vers_ivf_range_search_exhaustive_filtered_partial_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev, uint32_t metric,
                                                              uint32_t flags, const uint64_t* filters_dev, uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits,
                                                              const uint32_t* filter_of_dev, uint64_t* out_lims_dev, uint64_t* out_keys_dev, uint64_t* out_ids_dev,
                                                              uint64_t cap, uint64_t* out_total, void* stream) {
  const char* who = "vers_ivf_range_search_exhaustive_filtered_partial_dev";
  return range_filtered_dev_common(h, who, who, false, FilterForm::kEither, queries_dev, ldq_floats, b, radius_dev, metric, flags,
                                   FilterArg{filters_dev, filter_stride_words, n_filters, n_bits, filter_of_dev}, out_lims_dev, out_keys_dev, out_ids_dev, nullptr, cap, out_total,
                                   stream);
}

int32_t vers_ivf_range_search_filtered_sharded_dev(vers_ivf_t* h, const vers_comm_t* comm, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev,
                                                   uint32_t nprobe, uint32_t flags, const uint64_t* filters_dev, uint64_t filter_stride_words, uint32_t n_filters,
                                                   uint64_t n_bits, const uint32_t* filter_of_dev, uint64_t* out_lims_dev, uint64_t* out_ids_dev, float* out_dist_dev,
                                                   uint64_t cap, uint64_t* out_total, void* stream) {
  return range_filtered_sharded_common(h, "vers_ivf_range_search_filtered_sharded_dev", true, comm, queries_dev, ldq_floats, b, radius_dev, nprobe, flags,
                                       FilterArg{filters_dev, filter_stride_words, n_filters, n_bits, filter_of_dev}, out_lims_dev, out_ids_dev, out_dist_dev, cap, out_total,
                                       stream);
}

int32_t vers_ivf_range_search_exhaustive_filtered_sharded_dev(vers_ivf_t* h, const vers_comm_t* comm, const float* queries_dev, uint64_t ldq_floats, uint32_t b,
                                                              const float* radius_dev, uint32_t metric, uint32_t flags, const uint64_t* filters_dev,
                                                              uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits, const uint32_t* filter_of_dev,
                                                              uint64_t* out_lims_dev, uint64_t* out_ids_dev, float* out_dist_dev, uint64_t cap, uint64_t* out_total,
                                                              void* stream) {
  return range_filtered_sharded_common(h, "vers_ivf_range_search_exhaustive_filtered_sharded_dev", false, comm, queries_dev, ldq_floats, b, radius_dev, metric, flags,
                                       FilterArg{filters_dev, filter_stride_words, n_filters, n_bits, filter_of_dev}, out_lims_dev, out_ids_dev, out_dist_dev, cap, out_total,
                                       stream);
}

// ---- prepared filters (vers_hip.h): the object's lifecycle, and the four searches that take it ----
namespace {
// is `f` one of h's live objects?  (an object of another handle, or one destroyed already, is not in the registry)
bool filter_is_ours(vers_ivf* h, const vers_filter* f) {
  std::lock_guard<std::mutex> lk(h->flt_mu);
  return std::find(h->filters.begin(), h->filters.end(), f) != h->filters.end();
}

int32_t filter_prepare_common(vers_ivf_t* h, const char* who_c, const uint64_t* filters, bool on_device, uint64_t stride_words, uint32_t n_filters, uint64_t n_bits,
                              vers_filter_t** out) {
  const std::string who = who_c;
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (!out) return fail(VERS_ERR_INVALID, who + ": NULL out");
  *out = nullptr;
  if (n_filters == 0) return fail(VERS_ERR_INVALID, who + ": n_filters == 0");
  if (n_filters > VERS_FILTER_MAX) return fail(VERS_ERR_INVALID, who + ": more than VERS_FILTER_MAX bitmaps in one object; split by allowed set");
  if (n_bits != 0 && stride_words < (n_bits + 63) / 64) return fail(VERS_ERR_INVALID, who + ": filter_stride_words is smaller than ceil(n_bits / 64)");
  if (n_bits != 0 && filters == nullptr) return fail(VERS_ERR_INVALID, who + ": n_bits > 0 with NULL filters");
  std::shared_lock<std::shared_mutex> lk(h->index);
  DeviceGuard g(h->device);
  std::unique_ptr<vers_filter> o(new (std::nothrow) vers_filter());
  if (!o) return fail(VERS_ERR_INVALID, "out of host memory");
  o->owner = h;
  o->n_filters = n_filters;
  o->n_bits = n_bits;
  o->words = std::max<uint64_t>(1, (n_bits + 63) / 64);
  VERS_HIP_TRY(hipEventCreateWithFlags(&o->ready, hipEventDisableTiming));
  if (int32_t rc = o->bits.reserve((size_t)n_filters * o->words * sizeof(uint64_t))) return rc;
  if (n_bits == 0) VERS_HIP_TRY(hipMemset(o->bits.p, 0, (size_t)n_filters * o->words * sizeof(uint64_t)));
  else  // the object's own copy, packed: the caller's array may change or go
    VERS_HIP_TRY(hipMemcpy2D(o->bits.p, o->words * sizeof(uint64_t), filters, stride_words * sizeof(uint64_t), o->words * sizeof(uint64_t), n_filters,
                             on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  WsLease lease(h, true, nullptr);
  if (lease.rc) return lease.rc;
  if (int32_t rc = lease.order_on(nullptr)) return rc;
  W->ev_on = false;  // (no search: nothing for the scan-timing ring)
  // the masks for the index as it stands, in the form the object's first search can ask for without a second pass being likelier
  if (int32_t rc = prepared_sync(h, o.get(), n_filters == 1 ? 0 : 1, false, nullptr)) return rc;
  VERS_HIP_TRY(hipStreamSynchronize(nullptr));
  o->pending = false;
  {
    std::lock_guard<std::mutex> rk(h->flt_mu);
    h->filters.push_back(o.get());
  }
  *out = o.release();
  return VERS_OK;
}

// what the four prepared searches refuse on top of the _filtered_sharded_dev calls' checks
int32_t prepared_check(vers_ivf_t* h, const char* who, const vers_filter_t* f) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (!f) return fail(VERS_ERR_INVALID, std::string(who) + ": NULL filter object");
  if (!filter_is_ours(h, f)) return fail(VERS_ERR_INVALID, std::string(who) + ": the filter object was not prepared on this handle (or is destroyed)");
  {
    std::shared_lock<std::shared_mutex> lk(h->index);
    if (h->world > 1)
      return fail(VERS_ERR_INVALID, std::string(who) + ": the handle is sharded by cluster; prepared filters on a sharded handle are out of scope (use the _filtered_sharded_dev calls)");
  }
  return VERS_OK;
}
}  // namespace

int32_t vers_ivf_filter_prepare(vers_ivf_t* h, const uint64_t* filters, uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits, vers_filter_t** out) {
  return filter_prepare_common(h, "vers_ivf_filter_prepare", filters, false, filter_stride_words, n_filters, n_bits, out);
}

int32_t vers_ivf_filter_prepare_dev(vers_ivf_t* h, const uint64_t* filters_dev, uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits, vers_filter_t** out) {
  return filter_prepare_common(h, "vers_ivf_filter_prepare_dev", filters_dev, true, filter_stride_words, n_filters, n_bits, out);
}

int32_t vers_ivf_filter_refresh(vers_ivf_t* h, vers_filter_t* f, void* stream) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (!f || !filter_is_ours(h, f)) return fail(VERS_ERR_INVALID, "vers_ivf_filter_refresh: not a filter object of this handle");
  std::shared_lock<std::shared_mutex> lk(h->index);
  DeviceGuard g(h->device);
  WsLease lease(h, true, (hipStream_t)stream);
  if (lease.rc) return lease.rc;
  if (int32_t rc = lease.order_on((hipStream_t)stream)) return rc;
  W->ev_on = false;  // (no search: nothing for the scan-timing ring)
  return prepared_sync(h, f, -1, false, (hipStream_t)stream);
}

int32_t vers_ivf_filter_info(vers_ivf_t* h, const vers_filter_t* f, uint64_t* out8) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (!f || !out8 || !filter_is_ours(h, f)) return fail(VERS_ERR_INVALID, "vers_ivf_filter_info: not a filter object of this handle, or NULL out8");
  std::shared_lock<std::shared_mutex> lk(h->index);
  vers_filter_t* o = const_cast<vers_filter_t*>(f);
  std::lock_guard<std::mutex> ok(o->mu);
  out8[0] = o->n_filters; out8[1] = o->n_bits; out8[2] = o->device_bytes(); out8[3] = o->builds; out8[4] = o->tails; out8[5] = o->hits;
  out8[6] = (o->built && o->seen_moved == h->flt_moved && o->seen_appended == h->flt_appended) ? 1 : 0;
  out8[7] = 0;
  return VERS_OK;
}

int32_t vers_ivf_filter_destroy(vers_ivf_t* h, vers_filter_t* f) {
  if (!h) return fail(VERS_ERR_INVALID, "null handle");
  if (!f) return VERS_OK;
  {
    std::lock_guard<std::mutex> lk(h->flt_mu);
    auto it = std::find(h->filters.begin(), h->filters.end(), f);
    if (it == h->filters.end()) return fail(VERS_ERR_INVALID, "vers_ivf_filter_destroy: not a filter object of this handle");
    h->filters.erase(it);
  }
  DeviceGuard g(h->device);
  (void)hipDeviceSynchronize();  // searches in flight on any stream may still read the object's arrays
  delete f;
  return VERS_OK;
}

int32_t vers_ivf_search_prepared_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k, uint32_t nprobe, const vers_filter_t* f,
                                     const uint32_t* filter_of_dev, const vers_adaptive_t* adaptive, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev,
                                     void* stream) {
  const char* who = "vers_ivf_search_prepared_dev";
  if (int32_t rc = prepared_check(h, who, f)) return rc;
  const FilterArg sf = prepared_filter(f, filter_of_dev);
  return filtered_sharded_common(h, who, true, nullptr, queries_dev, ldq_floats, b, top_k, nprobe, sf, adaptive, out_ids_dev, out_dist_dev,
                                 out_count_dev, stream);
}

int32_t vers_ivf_search_exhaustive_prepared_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k, uint32_t metric,
                                                const vers_filter_t* f, const uint32_t* filter_of_dev, uint64_t* out_ids_dev, float* out_dist_dev,
                                                uint32_t* out_count_dev, void* stream) {
  const char* who = "vers_ivf_search_exhaustive_prepared_dev";
  if (int32_t rc = prepared_check(h, who, f)) return rc;
  const FilterArg sf = prepared_filter(f, filter_of_dev);
  return filtered_sharded_common(h, who, false, nullptr, queries_dev, ldq_floats, b, top_k, metric, sf, nullptr, out_ids_dev, out_dist_dev,
                                 out_count_dev, stream);
}

int32_t vers_ivf_range_search_prepared_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev, uint32_t nprobe,
                                           uint32_t flags, const vers_filter_t* f, const uint32_t* filter_of_dev, uint64_t* out_lims_dev, uint64_t* out_ids_dev,
                                           float* out_dist_dev, uint64_t cap, uint64_t* out_total, void* stream) {
  const char* who = "vers_ivf_range_search_prepared_dev";
  if (int32_t rc = prepared_check(h, who, f)) return rc;
  const FilterArg sf = prepared_filter(f, filter_of_dev);
  return range_filtered_sharded_common(h, who, true, nullptr, queries_dev, ldq_floats, b, radius_dev, nprobe, flags, sf, out_lims_dev,
                                       out_ids_dev, out_dist_dev, cap, out_total, stream);
}

int32_t vers_ivf_range_search_exhaustive_prepared_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev,
                                                      uint32_t metric, uint32_t flags, const vers_filter_t* f, const uint32_t* filter_of_dev, uint64_t* out_lims_dev,
                                                      uint64_t* out_ids_dev, float* out_dist_dev, uint64_t cap, uint64_t* out_total, void* stream) {
  const char* who = "vers_ivf_range_search_exhaustive_prepared_dev";
  if (int32_t rc = prepared_check(h, who, f)) return rc;
  const FilterArg sf = prepared_filter(f, filter_of_dev);
  return range_filtered_sharded_common(h, who, false, nullptr, queries_dev, ldq_floats, b, radius_dev, metric, flags, sf, out_lims_dev,
                                       out_ids_dev, out_dist_dev, cap, out_total, stream);
}

int32_t vers_range_phases(double* out8, int32_t reset) {
  std::lock_guard<std::mutex> lk(g_rg_mu);
  if (out8)
    for (int i = 0; i < kRangePhases; ++i) out8[i] = g_rg[i];
  if (reset)
    for (double& v : g_rg) v = 0.0;
  return VERS_OK;
}

}  // extern "C"
