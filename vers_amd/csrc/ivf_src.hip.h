// ivf_src.hip.h -- how the scan engine (scan.hip.h) sees the index: work-item sources of the coarse quantiser / exhaustive scan
// (SegSrc), the inverted-list scans (IvfSrc) and the single query's item records (Item1Rec / Rec1Src), + what the host
// needs to launch them on a leased workspace: the timing ring's bracket, the parameter and source fills, and the launch of a segment scan,
// which the planner (coarse quantiser) and the search (exhaustive scan) share.
#pragma once
#include "ivf_handle.hpp"
#include "scan_launch.hip.h"

namespace vers {

// ---- sources for the scan engine -----------------------------------------------------------
// coarse quantiser / exhaustive scan: item = (row segment, query group), slot(q, seg) = q*n_segs + seg;
// QG > 1: segments padded to a multiple of 4 with empty items (quads share a query block, scan.hip.h)
template <int QG, bool SEQ_IDS>
struct SegSrc {
  static constexpr bool kSeqIds = SEQ_IDS;
  static constexpr bool kStreamOnce = SEQ_IDS;  // exhaustive scan of the stored rows: once; coarse quantiser: centroids are re-read
  const float* rows;
  uint64_t n;
  uint32_t ld;
  uint32_t seg_rows, n_segs, n_segs_pad;
  const float* queries;  // QG == 1: [b][ldq]; else interleaved blocks
  uint32_t ldq, b;
  uint64_t* partials;
  uint32_t k;
  const uint32_t* ids;
  __device__ __forceinline__ uint32_t n_items() const { return n_segs_pad * ((b + QG - 1) / QG); }
  __device__ __forceinline__ void get(uint32_t it, ItemView<QG>& v) const {
    const uint32_t seg = it % n_segs_pad, qg = it / n_segs_pad;
    const bool real = seg < n_segs;
    const uint64_t row0 = real ? (uint64_t)seg * seg_rows : 0;
    v.rows = rows + row0 * ld;
    v.nrows = real ? (uint32_t)((n - row0 < seg_rows) ? (n - row0) : seg_rows) : 0u;
    const uint32_t q0 = qg * QG;
    v.nq = (b - q0 < (uint32_t)QG) ? (b - q0) : QG;
    v.qb = queries + (uint64_t)qg * ldq * QG;
  }
  __device__ __forceinline__ uint32_t seq_base(uint32_t it, int) const { return (it % n_segs_pad) * seg_rows; }
  __device__ __forceinline__ const uint32_t* seq_ids(uint32_t it) const { return ids + (uint64_t)(it % n_segs_pad) * seg_rows; }
  __device__ __forceinline__ uint64_t* out(uint32_t it, int qi) const {
    const uint32_t seg = it % n_segs_pad, qg = it / n_segs_pad;
    return partials + ((uint64_t)(qg * QG + qi) * n_segs + seg) * k;
  }
  __device__ __forceinline__ uint32_t bound_slot(uint32_t it, int qi) const { return (it / n_segs_pad) * QG + qi; }
  // range walk (range.hip.h): storage rows of the index, slack and freed rows among them
  static constexpr int kRangeRows = kRangeRowsStored;
  __device__ __forceinline__ uint32_t range_query(uint32_t it, int qi) const { return (it / n_segs_pad) * QG + qi; }
  __device__ __forceinline__ uint64_t range_slot(uint32_t it, int qi) const { return (uint64_t)range_query(it, qi) * n_segs + it % n_segs_pad; }
  __device__ __forceinline__ uint32_t storage_row(uint32_t it) const { return (it % n_segs_pad) * seg_rows; }
};

// inverted-list scan: item = (list, query group of the list, row segment of the list)
template <int QG>
struct IvfSrc {
  static constexpr bool kSeqIds = false;
  static constexpr bool kStreamOnce = true;
  const float* rows;
  uint32_t ld;
  const uint32_t* list_off;  // storage row of each (local) list
  const uint32_t* list_len;
  const ItemDesc* items;
  const GroupTotals* totals;   // the batch's totals on the device (group_scatter_kernel): the work order's length and its hot part
  const uint32_t* cnt;        // pairs per list
  const uint32_t* pair_off;   // first pair of each list
  const uint32_t* pairs;      // pair -> q*P + j
  const uint32_t* group_off;  // first group id of each list
  const float* qblocks;       // QG > 1: [group][ldq][QG]
  const float* qp;            // QG == 1: padded queries [b][ldq]
  uint32_t ldq, P, S_max, k_keep, seg_rows, seg_target;
  uint32_t bound_per_pair;    // reference mode merges per (query, list); nprobe mode per query
  const uint32_t* pj_pref;    // [b*P] sequence base of probe j of query q
  uint64_t* partials;         // [b*P*S_max][k_keep]

  __device__ __forceinline__ uint32_t n_items() const { return totals->n_items; }
  __device__ __forceinline__ uint32_t hot_items() const { return totals->hot_items; }  // items of the hot lists, the first of the work order
  __device__ __forceinline__ void get(uint32_t it, ItemView<QG>& v) const {
    const ItemDesc d = items[it];
    const bool real = d.seg != kNoSeg;
    const uint32_t len = list_len[d.list];
    const uint32_t sr = list_seg_rows(len, seg_rows, seg_target);
    const uint32_t r0 = real ? d.seg * sr : 0;
    v.rows = rows + ((uint64_t)list_off[d.list] + r0) * ld;
    v.row0 = r0;
    v.nrows = real ? (len - r0 < sr ? len - r0 : sr) : 0u;
    const uint32_t c = cnt[d.list] - d.group * QG;
    v.nq = c < (uint32_t)QG ? c : QG;
    if (QG == 1) v.qb = qp + (uint64_t)(pairs[pair_off[d.list] + d.group] / P) * ldq;
    else v.qb = qblocks + (uint64_t)(group_off[d.list] + d.group) * ldq * QG;
  }
  __device__ __forceinline__ uint32_t pair_of(uint32_t it, int qi) const {
    const ItemDesc d = items[it];
    return pairs[pair_off[d.list] + d.group * QG + qi];
  }
  __device__ __forceinline__ uint32_t query_index(uint32_t it, uint32_t qi) const {  // the batch's query in slot qi
    const ItemDesc d = items[it];
    return pairs[pair_off[d.list] + d.group * QG + qi] / P;
  }
  __device__ __forceinline__ const float* query_row(uint32_t it, uint32_t qi) const {  // padded query of slot qi
    const ItemDesc d = items[it];
    return qp + (uint64_t)(pairs[pair_off[d.list] + d.group * QG + qi] / P) * ldq;
  }
  __device__ __forceinline__ uint32_t storage_row(uint32_t it) const {  // first storage row of the item
    const ItemDesc d = items[it];
    return list_off[d.list] + (d.seg != kNoSeg ? d.seg * list_seg_rows(list_len[d.list], seg_rows, seg_target) : 0u);
  }
  // get's v.nrows and storage_row of a descriptor ALREADY loaded, for the head filter's look-ahead (head_filter.hip.h), which requests
  // the descriptor a quad early.  The rule is the two functions' above, restated beside them and not shared with them: the list scan's
  // kernels are held to their register figures, and routing get through a helper moved two of them.  tests/test_head_stream_gpu.py
  // fails on any difference (a wrong segment gives wrong verdicts).
  __device__ __forceinline__ void seg_span(const ItemDesc& d, uint32_t& row_s, uint32_t& nrows) const {
    const bool real = d.seg != kNoSeg;
    const uint32_t len = list_len[d.list];
    const uint32_t sr = list_seg_rows(len, seg_rows, seg_target);
    const uint32_t r0 = real ? d.seg * sr : 0;
    row_s = list_off[d.list] + r0;
    nrows = real ? (len - r0 < sr ? len - r0 : sr) : 0u;
  }
  __device__ __forceinline__ uint32_t seq_base(uint32_t it, int qi) const {
    const ItemDesc d = items[it];
    return pj_pref[pairs[pair_off[d.list] + d.group * QG + qi]] + d.seg * list_seg_rows(list_len[d.list], seg_rows, seg_target);
  }
  __device__ __forceinline__ const uint32_t* seq_ids(uint32_t) const { return nullptr; }
  __device__ __forceinline__ uint64_t* out(uint32_t it, int qi) const {  // ordered-chain scan: S_max counts segments
    return partials + ((uint64_t)pair_of(it, qi) * S_max + items[it].seg) * k_keep;
  }
  // slot of a whole quad of segments (matrix-core scan: one list per query and block); S_max counts quads there
  __device__ __forceinline__ uint64_t* out_quad(uint32_t it0, int qi) const {
    return partials + ((uint64_t)pair_of(it0, qi) * S_max + (items[it0].seg >> 2)) * k_keep;
  }
  __device__ __forceinline__ uint32_t bound_slot(uint32_t it, int qi) const {
    const uint32_t pr = pair_of(it, qi);
    return bound_per_pair ? pr : pr / P * P;
  }
  __device__ __forceinline__ uint32_t slot_of_pair(uint32_t pr) const { return bound_per_pair ? pr : pr / P * P; }
  // range walk (range.hip.h): the rows of a list are all live; slot = pair * S_max + segment
  static constexpr int kRangeRows = kRangeRowsListed;
  __device__ __forceinline__ uint32_t range_query(uint32_t it, int qi) const { return pair_of(it, qi) / P; }
  __device__ __forceinline__ uint64_t range_slot(uint32_t it, int qi) const { return (uint64_t)pair_of(it, qi) * S_max + items[it].seg; }
};

// Single query (planned by plan1_block): an item is a 16-byte RECORD -- where its rows are, how many, the sequence number of the
// first and its partial slot -- so that a wave reaches its first tile load after ONE round trip.  Through IvfSrc it is five
// dependent ones (item count -> item -> the list's tables -> pair -> sequence base): ~3 us of a 58 us launch in which every wave
// has exactly one item.
struct Item1Rec {
  uint32_t row0;   // storage row of the item's first row
  uint32_t nrows;
  uint32_t seq0;   // sequence number of the first row (the probe's base + the segment's offset in its list)
  uint32_t out;    // partial slot, in units of k_keep keys: pair * S_max + segment
};
struct Rec1Src {  // what scan_item asks of its source, answered from the record in registers
  static constexpr bool kSeqIds = false;
  static constexpr bool kStreamOnce = true;
  Item1Rec r;
  uint64_t* partials;
  uint32_t k_keep, S_max, bound_per_pair;
  __device__ __forceinline__ uint32_t seq_base(uint32_t, int) const { return r.seq0; }
  __device__ __forceinline__ const uint32_t* seq_ids(uint32_t) const { return nullptr; }
  __device__ __forceinline__ uint64_t* out(uint32_t, int) const { return partials + (uint64_t)r.out * k_keep; }
  __device__ __forceinline__ uint32_t bound_slot(uint32_t, int) const { return bound_per_pair ? r.out / S_max : 0u; }
};
struct Scan1Args {
  const float* rows; const Item1Rec* recs; const uint32_t* n_items_dev; const float* qp;
  uint64_t* partials; uint32_t k_keep, S_max, bound_per_pair;
};

}  // namespace vers

namespace vers {
namespace ivf {

// ---- launching the index's scans (the leased workspace W: status word, timing ring, hand-out counter) -------------------------------
// The bracket of the scan-timing ring (vers_ivf_scan_times, option "scan_events") around whatever launch() queues on st: a record before it
// and, when it succeeded, one behind it and a ring entry more.
template <class F>
inline int32_t timed_scan(hipStream_t st, F&& launch) {
  const uint32_t slot = (uint32_t)(W->ev_count % SearchWs::kEvRing);
  if (W->ev_on) VERS_HIP_TRY(hipEventRecord(W->ev0[slot], st));
  if (int32_t rc = launch()) return rc;
  if (W->ev_on) {
    VERS_HIP_TRY(hipEventRecord(W->ev1[slot], st));
    W->ev_count += 1;
  }
  return VERS_OK;
}
// launch_scan inside the bracket (the launch attribute is set ahead of it)
template <class K, class... A>
inline int32_t launch_scan_timed(K kern, uint32_t blocks, int waves, size_t lds, hipStream_t st, const A&... args) {
  if (int32_t rc = scan_prepare_launch(kern, lds)) return rc;
  return timed_scan(st, [&]() -> int32_t {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(kWave * waves), lds, st, args...);
    VERS_HIP_TRY(hipGetLastError());
    return VERS_OK;
  });
}

// what every scan of the index's rows shares; as it stands: no pruning bounds, no hand-out counter, no diagnosis switches
inline ScanParams ivf_scan_params(const vers_ivf* h, uint32_t k, const uint64_t* lower) {
  ScanParams p;
  p.ld = h->ld;
  p.n_chunks = h->ld / kChunk;
  p.k = k;
  p.status = W->st_word();
  p.debug = 0;
  p.stamps = nullptr;
  p.bounds = nullptr;
  p.lower = lower;  // (results of more than 64 keys: 64 ranks per pass)
  p.next_quad = nullptr;
  return p;
}
// the batched kernels' dynamic quad hand-out: the workspace's counter, zeroed on st for the launch that follows
inline int32_t fresh_quad_counter(hipStream_t st, uint32_t** out) {
  if (int32_t rc = W->quad_counter.reserve(16)) return rc;
  VERS_HIP_TRY(hipMemsetAsync(W->quad_counter.p, 0, 16, st));
  *out = W->quad_counter.as<uint32_t>();
  return VERS_OK;
}

// the planned items of a search as the list-scan kernels see them.  bound_per_pair: pruning bounds (and merges) per (query, list) -- the
// reference's own mode -- instead of per query
template <int QG>
inline IvfSrc<QG> make_ivf_src(const vers_ivf* h, const SearchPlan& s, uint32_t bound_per_pair) {
  IvfSrc<QG> src;
  src.rows = h->rows.as<float>(); src.ld = h->ld; src.list_off = h->slot_off.as<uint32_t>();  // (items name lists by slot)
  src.list_len = h->slot_len.as<uint32_t>(); src.items = W->items.as<ItemDesc>(); src.totals = s.tot;
  src.cnt = s.cnt; src.pair_off = s.pair_off; src.pairs = W->pairs.as<uint32_t>(); src.group_off = s.group_off;
  src.qblocks = W->qblocks.as<float>(); src.qp = s.qp; src.ldq = h->ldq; src.P = s.P; src.S_max = s.S_max; src.k_keep = s.k_keep;
  src.seg_rows = s.seg_rows; src.seg_target = s.seg_target; src.pj_pref = s.pj_pref; src.partials = W->partials.as<uint64_t>();
  src.bound_per_pair = bound_per_pair;
  return src;
}

// a segment scan (coarse quantiser, exhaustive scan); not timed.  Items of a query are concurrent: nothing to prune, and the atomics of a
// shared bound would contend
template <int QG, bool SEQ_IDS>
int32_t launch_seg_scan(vers_ivf* h, const SegSrc<QG, SEQ_IDS>& src, uint32_t n_items, int metric, hipStream_t st,
                        const uint64_t* lower = nullptr) {
  const ScanParams p = ivf_scan_params(h, src.k, lower);
  return with_metric(metric, [&](auto m) -> int32_t {
    return launch_scan(scan_kernel<QG, decltype(m)::value, SegSrc<QG, SEQ_IDS>>, scan_grid(h->n_cu, QG, h->ld, n_items), kWavesPerBlock, scan_lds_bytes(QG, h->ld), st, src, p);
  });
}

}  // namespace ivf
}  // namespace vers
