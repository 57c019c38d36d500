// update_plan.hpp -- the index arithmetic of vers_ivf_update_batch (ivf_build.hip): which list a storage row belongs to, whether an
// updated row stays or moves, where the rows of a list that gains rows end up (the in-place BACKWARD merge, the mirror image of
// remove_compact_kernel), which tiles that touches, the lists' new lengths and the grow decision.  No HIP dependency: the kernels include
// it, and the host compiler alone builds it (tests/cpp/update_plan_demo.cpp emulates the merge tile by tile with these functions).
//
// A list that gains rows holds `len` old rows (ascending vec id, the movers that leave already compacted away) and receives n_in new rows,
// sorted by vec id.  pos[t] = #old ids < v_t (the reference's partition_point) is non-decreasing in t, so
//   new row t  -> pos[t] + t                       strictly increasing in t
//   old row s  -> s + #{t : pos[t] <= s}           (v_t < id_s  <=>  pos[t] <= s)
// and every destination is >= its source: walking the destination tiles in DESCENDING order, the sources of a tile lie in that tile or in
// front of it, where nothing has been written yet.  Rows in front of pos[0] do not move.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VERS_UPD_HD __host__ __device__
#else
#define VERS_UPD_HD
#endif

namespace vers {
namespace upd {

constexpr uint32_t kNone = 0xFFFFFFFFu;    // no row: slack behind a list / a vec id without an update
constexpr uint32_t kNewBit = 0x80000000u;  // merge_source: the row comes from the call's rows, not from the list (a list holds < 2^31 rows)

// status of one update (vers_hip.h)
constexpr uint8_t kStayed = 0, kMoved = 1, kSkipped = 2;

// the list of storage row r: the last list with list_off <= r (lists without storage share their offset with the next one that has some)
VERS_UPD_HD inline uint32_t list_of_row(const uint32_t* list_off, uint32_t k, uint64_t r) {
  uint32_t lo = 0, hi = k;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (list_off[mid] <= r) lo = mid;
    else hi = mid;
  }
  return lo;
}

// locate: a stored row whose id has an update stays when its first-minimum centroid is the list it lies in
VERS_UPD_HD inline uint8_t classify(uint32_t list_now, uint32_t list_new) { return list_now == list_new ? kStayed : kMoved; }

// #ids < v among ids[0 .. len), ascending: ids[c].partition_point(|&y| y < v)
VERS_UPD_HD inline uint32_t insertion_point(const uint32_t* ids, uint32_t len, uint32_t v) {
  uint32_t lo = 0, hi = len;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (ids[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

VERS_UPD_HD inline uint32_t new_row_dest(const uint32_t* pos, uint32_t t) { return pos[t] + t; }

// #{t : pos[t] + t < j}: the new rows placed in front of destination row j
VERS_UPD_HD inline uint32_t new_rows_before(const uint32_t* pos, uint32_t n_in, uint32_t j) {
  uint32_t lo = 0, hi = n_in;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (pos[mid] + mid < j) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

VERS_UPD_HD inline uint32_t old_row_dest(const uint32_t* pos, uint32_t n_in, uint32_t s) {
  uint32_t lo = 0, hi = n_in;  // #{t : pos[t] <= s}
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (pos[mid] <= s) lo = mid + 1;
    else hi = mid;
  }
  return s + lo;
}

// what destination row j of the merged list holds: kNewBit | t (new row t), s (old row s <= j), kNone (slack: j >= len + n_in)
VERS_UPD_HD inline uint32_t merge_source(const uint32_t* pos, uint32_t n_in, uint32_t len, uint32_t j) {
  const uint32_t t = new_rows_before(pos, n_in, j);
  if (t < n_in && pos[t] + t == j) return kNewBit | t;
  const uint32_t s = j - t;
  return s < len ? s : kNone;
}

// the destination tiles (list-relative) the merge writes: [first, last], walked from last down to first (n_in >= 1)
VERS_UPD_HD inline uint32_t merge_first_tile(const uint32_t* pos) { return pos[0] / 64u; }
VERS_UPD_HD inline uint32_t merge_last_tile(uint32_t len, uint32_t n_in) { return (len + n_in - 1u) / 64u; }

// lengths after the movers left (mid) and after they arrived (fin); true when a list outgrows its capacity (one re-layout, before placement)
inline bool plan_lengths(const uint32_t* len, const uint32_t* out_cnt, const uint32_t* in_cnt, const uint32_t* cap, uint32_t k, uint32_t* mid, uint32_t* fin) {
  bool grow = false;
  for (uint32_t c = 0; c < k; ++c) {
    mid[c] = len[c] - out_cnt[c];
    fin[c] = mid[c] + in_cnt[c];
    if (fin[c] > cap[c]) grow = true;
  }
  return grow;
}

}  // namespace upd
}  // namespace vers
