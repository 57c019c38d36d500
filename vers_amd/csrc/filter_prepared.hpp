// filter_prepared.hpp -- the host part of a prepared filter's TAIL REFRESH (filter_prepared.hip.h), without HIP types: which lists grew since
// the object's snapshot, the tiles of each that can hold a changed bit, and the shortcut that makes the refresh free.
//
// Between the snapshot and now only add / add_batch ran, and only in place (vers_ivf::flt_appended moved, flt_moved did not): cap_rows,
// list_off and every row below snap_len[L] are what they were.  The rows [snap_len[L], len[L]) of every OWNED list that grew are the only
// rows whose mask bits can differ, and they hold the vec ids first_new_id, first_new_id + 1, ... handed out since.  Ids at or beyond n_bits
// are not allowed whatever the bitmaps say, and a slack row's bits were 0 already: if first_new_id >= n_bits the plan is EMPTY.
#pragma once
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define VERS_TAIL_HD __host__ __device__
#else
#define VERS_TAIL_HD
#endif

namespace vers {

// One wave's work: list `list` grew from old_len to new_len rows (old_len < new_len).
struct TailItem {
  uint32_t list, old_len, new_len;
};
// the list-relative 64-row tiles an item covers, first and last (lists start on tile boundaries: a storage tile belongs to one list)
VERS_TAIL_HD inline uint32_t tail_first_tile(const TailItem& it) { return it.old_len / 64u; }
VERS_TAIL_HD inline uint32_t tail_last_tile(const TailItem& it) { return (it.new_len - 1u) / 64u; }

// snap_len / len: [k] list lengths at the snapshot and now (the handle's GLOBAL lengths: those of a list another rank stores grow too, and
// are skipped -- owner nullable = every list is this rank's).  Appends the items to `out` in list order; returns the rows they cover.
inline uint64_t filter_tail_plan(const uint32_t* snap_len, const uint32_t* len, const uint8_t* owner, uint32_t rank, uint32_t k, uint64_t first_new_id,
                                 uint64_t n_bits, std::vector<TailItem>& out) {
  if (first_new_id >= n_bits) return 0;  // no new row can be allowed
  uint64_t rows = 0;
  for (uint32_t L = 0; L < k; ++L) {
    if (owner != nullptr && (uint32_t)owner[L] != rank) continue;
    if (len[L] <= snap_len[L]) continue;
    out.push_back(TailItem{L, snap_len[L], len[L]});
    rows += len[L] - snap_len[L];
  }
  return rows;
}

}  // namespace vers
