// fetch_plan.hpp -- the host part of vers_ivf_fetch's vec id -> storage row map (ivf_fetch.hip, fetch.hip.h), without HIP types: how a map
// made earlier is brought up to date, and the tile jobs of the pass over row_ids that does it.
//
// The map is read-side state, like a prepared filter: no mutator touches it, and it is judged against the two counters the mutators keep
// for the prepared filters (vers_ivf::flt_moved / flt_appended):
//   flt_moved changed            a storage row may hold another vector, or the tables changed   -> FULL rebuild
//   only flt_appended changed    add / add_batch wrote rows into list slack in place: cap_rows, list_off and every row below the
//                                snapshot's lengths are what they were                          -> the APPENDED id range alone
//   neither changed              (an update_batch in which every row stayed changes values, not places) -> valid as it is
// A pass covers only rows below their list's length -- what a slack row's row_ids entry holds is never looked at.
#pragma once
#include <cstdint>
#include <vector>

namespace vers {

enum class MapRefresh : int { kNone = 0, kAppended = 1, kFull = 2 };

// built: the map describes the index as of (seen_moved, seen_appended); cap_ids: vec ids it has room for
inline MapRefresh fetch_map_decide(bool built, uint64_t seen_moved, uint64_t seen_appended, uint64_t moved, uint64_t appended) {
  if (!built || seen_moved != moved) return MapRefresh::kFull;
  if (seen_appended != appended) return MapRefresh::kAppended;
  return MapRefresh::kNone;
}

// One job of the pass: rows first .. end - 1 of storage tile `tile` (64 rows) lie below their list's length.
struct MapJob {
  uint32_t tile, first, end;  // 0 <= first < end <= 64
};

// Rows [from[c], len[c]) of every owned list c with storage at off[c] (a multiple of 64), tile by tile.  from == nullptr: from 0 (the full
// pass).  owner nullable = every list is this rank's.  Returns the rows covered.
inline uint64_t fetch_map_plan(const uint32_t* from, const uint32_t* len, const uint32_t* off, const uint8_t* owner, uint32_t rank, uint32_t k,
                               std::vector<MapJob>& out) {
  uint64_t rows = 0;
  for (uint32_t c = 0; c < k; ++c) {
    if (owner != nullptr && (uint32_t)owner[c] != rank) continue;
    const uint32_t lo = from != nullptr ? from[c] : 0u, hi = len[c];
    if (hi <= lo) continue;
    for (uint32_t t = lo / 64u; t <= (hi - 1u) / 64u; ++t) {
      const uint32_t a = t * 64u < lo ? lo - t * 64u : 0u;
      const uint32_t b = hi - t * 64u < 64u ? hi - t * 64u : 64u;
      out.push_back(MapJob{off[c] / 64u + t, a, b});
    }
    rows += hi - lo;
  }
  return rows;
}

}  // namespace vers
