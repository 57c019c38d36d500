// vers_amd/csrc/fetch_plan.hpp with the host compiler alone: the refresh decision of vers_ivf_fetch's vec id -> storage row map as a pure
// function of (the counters the map has seen, the handle's counters), and the tile jobs of the full pass and of the appended-range pass
// against a row-by-row restatement.
#include <cstdio>
#include <set>
#include <utility>

#include "fetch_plan.hpp"

using namespace vers;

static int bad = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); ++bad; } } while (0)

static std::set<uint64_t> rows_of(const std::vector<MapJob>& jobs) {
  std::set<uint64_t> s;
  for (const MapJob& j : jobs) {
    CHECK(j.first < j.end && j.end <= 64u);
    for (uint32_t r = j.first; r < j.end; ++r) CHECK(s.insert((uint64_t)j.tile * 64 + r).second);  // no row twice
  }
  return s;
}

int main() {
  // never built -> full, whatever the counters say
  CHECK(fetch_map_decide(false, 0, 0, 0, 0) == MapRefresh::kFull);
  CHECK(fetch_map_decide(false, 3, 4, 3, 4) == MapRefresh::kFull);
  // neither counter moved (an update_batch in which every row stayed bumps neither): valid as it is
  CHECK(fetch_map_decide(true, 3, 4, 3, 4) == MapRefresh::kNone);
  // only appends since: the appended range alone
  CHECK(fetch_map_decide(true, 3, 4, 3, 5) == MapRefresh::kAppended);
  CHECK(fetch_map_decide(true, 3, 4, 3, 9) == MapRefresh::kAppended);
  // anything moved -> full, appends or not
  CHECK(fetch_map_decide(true, 3, 4, 4, 4) == MapRefresh::kFull);
  CHECK(fetch_map_decide(true, 3, 4, 4, 7) == MapRefresh::kFull);

  // lists ending at 1, 63, 64, 65 rows, an empty one, one of two whole tiles + 2, one that belongs to another rank
  const uint32_t k = 7;
  const uint32_t off[k] = {0, 64, 192, 320, 448, 512, 704}, len[k] = {1, 63, 64, 65, 0, 130, 50};
  const uint8_t owner[k] = {0, 0, 0, 0, 0, 0, 1};
  std::vector<MapJob> full;
  const uint64_t n_full = fetch_map_plan(nullptr, len, off, owner, 0, k, full);
  CHECK(n_full == 1 + 63 + 64 + 65 + 130);
  std::set<uint64_t> want;
  for (uint32_t c = 0; c < 6; ++c)
    for (uint32_t r = 0; r < len[c]; ++r) want.insert((uint64_t)off[c] + r);
  CHECK(rows_of(full) == want);  // every row below its list's length, no slack row, nothing of the other rank's list
  CHECK(full.size() == 1 + 1 + 1 + 2 + 0 + 3);
  std::vector<MapJob> all;
  CHECK(fetch_map_plan(nullptr, len, off, nullptr, 0, k, all) == n_full + 50);  // owner == nullptr: every list is this rank's

  // appended: list 0 grew 1 -> 3, list 1 63 -> 70 (into its second tile), list 3 65 -> 65 (unchanged), list 5 130 -> 200 (over a tile boundary)
  const uint32_t now[k] = {3, 70, 64, 65, 0, 200, 50};
  std::vector<MapJob> tail;
  const uint64_t n_tail = fetch_map_plan(len, now, off, owner, 0, k, tail);
  CHECK(n_tail == 2 + 7 + 70);
  std::set<uint64_t> grown;
  for (uint32_t c = 0; c < 6; ++c)
    for (uint32_t r = len[c]; r < now[c]; ++r) grown.insert((uint64_t)off[c] + r);
  CHECK(rows_of(tail) == grown);
  // nothing grew: no job
  std::vector<MapJob> none;
  CHECK(fetch_map_plan(now, now, off, owner, 0, k, none) == 0 && none.empty());
  printf(bad ? "FAILED\n" : "all ok\n");
  return bad ? 1 : 0;
}
