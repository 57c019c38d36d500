// update_demo.cpp -- vers_amd/host/ivfflat.hpp's update_batch from compiled code (tests/test_update_cpp_gpu.py): stays, moves, an id
// that is in no list, the refusals, and the specification -- the updated index equals the one load_index makes of its saved file.
#include <algorithm>
#include <cstdio>

#include "../../vers_amd/host/ivfflat.hpp"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  constexpr size_t N = 40;
  std::vector<vers::Vector<N>> X(600);
  for (size_t i = 0; i < X.size(); ++i)
    for (size_t j = 0; j < N; ++j) X[i].v[j] = (float)((i * 7 + j * 13) % 31) * 0.25f + (float)(i % 5);
  std::vector<uint64_t> init = {3, 90, 200, 333, 480, 599};
  auto a = vers::IVFFlatIndex<N>::build_index(6, 1, 5, X, &init);
  a.remove_batch({11, 12});
  // every third row takes the value of the row 7 further on: some stay in their list, some move; 11 is in no list
  std::vector<size_t> vids;
  std::vector<vers::Vector<N>> rows;
  for (size_t v = 2; v < 590; v += 3) { vids.push_back(v); rows.push_back(X[v + 7]); }
  const size_t live = a.live_count();
  const auto st = a.update_batch(vids, rows);
  size_t stayed = 0, moved = 0, skipped = 0;
  for (uint8_t s : st) (s == 0 ? stayed : s == 1 ? moved : skipped) += 1;
  if (skipped != 1 || stayed + moved + skipped != vids.size()) { std::puts("STATUS"); return 1; }
  if (a.live_count() != live || a.assignments.size() != 600 || a.values.size() != 600) { std::puts("FIELDS"); return 1; }
  size_t listed = 0;
  for (size_t c = 0; c < a.ids.size(); ++c) {
    if (!std::is_sorted(a.ids[c].begin(), a.ids[c].end())) { std::puts("NOT ASCENDING"); return 1; }
    for (size_t x : a.ids[c]) if (a.assignments[x] != c) { std::puts("ASSIGNMENTS"); return 1; }
    listed += a.ids[c].size();
  }
  if (listed != live) { std::puts("LISTED"); return 1; }
  std::printf("stayed %zu moved %zu skipped %zu\n", stayed, moved, skipped);
  // all or nothing
  const auto ids_before = a.ids;
  for (int what = 0; what < 2; ++what) {
    bool threw = false;
    try {
      if (what == 0) a.update_batch({1, 650}, {X[0], X[1]});
      else a.update_batch({5, 9, 5}, {X[0], X[1], X[2]});
    } catch (const vers::Panic& p) { threw = p.status == VERS_ERR_INVALID; }
    if (!threw || a.ids != ids_before) { std::puts("INVALID"); return 1; }
  }
  // the specification: the saved file, loaded, is the same index
  a.save_index(argv[1]);
  auto b = vers::IVFFlatIndex<N>::load_index(argv[1]);
  if (b.live_count() != a.live_count() || b.ids != a.ids || b.assignments != a.assignments) { std::puts("LOAD"); return 1; }
  for (size_t q = 0; q < 30; ++q) {
    auto ra = a.search_approximate(X[q * 19], 10), rb = b.search_approximate(X[q * 19], 10);
    if (ra != rb) { std::puts("SEARCH"); return 1; }
  }
  std::puts("SAME");
  return 0;
}
