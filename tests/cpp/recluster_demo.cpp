// recluster_demo.cpp -- vers_amd/host/ivfflat.hpp's recluster from compiled code (tests/test_recluster_cpp_gpu.py): removed ids stay in no
// list and keep their numbers, k changes, the refusals change nothing, and the specification -- the reclustered index equals the one
// load_index makes of its saved file (an upload of the new fields followed by the removal of the ids that are in no list).
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
  std::vector<size_t> gone = {0, 11, 12, 599};
  for (size_t v = 5; v < 600; v += 9) gone.push_back(v);
  a.remove_batch(gone);
  a.add(X[17], 0);  // id 600
  const size_t live = a.live_count(), n = a.assignments.size();
  const auto values_before = a.values.size();
  // the refusals: an init position == m, zero clusters -- nothing changes
  const auto ids_before = a.ids;
  for (int what = 0; what < 2; ++what) {
    bool threw = false;
    std::vector<uint64_t> bad = {0, live};
    try {
      if (what == 0) a.recluster(2, 1, 3, &bad);
      else a.recluster(0, 1, 3, nullptr);
    } catch (const vers::Panic& p) { threw = p.status == (what == 0 ? VERS_ERR_INVALID : VERS_ERR_EMPTY); }
    if (!threw || a.ids != ids_before || a.num_centroids != 6) { std::puts("REFUSAL"); return 1; }
  }
  // 9 clusters from 6; two attempts; the draws are positions among the live rows
  std::vector<uint64_t> draws;
  for (size_t i = 0; i < 18; ++i) draws.push_back((i * 53 + 7) % live);
  const auto res = a.recluster(9, 2, 4, &draws);
  if (!res.second || !(res.first < 1e30f)) { std::puts("KEPT"); return 1; }
  if (a.num_centroids != 9 || a.centroids.size() != 9 || a.ids.size() != 9) { std::puts("K"); return 1; }
  if (a.live_count() != live || a.assignments.size() != n || a.values.size() != values_before) { std::puts("FIELDS"); return 1; }
  size_t listed = 0;
  for (size_t c = 0; c < a.ids.size(); ++c) {
    if (!std::is_sorted(a.ids[c].begin(), a.ids[c].end())) { std::puts("NOT ASCENDING"); return 1; }
    for (size_t x : a.ids[c]) if (a.assignments[x] != c) { std::puts("ASSIGNMENTS"); return 1; }
    listed += a.ids[c].size();
  }
  if (listed != live) { std::puts("LISTED"); return 1; }
  for (size_t v : gone)
    if (a.assignments[v] != 0) { std::puts("DEAD IDS"); return 1; }
  for (size_t c = 0; c < a.ids.size(); ++c)
    for (size_t v : gone)
      if (std::binary_search(a.ids[c].begin(), a.ids[c].end(), v)) { std::puts("REVIVED"); return 1; }
  a.add(X[23], 0);  // the next id is n, whatever was removed
  if (a.assignments.size() != n + 1 || a.ids[a.assignments[n]].back() != n) { std::puts("NEXT ID"); return 1; }
  std::printf("cost %g live %zu\n", (double)res.first, live);
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
