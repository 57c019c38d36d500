// fetch_demo.cpp -- vers_amd/host/ivfflat.hpp's fetch and search_by_id from compiled code (tests/test_fetch_host_cpp_gpu.py): after a
// removal and an update the device returns the mirror's vectors and clusters bit for bit, ids in no list come back as zeros with status 2,
// a search by id is the search with the stored vector, and the refusals throw with nothing written.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "../../vers_amd/host/ivfflat.hpp"

int main() {
  constexpr size_t N = 40;
  std::vector<vers::Vector<N>> X(600);
  for (size_t i = 0; i < X.size(); ++i)
    for (size_t j = 0; j < N; ++j) X[i].v[j] = (float)((i * 7 + j * 13) % 31) * 0.25f + (float)(i % 5);
  std::vector<uint64_t> init = {3, 90, 200, 333, 480, 599};
  auto a = vers::IVFFlatIndex<N>::build_index(6, 1, 5, X, &init);
  a.remove_batch({11, 12, 599});
  std::vector<size_t> vids;
  std::vector<vers::Vector<N>> rows;
  for (size_t v = 2; v < 590; v += 3) { vids.push_back(v); rows.push_back(X[v + 7]); }
  a.update_batch(vids, rows);
  // every id, descending, id 5 twice
  std::vector<size_t> all;
  for (size_t v = 600; v-- > 0;) all.push_back(v);
  all.push_back(5);
  const auto f = a.fetch(all);
  if (f.found + f.in_no_list != all.size() || f.in_no_list != 3 || f.found != a.live_count() + 1) { std::puts("COUNTS"); return 1; }
  for (size_t i = 0; i < all.size(); ++i) {
    const size_t v = all[i];
    const bool gone = v == 11 || v == 12 || v == 599;
    if (f.status[i] != (gone ? 2 : 0)) { std::puts("STATUS"); return 1; }
    if (gone) {
      if (f.clusters[i] != (size_t)UINT64_MAX) { std::puts("NO CLUSTER"); return 1; }
      for (size_t j = 0; j < N; ++j) if (f.rows[i].v[j] != 0.0f) { std::puts("ZEROS"); return 1; }
    } else {
      if (f.clusters[i] != a.assignments[v]) { std::puts("CLUSTERS"); return 1; }
      if (std::memcmp(f.rows[i].v, a.values[v].v, N * sizeof(float)) != 0) { std::puts("ROWS"); return 1; }
    }
  }
  // a search by id is the search with the stored vector; without itself the id is not in the answer
  for (size_t v : {0ul, 7ul, 300ul, 598ul}) {
    if (a.search_by_id(v, 10) != a.search_approximate(a.values[v], 10)) { std::puts("BY ID"); return 1; }
    const auto r = a.search_by_id(v, 10, 3, true);
    for (const auto& p : r) if (p.first == v) { std::puts("SELF"); return 1; }
    const auto with = a.search_by_id(v, 11, 3);
    std::vector<std::pair<size_t, float>> want;
    for (const auto& p : with) if (p.first != v && want.size() < 10) want.push_back(p);
    if (r != want) { std::puts("EXCLUDE"); return 1; }
  }
  // refusals: an id beyond n, an id in no list, the flag in the reference's mode
  for (int what = 0; what < 3; ++what) {
    bool threw = false;
    try {
      if (what == 0) a.fetch({1, 650});
      else if (what == 1) a.search_by_id(11, 5);
      else a.search_by_id(1, 5, 0, true);
    } catch (const vers::Panic& p) { threw = p.status == VERS_ERR_INVALID; }
    if (!threw) { std::puts("INVALID"); return 1; }
  }
  std::puts("SAME");
  return 0;
}
