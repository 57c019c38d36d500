// The C++ host mirror's compact() (vers_amd/host/ivfflat.hpp) from compiled code: remove -> compact -> every search equals the one
// before the compaction, the fields are untouched, storage shrank, adds and a second compaction work afterwards.
// Driven by tests/test_compact_gpu.py.
#include <cstdio>
#include <vector>

#include "../../vers_amd/host/ivfflat.hpp"

int main() {
  constexpr size_t N = 40;
  std::vector<vers::Vector<N>> X(900), extra(30);
  for (size_t i = 0; i < X.size(); ++i)
    for (size_t j = 0; j < N; ++j) X[i].v[j] = (float)((i * 7 + j * 13) % 31) * 0.25f + (float)(i % 6);
  for (size_t i = 0; i < extra.size(); ++i)
    for (size_t j = 0; j < N; ++j) extra[i].v[j] = (float)((i * 11 + j * 3) % 17) * 0.5f;
  std::vector<uint64_t> init = {3, 90, 200, 333, 480, 899};
  auto a = vers::IVFFlatIndex<N>::build_index(6, 1, 5, X, &init);
  std::vector<size_t> gone;
  for (size_t v = 0; v < X.size(); ++v)
    if (v % 3 != 1) gone.push_back(v);
  if (a.remove_batch(gone) != gone.size()) { std::puts("COUNT"); return 1; }
  std::vector<std::vector<std::pair<size_t, float>>> before;
  for (size_t q = 0; q < 25; ++q) before.push_back(a.search_approximate(X[q * 31], 10));
  const auto ids = a.ids;
  const size_t live = a.live_count();
  const auto r = a.compact();
  if (!(r.second < r.first) || r.second % 64 != 0) { std::printf("ROWS %llu %llu\n", (unsigned long long)r.first, (unsigned long long)r.second); return 1; }
  if (a.ids != ids || a.live_count() != live || a.assignments.size() != X.size() || a.values.size() != X.size()) { std::puts("FIELDS"); return 1; }
  for (size_t q = 0; q < 25; ++q)
    if (a.search_approximate(X[q * 31], 10) != before[q]) { std::puts("SEARCH"); return 1; }
  a.add_batch(extra);
  if (a.live_count() != live + extra.size() || a.ids[a.assignments[900]].back() < 900) { std::puts("ADD"); return 1; }
  const auto r2 = a.compact(), r3 = a.compact();
  if (r3.first != r3.second || r3.first != r2.second) { std::puts("TWICE"); return 1; }
  for (size_t q = 0; q < 25; ++q)
    for (auto& p : a.search_approximate(X[q * 31], 10))
      if (p.first < 900 && p.first % 3 != 1) { std::puts("REMOVED ROW FOUND"); return 1; }
  std::puts("SAME");
  return 0;
}
