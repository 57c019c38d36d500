// The C++ host mirror's range_search_filtered() / range_search_exhaustive_filtered() (vers_amd/host/ivfflat.hpp) from compiled code: builds a
// small index from a closed-form corpus and prints every result of a few filtered range searches as "query mode id distance-bits" lines
// (mode 0: probed, nprobe 3; mode 1: exhaustive; modes 2 / 3: the same in walk order).  tests/test_filtered_range_gpu.py builds the same
// index through the Python mirror and compares the lines with its own results.  Filter of query q: vec id v is allowed when
// v % (q + 2) == 0, over the first 900 - 37 q ids.  Radius of query q: 150 + 100 q for even q, +inf for odd q.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../vers_amd/host/ivfflat.hpp"

int main() {
  constexpr size_t N = 40;
  std::vector<vers::Vector<N>> X(900);
  for (size_t i = 0; i < X.size(); ++i)
    for (size_t j = 0; j < N; ++j) X[i].v[j] = (float)((i * 7 + j * 13) % 31) * 0.25f + (float)(i % 6);
  std::vector<uint64_t> init = {3, 90, 200, 333, 480, 899};
  auto a = vers::IVFFlatIndex<N>::build_index(6, 1, 5, X, &init);
  for (size_t q = 0; q < 6; ++q) {
    std::vector<bool> allowed(900 - 37 * q, false);
    for (size_t v = 0; v < allowed.size(); v += q + 2) allowed[v] = true;
    const float radius = q % 2 ? std::numeric_limits<float>::infinity() : 150.0f + 100.0f * (float)q;
    for (int mode = 0; mode < 4; ++mode) {
      const bool walk = mode >= 2;
      const auto r = mode % 2 == 0 ? a.range_search_filtered(X[q * 31], radius, 3, allowed, walk)
                                   : a.range_search_exhaustive_filtered(X[q * 31], radius, allowed, VERS_METRIC_L2SQ, walk);
      for (auto& p : r) {
        uint32_t bits;
        std::memcpy(&bits, &p.second, 4);
        std::printf("%zu %d %zu %u\n", q, mode, p.first, bits);
      }
    }
  }
  std::puts("DONE");
  return 0;
}
