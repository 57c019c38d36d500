// The C++ host mirror's range_search_exhaustive() (vers_amd/host/ivfflat.hpp) from compiled code: builds a small index from a closed-form
// corpus and prints every result of a few exhaustive range searches, both orders, as "query order id distance-bits" lines.
// tests/test_range_exhaustive_gpu.py builds the same index through the Python mirror and compares the lines with its own results.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../vers_amd/host/ivfflat.hpp"

int main() {
  constexpr size_t N = 40;
  std::vector<vers::Vector<N>> X(900);
  for (size_t i = 0; i < X.size(); ++i)
    for (size_t j = 0; j < N; ++j) X[i].v[j] = (float)((i * 7 + j * 13) % 31) * 0.25f + (float)(i % 6);
  std::vector<uint64_t> init = {3, 90, 200, 333, 480, 899};
  auto a = vers::IVFFlatIndex<N>::build_index(6, 1, 5, X, &init);
  const float radii[3] = {0.0f, 150.0f, 400.0f};
  for (size_t q = 0; q < 6; ++q)
    for (int walk = 0; walk < 2; ++walk) {
      const auto r = a.range_search_exhaustive(X[q * 31], radii[q % 3], VERS_METRIC_L2SQ, walk != 0);
      for (auto& p : r) {
        uint32_t bits;
        std::memcpy(&bits, &p.second, 4);
        std::printf("%zu %d %zu %u\n", q, walk, p.first, bits);
      }
    }
  std::puts("DONE");
  return 0;
}
