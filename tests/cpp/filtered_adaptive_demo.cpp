// The C++ host mirror's search_filtered_adaptive() (vers_amd/host/ivfflat.hpp) from compiled code: builds a small index from a closed-form
// corpus and prints, for a few queries, "query D depth" and every result as "query R id distance-bits".  tests/test_filtered_adaptive_gpu.py
// builds the same index through the Python mirror and compares the lines with its own results.  Filter of query q: vec id v is allowed when
// v % (13 + 7 q) == 0, over the first 900 - 37 q ids; top_k 12, nprobe_min 1, nprobe_max 5, min_allowed 6 + 3 q.
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
  for (size_t q = 0; q < 6; ++q) {
    std::vector<bool> allowed(900 - 37 * q, false);
    for (size_t v = 0; v < allowed.size(); v += 13 + 7 * q) allowed[v] = true;
    size_t depth = 0;
    const auto r = a.search_filtered_adaptive(X[q * 31], 12, 1, 5, 6 + 3 * q, allowed, &depth);
    std::printf("%zu D %zu\n", q, depth);
    for (auto& p : r) {
      uint32_t bits;
      std::memcpy(&bits, &p.second, 4);
      std::printf("%zu R %zu %u\n", q, p.first, bits);
    }
  }
  std::puts("DONE");
  return 0;
}
