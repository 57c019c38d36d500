// Host check of the adaptive filtered search's depth rule (vers_amd/csrc/adaptive_depth.hpp, built by the host compiler alone).  Reads cases
// from standard input, each "k nprobe_min nprobe_max min_allowed" followed by k allowed-row counts in ranking order, walks the ranks the way
// the plan kernel does -- the allowed rows before a rank carried along, a rank counted while the rule visits it -- and prints the depth of
// each case (tests/test_adaptive_depth_host.py compares them with a brute-force restatement of the definition).
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "adaptive_depth.hpp"

int main() {
  unsigned k, nprobe_min, nprobe_max, min_allowed;
  while (std::scanf("%u %u %u %u", &k, &nprobe_min, &nprobe_max, &min_allowed) == 4) {
    std::vector<uint32_t> a(k);
    for (unsigned j = 0; j < k; ++j)
      if (std::scanf("%" SCNu32, &a[j]) != 1) return 2;
    const uint32_t p_min = nprobe_min < k ? nprobe_min : k, p_max = nprobe_max < k ? nprobe_max : k;
    uint32_t before = 0, depth = 0;
    bool prefix = true;  // the visited ranks must be a prefix: no rank is visited behind one that was not
    for (uint32_t j = 0; j < p_max; ++j) {
      const bool v = vers::adaptive_rank_visited(j, before, p_min, p_max, min_allowed);
      if (v && depth != j) prefix = false;
      depth += v ? 1u : 0u;
      before += a[j];
    }
    if (vers::adaptive_rank_visited(p_max, before, p_min, p_max, min_allowed)) prefix = false;  // (nothing at or beyond P_max)
    std::printf("%u %d\n", depth, (int)prefix);
  }
  return 0;
}
