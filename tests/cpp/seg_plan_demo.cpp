// Host check of the exhaustive scans' segment plan (vers_amd/csrc/seg_plan.hpp, built by the host compiler alone): reads lines of
// "n_rows b ld n_cu fixed_seg_rows" from standard input and prints the plan of each (tests/test_seg_plan_host.py compares them with its
// own restatement of the formula).
#include <cinttypes>
#include <cstdio>

#include "seg_plan.hpp"

int main() {
  unsigned long long n_rows;
  unsigned b, ld;
  int n_cu;
  long long fixed;
  while (std::scanf("%llu %u %u %d %lld", &n_rows, &b, &ld, &n_cu, &fixed) == 5) {
    const vers::SegPlan s = vers::seg_plan(n_rows, b, ld, n_cu, fixed);
    std::printf("%u %u %u %u %u %d %d\n", s.seg_rows, s.n_segs, s.n_segs_pad, s.n_items, s.n_qg, s.QG, (int)s.too_large);
  }
  return 0;
}
