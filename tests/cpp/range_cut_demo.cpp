// Host check of the range pre-filter's cut (vers_amd/csrc/range_prescan.hip.h: range_cut, on pre_bound of prescan.hip.h -- the functions'
// own text, cut out of the headers by tests/test_range_cut_host.py into range_cut_snip.h).  Whenever `val > cut` holds in f32, the f64
// lower bound of the reference's distance that pre_bound gives for val must exceed the radius; with a non-finite input no val passes.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#define __host__
#define __device__
#include "range_cut_snip.h"

using vers::pre_bound;
using vers::PreBound;
using vers::range_cut;

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const uint32_t dpads[] = {64, 320, 768};
  const double radii[] = {0.0, 1e-6, 1e-3, 0.1, 0.5, 1.0, 2.0, 3.0, 4.0}, R2s[] = {0.0, 1e-7, (double)inf}, qns[] = {0.25, 1.0, 9.0}, xmaxs[] = {1.0, 90000.0};
  unsigned long long pairs = 0, ruled_out = 0, violations = 0, nonfinite_passed = 0;
  for (uint32_t d_pad : dpads)
    for (int metric = 0; metric < 2; ++metric)
      for (double r : radii)
        for (double R2 : R2s)
          for (double qn : qns)
            for (double xmax2 : xmaxs) {
              const float cut = range_cut(qn, xmax2, R2, (float)r, d_pad, metric);
              const bool finite_in = std::isfinite(R2);
              const PreBound pb = pre_bound(qn, xmax2, R2, d_pad, metric, 1);
              // vals round the cut: every f32 within 64 ulps, then steps of growing size either way, the extremes
              float grid[2 * 64 + 1 + 2 * 40 + 4];
              int n = 0;
              float up = cut, dn = cut;
              grid[n++] = cut;
              for (int k = 0; k < 64; ++k) { up = std::nextafterf(up, inf); dn = std::nextafterf(dn, -inf); grid[n++] = up; grid[n++] = dn; }
              for (int k = 0; k < 40; ++k) { const float step = std::ldexp(1.0f, k - 30); grid[n++] = cut + step; grid[n++] = cut - step; }
              grid[n++] = std::numeric_limits<float>::max(); grid[n++] = -std::numeric_limits<float>::max(); grid[n++] = inf; grid[n++] = nan;
              for (int i = 0; i < n; ++i) {
                const float val = grid[i];
                ++pairs;
                if (!(val > cut)) continue;
                if (!finite_in) { ++nonfinite_passed; continue; }
                if (val == inf) continue;  // (no finite row and query give it: pre_bound's model is of finite vals)
                ++ruled_out;
                const double lower = metric ? (double)val + 1.0 - pb.global : (double)val + pb.offset - pb.of((double)val);
                if (!(lower > (double)(float)r)) {
                  if (++violations <= 10) std::printf("VIOLATION d_pad %u metric %d r %g R2 %g qn %g xmax2 %g cut %.9g val %.9g lower %.17g\n", d_pad, metric, r, R2, qn, xmax2, cut, val, lower);
                }
              }
            }
  // the other non-finite inputs: |q|^2, max |x|^2, the radius
  const double bad[][4] = {{(double)nan, 1.0, 0.0, 1.0}, {(double)inf, 1.0, 0.0, 1.0}, {1.0, (double)inf, 0.0, 1.0}, {1.0, (double)nan, 0.0, 1.0},
                           {1.0, 1.0, (double)nan, 1.0}, {1.0, 1.0, 0.0, (double)inf}, {1.0, 1.0, 0.0, (double)-inf}, {1.0, 1.0, 0.0, (double)nan}};
  for (const auto& c : bad)
    for (int metric = 0; metric < 2; ++metric) {
      const float cut = range_cut(c[0], c[1], c[2], (float)c[3], 320, metric);
      const float vals[] = {-inf, -1e30f, -1.0f, 0.0f, 1.0f, 1e30f, std::numeric_limits<float>::max(), inf, nan};
      for (float val : vals) { ++pairs; if (val > cut) ++nonfinite_passed; }
    }
  std::printf("PAIRS %llu RULED_OUT %llu VIOLATIONS %llu NONFINITE_PASSED %llu\n", pairs, ruled_out, violations, nonfinite_passed);
  return violations == 0 && nonfinite_passed == 0 ? 0 : 1;
}
