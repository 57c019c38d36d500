// Host check of the sub-cluster ball bound (vers_amd/csrc/prescan.hip.h: ball_bracket, ball_lower next to pre_bound / prune_lower -- the
// functions' own text, cut out of the header by tests/test_ball_bound_host.py into prune_snip.h).  For (row, query, sub-cluster) triples at
// d = 64, 300 and 768 -- random clustered rows, and adversarial rows on the side of the query that set r_j, each also taken as a
// sub-cluster of its own so that it sits at distance exactly r_j after its fp16 rounding, where Cauchy-Schwarz is attained -- the bound must never exceed the val computed in f64 from the fp16 operands (+ the stored
// |x|^2) minus pre_bound's `common` (the emulation of the kernel's val tests/cpp/head_bound_demo.cpp uses), whichever way the dot product
// of the centre is summed in f32; and a NaN or an infinity in any input must make the test say "not dead".
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>
#define __host__
#define __device__
#include "prune_snip.h"

using vers::ball_bracket;
using vers::ball_lower;
using vers::pre_bound;
using vers::prune_round_up;

static float f16r(float v) { return (float)(_Float16)v; }

static std::vector<float> unit(std::mt19937& g, int d, int ld, const std::vector<float>* centre, float sigma, float scale) {
  std::normal_distribution<float> nd(0.0f, 1.0f);
  std::vector<float> v(ld, 0.0f);
  double n2 = 0.0;
  for (int j = 0; j < d; ++j) { v[j] = (centre ? (*centre)[j] : 0.0f) + sigma * nd(g); n2 += (double)v[j] * v[j]; }
  const float inv = (float)(1.0 / std::sqrt(n2 > 0 ? n2 : 1.0));
  for (int j = 0; j < d; ++j) v[j] = v[j] * inv * scale;
  return v;
}
// <s, q'> as an f32 sum of the exact products: forward, backward and pairwise
static float dot_f32(const std::vector<float>& s, const std::vector<float>& q, int order) {
  const int n = (int)s.size();
  if (order == 0) { float a = 0.0f; for (int j = 0; j < n; ++j) a = a + s[j] * q[j]; return a; }
  if (order == 1) { float a = 0.0f; for (int j = n - 1; j >= 0; --j) a = a + s[j] * q[j]; return a; }
  std::vector<float> t(n);
  for (int j = 0; j < n; ++j) t[j] = s[j] * q[j];
  for (int w = n; w > 1; w = (w + 1) / 2)
    for (int j = 0; j < w / 2; ++j) t[j] = t[j] + t[w - 1 - j];
  return t[0];
}

int main() {
  std::mt19937 g(0x5EED21);
  unsigned long long checks = 0, violations = 0, adversarial = 0;
  double closest = 1e300, closest_adv = 1e300, worst_adv = -1e300;  // (worst_adv: the LARGEST slack of a row exactly at r_j)
  const int dims[3] = {64, 300, 768};
  for (int d : dims) {
    const int ld = (d + 63) / 64 * 64;
    const float sigma = 0.5f / std::sqrt(d / 3.0f);
    for (int rep = 0; rep < 6; ++rep) {
      const float scale = rep == 4 ? 30.0f : (rep == 5 ? 0.02f : 1.0f);  // (rows far from and near the origin as well)
      const std::vector<float> mode = unit(g, d, ld, nullptr, 1.0f, 1.0f);
      std::vector<std::vector<float>> queries;
      for (int q = 0; q < 12; ++q) queries.push_back(unit(g, d, ld, q < 4 ? &mode : nullptr, q < 4 ? sigma : 1.0f, q % 3 == 2 ? 2.5f : 1.0f));
      std::vector<std::vector<float>> qs;  // q' = fp16(-2 q)
      for (auto& q : queries) { std::vector<float> t(ld); for (int j = 0; j < ld; ++j) t[j] = f16r(-2.0f * q[j]); qs.push_back(t); }
      // the sub-cluster: random rows of the mode + per query one adversarial row towards the query, 5 % FARTHER from the centre than the
      // farthest random row: the adversarial rows set r_j
      std::vector<std::vector<float>> rows;
      for (int r = 0; r < 40; ++r) rows.push_back(unit(g, d, ld, &mode, sigma, scale));
      std::vector<float> s(ld, 0.0f);
      for (int j = 0; j < ld; ++j) { float a = 0.0f; for (auto& r : rows) a += f16r(r[j]); s[j] = f16r(a / (float)rows.size()); }
      const size_t n_random = rows.size();
      double far2 = 0.0;
      for (auto& r : rows) { double acc = 0.0; for (int j = 0; j < ld; ++j) { const double dl = (double)f16r(r[j]) - (double)s[j]; acc += dl * dl; } far2 = std::max(far2, acc); }
      const double rho = 1.05 * std::sqrt(far2);
      for (auto& q : qs) {
        double n2 = 0.0;
        for (int j = 0; j < ld; ++j) n2 += (double)q[j] * q[j];
        std::vector<float> x(ld, 0.0f);
        for (int j = 0; j < d; ++j) x[j] = (float)((double)s[j] - rho * (double)q[j] / std::sqrt(n2));
        rows.push_back(x);
      }
      // what the derive pass keeps: r over the shadow rows in f64, rounded up; the smallest stored |x|^2; |s| rounded up
      float r_j = 0.0f, m_j = std::numeric_limits<float>::infinity(), xmax2 = 0.0f, R2 = 0.0f;
      std::vector<float> xn(rows.size()), r_row(rows.size());
      for (size_t r = 0; r < rows.size(); ++r) {
        double acc = 0.0; float a = 0.0f, rr = 0.0f;
        for (int j = 0; j < ld; ++j) {
          const double dl = (double)f16r(rows[r][j]) - (double)s[j]; acc += dl * dl;
          a = a + rows[r][j] * rows[r][j];
          const float e = rows[r][j] - f16r(rows[r][j]); rr = rr + e * e;
        }
        r_row[r] = prune_round_up(std::sqrt(acc * (1.0 + 1e-12)) * (1.0 + 1e-12));
        r_j = std::max(r_j, r_row[r]);
        xn[r] = a; m_j = std::min(m_j, a); xmax2 = std::max(xmax2, a); R2 = std::max(R2, rr);
      }
      double s2 = 0.0;
      for (int j = 0; j < ld; ++j) s2 += (double)s[j] * s[j];
      const float sn_j = prune_round_up(std::sqrt(s2) * (1.0 + 1e-12));
      for (size_t q = 0; q < qs.size(); ++q) {
        float qn = 0.0f, rq = 0.0f; double p2 = 0.0;
        for (int j = 0; j < ld; ++j) {
          qn = qn + queries[q][j] * queries[q][j];
          const float dl = -2.0f * queries[q][j] - qs[q][j]; rq = rq + dl * dl;
          p2 += (double)qs[q][j] * qs[q][j];
        }
        const float nq = prune_round_up(std::sqrt(p2) * (1.0 + 1e-12));
        const float bracket = ball_bracket((double)qn, (double)xmax2, (double)R2, (double)rq, (uint32_t)ld);
        const double common = pre_bound((double)qn, (double)xmax2, (double)R2, (uint32_t)ld, 0, 2, (double)rq).common;
        for (int order = 0; order < 3; ++order) {
          const float D = dot_f32(s, qs[q], order);
          const double lb = ball_lower(m_j, D, r_j, sn_j, nq, bracket, (uint32_t)ld);
          {  // the query's adversarial row as a sub-cluster of its own around the same centre: the row is EXACTLY at r_j after its fp16
             // rounding and m_j is its own |x|^2 -- what is left between the bound and the val are the rounding terms alone
            const size_t r = n_random + q;
            double a = 0.0;
            for (int j = 0; j < ld; ++j) a += (double)f16r(rows[r][j]) * (double)qs[q][j];
            const double val = a + (double)xn[r];
            const double lb1 = ball_lower(xn[r], D, r_row[r], sn_j, nq, bracket, (uint32_t)ld);
            ++checks; ++adversarial;
            if (!(lb1 <= val - common)) { if (++violations <= 5) std::printf("VIOLATION d %d rep %d q %zu order %d: bound of the row at r_j %.9g > val - common %.9g\n", d, rep, q, order, lb1, val - common); }
            const double slack = (val - common - lb1) / ((double)qn + (double)xmax2);
            closest = std::min(closest, slack);
            closest_adv = std::min(closest_adv, slack);
            worst_adv = std::max(worst_adv, slack);
          }
          for (size_t r = 0; r < rows.size(); ++r) {
            double a = 0.0;
            for (int j = 0; j < ld; ++j) a += (double)f16r(rows[r][j]) * (double)qs[q][j];
            const double val = a + (double)xn[r];
            const bool adv = r == n_random + q;
            ++checks; adversarial += adv ? 1 : 0;
            if (!(lb <= val - common)) { if (++violations <= 5) std::printf("VIOLATION d %d rep %d q %zu r %zu order %d: bound %.9g > val - common %.9g\n", d, rep, q, r, order, lb, val - common); }
            const double slack = (val - common - lb) / ((double)qn + (double)xmax2);
            closest = std::min(closest, slack);
            if (adv) closest_adv = std::min(closest_adv, slack);
          }
        }
      }
    }
    std::printf("d %d: ok so far (%llu checks, %llu adversarial; smallest (val - common - bound) / (|q|^2 + max|x|^2) = %.3g, adversarial rows %.3g)\n", d, checks, adversarial, closest, closest_adv);
  }
  // a NaN or an infinity anywhere -> "not dead": the comparison the kernel makes, ball_lower(...) > thr, must be false
  const float nanf = std::numeric_limits<float>::quiet_NaN(), inff = std::numeric_limits<float>::infinity();
  unsigned long long nan_checks = 0;
  auto not_dead = [&](double lb, double thr, const char* what) {
    ++nan_checks;
    if (lb > thr) { ++violations; std::printf("VIOLATION case '%s' says dead\n", what); }
  };
  not_dead(ball_lower(nanf, -0.2f, 0.4f, 1.0f, 2.0f, 1e-3f, 768u), -0.6, "m NaN (an open sub-cluster)");
  not_dead(ball_lower(1.0f, nanf, 0.4f, 1.0f, 2.0f, 1e-3f, 768u), -0.6, "D NaN");
  not_dead(ball_lower(1.0f, inff, 0.4f, 1.0f, 2.0f, 1e-3f, 768u), -0.6, "D +inf");
  not_dead(ball_lower(1.0f, -inff, 0.4f, 1.0f, 2.0f, 1e-3f, 768u), -0.6, "D -inf");
  not_dead(ball_lower(1.0f, -0.2f, nanf, 1.0f, 2.0f, 1e-3f, 768u), -0.6, "r NaN");
  not_dead(ball_lower(1.0f, -0.2f, inff, 1.0f, 2.0f, 1e-3f, 768u), -0.6, "r inf");
  not_dead(ball_lower(1.0f, -0.2f, 0.4f, nanf, 2.0f, 1e-3f, 768u), -0.6, "sn NaN");
  not_dead(ball_lower(1.0f, -0.2f, 0.4f, inff, 2.0f, 1e-3f, 768u), -0.6, "sn inf");
  not_dead(ball_lower(1.0f, -0.2f, 0.4f, 1.0f, nanf, 1e-3f, 768u), -0.6, "nq' NaN");
  not_dead(ball_lower(1.0f, -0.2f, 0.4f, 1.0f, inff, 1e-3f, 768u), -0.6, "nq' inf");
  not_dead(ball_lower(1.0f, -0.2f, 0.4f, 1.0f, 2.0f, nanf, 768u), -0.6, "bracket NaN");
  not_dead(ball_lower(1.0f, -0.2f, 0.4f, 1.0f, 2.0f, inff, 768u), -0.6, "bracket inf");
  not_dead(ball_lower(1.0f, -0.2f, 0.4f, 1.0f, 2.0f, ball_bracket(nanf, 1.0, 1e-8, 1e-8, 768u), 768u), -0.6, "|q|^2 NaN");
  not_dead(ball_lower(1.0f, -0.2f, 0.4f, 1.0f, 2.0f, ball_bracket(1.0, 1.0, 1e-8, nanf, 768u), 768u), -0.6, "query residual NaN");
  not_dead(ball_lower(1.0f, -0.2f, 0.4f, 1.0f, 2.0f, 1e-3f, 768u), (double)nanf, "threshold NaN");
  not_dead(ball_lower(1.0f, -0.2f, 0.4f, 1.0f, 2.0f, 1e-3f, 768u), (double)inff, "threshold +inf (none yet)");
  // ... and the same arguments without a NaN do say dead (the cases above test something)
  if (!(ball_lower(1.0f, -0.2f, 0.4f, 1.0f, 2.0f, 1e-3f, 768u) > -0.6)) { ++violations; std::printf("VIOLATION the finite twin of the NaN cases is not dead\n"); }
  std::printf("CHECKS %llu ADVERSARIAL %llu NANS %llu VIOLATIONS %llu SLACK %.3g ADVMIN %.3g ADVMAX %.3g\n", checks, adversarial, nan_checks, violations, closest, closest_adv, worst_adv);
  return violations ? 1 : 0;
}
