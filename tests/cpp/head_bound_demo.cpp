// Host check of the int8 head's bound (vers_amd/csrc/prescan.hip.h: head_scale, head_quant, head_resid, head_extra, head_lower next to
// pre_bound / prune_tail_entry -- the functions' own text, cut out of the header by tests/test_head_bound_host.py into prune_snip.h).
// For (row, query, H, boundary) the bound from the int8 images must never exceed the val computed in f64 from the fp16 operands (+ the
// stored |x|^2) minus pre_bound's `common`; with the minima over a tile's rows it must stay below the smallest of their vals; and a NaN
// in any input must make the test say "not dead".
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

using vers::head_extra;
using vers::head_lower;
using vers::head_quant;
using vers::head_resid;
using vers::head_scale;
using vers::pre_bound;
using vers::prune_eps;
using vers::prune_tail_entry;

static float f16r(float v) { return (float)(_Float16)v; }

struct Family {
  const char* name;
  std::vector<std::vector<float>> rows, queries;
};

static std::vector<float> unit(std::mt19937& g, int d, const std::vector<float>* centre, float sigma, float scale) {
  std::normal_distribution<float> nd(0.0f, 1.0f);
  std::vector<float> v(d);
  double n2 = 0.0;
  for (int j = 0; j < d; ++j) { v[j] = (centre ? (*centre)[j] : 0.0f) + sigma * nd(g); n2 += (double)v[j] * v[j]; }
  const float inv = (float)(1.0 / std::sqrt(n2 > 0 ? n2 : 1.0));
  for (int j = 0; j < d; ++j) v[j] = v[j] * inv * scale;
  return v;
}

int main() {
  const int d = 768, n_rows = 64, n_q = 16;
  std::mt19937 g(0x5EED13);
  std::vector<Family> fams;
  auto clustered = [&](const char* name) {
    Family f; f.name = name;
    std::vector<std::vector<float>> centres;
    for (int m = 0; m < 8; ++m) centres.push_back(unit(g, d, nullptr, 1.0f, 1.0f));
    const float sigma = 0.5f / std::sqrt(d / 3.0f);
    for (int r = 0; r < n_rows; ++r) f.rows.push_back(unit(g, d, &centres[r % 8], sigma, 1.0f));
    for (int q = 0; q < n_q; ++q) f.queries.push_back(unit(g, d, &centres[(q + 3) % 8], sigma, 1.0f));
    return f;
  };
  fams.push_back(clustered("clustered, foreign modes"));
  {  // elements AT the clamp: many head elements equal to +- the maximum
    Family f = clustered("elements at the clamp");
    float mx = 0.0f;
    for (auto& r : f.rows) for (int j = 0; j < 512; ++j) mx = std::max(mx, std::fabs(r[j]));
    for (int r = 0; r < n_rows; ++r) for (int j = r % 5; j < 512; j += 5) f.rows[r][j] = (j & 1) ? mx : -mx;
    for (int q = 0; q < n_q; ++q) for (int j = q % 3; j < 512; j += 3) f.queries[q][j] = (j & 2) ? 0.11f : -0.11f;
    fams.push_back(f);
  }
  {  // an OUTLIER sets s_x 50x the typical element
    Family f = clustered("outlier x50");
    f.rows[7][13] = 50.0f / std::sqrt((float)d);
    fams.push_back(f);
  }
  {  // all-zero head columns (rows and, for half the queries, the query)
    Family f = clustered("all-zero head");
    for (auto& r : f.rows) for (int j = 0; j < 512; ++j) r[j] = 0.0f;
    for (int q = 0; q < n_q; q += 2) for (int j = 0; j < 512; ++j) f.queries[q][j] = 0.0f;
    fams.push_back(f);
  }
  {  // negative and positive I: queries equal to a row and to its negative
    Family f = clustered("queries = +- rows");
    for (int q = 0; q < n_q; ++q) { f.queries[q] = f.rows[q]; if (q & 1) for (float& v : f.queries[q]) v = -v; }
    fams.push_back(f);
  }
  Family aligned = clustered("residual aligned with the query");  // (its queries are built per H below: q'_P proportional to -delta of a row)
  fams.push_back(aligned);

  unsigned long long checks = 0, violations = 0, tile_checks = 0;
  double closest = 1e300;
  for (Family& f : fams) {
    const bool align = &f == &fams.back();
    for (int H = 256; H <= 512; H += 64) {
      // the handle's measurements over its stored rows
      std::vector<float> xn(n_rows);
      float xmax2 = 0.0f, R2 = 0.0f, hmax = 0.0f;
      for (int r = 0; r < n_rows; ++r) {
        float a = 0.0f, rr = 0.0f;
        for (int j = 0; j < d; ++j) { a = a + f.rows[r][j] * f.rows[r][j]; const float dl = f.rows[r][j] - f16r(f.rows[r][j]); rr = rr + dl * dl; }
        xn[r] = a; xmax2 = std::max(xmax2, a); R2 = std::max(R2, rr);
        for (int j = 0; j < H; ++j) hmax = std::max(hmax, std::fabs(f16r(f.rows[r][j])));
      }
      const float sx = head_scale(hmax);
      std::vector<std::vector<int32_t>> X(n_rows, std::vector<int32_t>(H));
      float Rh2 = 0.0f;
      for (int r = 0; r < n_rows; ++r) {
        double acc = 0.0;
        for (int j = 0; j < H; ++j) {
          const float v = f16r(f.rows[r][j]);
          X[r][j] = head_quant(v, sx);
          if (X[r][j] < -127 || X[r][j] > 127) { std::printf("VIOLATION quantiser out of range\n"); ++violations; }
          const double e = head_resid(v, sx, X[r][j]);
          acc += e * e;
        }
        Rh2 = std::max(Rh2, vers::prune_round_up(acc * (1.0 + 1e-12)));
      }
      if (align)  // query q: head = -(a large multiple of) the residual of row q, so that <delta, q'_P> = -|delta| |q'_P|
        for (int q = 0; q < n_q; ++q)
          for (int j = 0; j < H; ++j) f.queries[q][j] = (float)(0.5 * 40.0 * head_resid(f16r(f.rows[q][j]), sx, X[q][j]));
      const double om = 1.0 - prune_eps(d);
      for (int q = 0; q < n_q; ++q) {
        std::vector<float> qs(d);
        float qn = 0.0f, rq = 0.0f, qmax = 0.0f;
        for (int j = 0; j < d; ++j) {
          const float y = -2.0f * f.queries[q][j];
          qs[j] = f16r(y);
          qn = qn + f.queries[q][j] * f.queries[q][j];
          const float dl = y - qs[j]; rq = rq + dl * dl;
          if (j < H) qmax = std::max(qmax, std::fabs(qs[j]));
        }
        const float sn = head_scale(qmax);
        std::vector<int32_t> Q(H);
        double e2 = 0.0, p2 = 0.0;
        for (int j = 0; j < H; ++j) {
          Q[j] = head_quant(qs[j], sn);
          const double e = head_resid(qs[j], sn, Q[j]);
          e2 += e * e; p2 += (double)qs[j] * qs[j];
        }
        const float extra = head_extra(p2, e2, (double)xmax2, (double)R2, (double)Rh2);
        const double common = pre_bound((double)qn, (double)xmax2, (double)R2, (uint32_t)d, 0, 2, (double)rq).common;
        std::vector<double> val(n_rows);
        for (int r = 0; r < n_rows; ++r) {
          double a = 0.0;
          for (int j = 0; j < d; ++j) a += (double)f16r(f.rows[r][j]) * (double)qs[j];
          val[r] = a + (double)xn[r];
        }
        for (int c = 4; c <= H / 64; ++c) {
          float hS2 = 0.0f;
          for (int j = d - 1; j >= 64 * c; --j) { const float hh = -0.5f * qs[j]; hS2 = hS2 + hh * hh; }
          const float tail = prune_tail_entry((double)hS2, (double)qn, (double)xmax2, (double)R2, (double)rq, (uint32_t)d);
          const float bracket = vers::prune_round_up((double)tail + (double)extra);
          int32_t I_min = std::numeric_limits<int32_t>::max();
          uint32_t N_min = 0xFFFFFFFFu;
          double val_min = 1e300;
          for (int r = 0; r < n_rows; ++r) {
            int32_t I = 0; uint32_t N = 0;
            for (int j = 0; j < 64 * c; ++j) { I += X[r][j] * Q[j]; N += (uint32_t)(X[r][j] * X[r][j]); }
            const double lb = head_lower(I, N, sx, sn, (double)Rh2, om, bracket);
            ++checks;
            if (!(lb <= val[r] - common)) { if (++violations <= 5) std::printf("VIOLATION %s H %d q %d c %d r %d: bound %.9g > val - common %.9g\n", f.name, H, q, c, r, lb, val[r] - common); }
            if (std::isfinite(lb)) closest = std::min(closest, (val[r] - common - lb) / ((double)qn + (double)xmax2));
            I_min = std::min(I_min, I); N_min = std::min(N_min, N); val_min = std::min(val_min, val[r]);
          }
          const double lbt = head_lower(I_min, N_min, sx, sn, (double)Rh2, om, bracket);
          ++tile_checks;
          if (!(lbt <= val_min - common)) { ++violations; std::printf("VIOLATION %s H %d q %d c %d: tile bound %.9g > %.9g\n", f.name, H, q, c, lbt, val_min - common); }
        }
      }
    }
    std::printf("%s: ok so far (%llu checks, smallest (val - common - bound) / (|q|^2 + max|x|^2) = %.3g)\n", f.name, checks, closest);
  }
  // a NaN anywhere -> "not dead": the comparison the kernel makes, head_lower(...) > thr, must be false
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const float nanf = std::numeric_limits<float>::quiet_NaN(), inff = std::numeric_limits<float>::infinity();
  unsigned long long nan_checks = 0;
  auto not_dead = [&](double lb, double thr, const char* what) {
    ++nan_checks;
    if (lb > thr) { ++violations; std::printf("VIOLATION NaN case '%s' says dead\n", what); }
  };
  not_dead(head_lower(100000, 5000u, nanf, 0.01f, 1e-4, 0.999, 0.5f), -0.6, "s_x NaN");
  not_dead(head_lower(100000, 5000u, inff, 0.01f, 1e-4, 0.999, 0.5f), -0.6, "s_x inf");
  not_dead(head_lower(100000, 5000u, 0.01f, nanf, 1e-4, 0.999, 0.5f), -0.6, "s_n NaN");
  not_dead(head_lower(100000, 5000u, 0.01f, inff, 1e-4, 0.999, 0.5f), -0.6, "s_n inf");
  not_dead(head_lower(100000, 5000u, 0.01f, 0.01f, nan, 0.999, 0.5f), -0.6, "Rh2 NaN");
  not_dead(head_lower(100000, 5000u, 0.01f, 0.01f, 1e-4, nan, 0.5f), -0.6, "1 - eps NaN");
  not_dead(head_lower(100000, 5000u, 0.01f, 0.01f, 1e-4, 0.999, nanf), -0.6, "bracket NaN");
  not_dead(head_lower(100000, 5000u, 0.01f, 0.01f, 1e-4, 0.999, inff), -0.6, "bracket inf");
  not_dead(head_lower(100000, 5000u, 0.01f, 0.01f, 1e-4, 0.999, 0.5f), nan, "threshold NaN");
  // a NaN element: the quantiser gives 0 and the residual, hence Rh2 / head_extra / the bracket, is NaN
  if (head_quant(nanf, 0.01f) != 0 || head_quant(1.0f, nanf) != 0 || head_quant(1.0f, 0.0f) != 0 || head_quant(1.0f, inff) != 0) { ++violations; std::printf("VIOLATION quantiser of a NaN\n"); }
  if (head_resid(nanf, 0.01f, 0) == head_resid(nanf, 0.01f, 0)) { ++violations; std::printf("VIOLATION residual of a NaN is not NaN\n"); }
  not_dead(head_lower(100000, 5000u, 0.01f, 0.01f, 1e-4, 0.999, head_extra(1.0, nan, 1.0, 1e-8, 1e-4)), -0.6, "query residual NaN");
  not_dead(head_lower(100000, 5000u, 0.01f, 0.01f, 1e-4, 0.999, head_extra(1.0, 1e-6, 1.0, 1e-8, nan)), -0.6, "head residual NaN in the bracket");
  not_dead(head_lower(100000, 5000u, 0.01f, 0.01f, 1e-4, 0.999, head_extra(1.0, 1e-6, nan, 1e-8, 1e-4)), -0.6, "max |x|^2 NaN");
  // ... and the same arguments without a NaN do say dead (the cases above test something)
  if (!(head_lower(100000, 5000u, 0.01f, 0.01f, 1e-4, 0.999, 0.5f) > -0.6)) { ++violations; std::printf("VIOLATION the finite twin of the NaN cases is not dead\n"); }
  std::printf("CHECKS %llu TILES %llu NANS %llu VIOLATIONS %llu\n", checks, tile_checks, nan_checks, violations);
  return violations ? 1 : 0;
}
