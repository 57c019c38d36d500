// Host check of the list scan's early-abandon bound (vers_amd/csrc/prescan.hip.h: pre_bound, prune_tail_entry, prune_lower -- the
// functions' own text, cut out of the header by tests/test_prune_bound_host.py into prune_snip.h).  For (row, query, c) triples the
// bound after c 64-column steps must never exceed the f32 value the kernel's arithmetic produces for the whole row: fp16-rounded
// operands, exact products, f32 accumulation -- here in shuffled orders, prefix first as the step loop runs it --, + the stored |x|^2.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#define __host__
#define __device__
#include "prune_snip.h"

using vers::pre_bound;
using vers::prune_eps;
using vers::prune_lower;
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
  const int d = 768, n_steps = d / 64, n_rows = 96, n_q = 16;
  std::mt19937 g(0x5EED07);
  std::vector<Family> fams;
  auto clustered = [&](const char* name, float scale) {
    Family f; f.name = name;
    std::vector<std::vector<float>> centres;
    for (int m = 0; m < 8; ++m) centres.push_back(unit(g, d, nullptr, 1.0f, 1.0f));
    const float sigma = 0.5f / std::sqrt(d / 3.0f);
    for (int r = 0; r < n_rows; ++r) f.rows.push_back(unit(g, d, &centres[r % 8], sigma, scale));
    for (int q = 0; q < n_q; ++q) f.queries.push_back(unit(g, d, &centres[q % 8], sigma, scale));
    return f;
  };
  fams.push_back(clustered("clustered", 1.0f));
  fams.push_back(clustered("scaled x300", 300.0f));
  fams.push_back(clustered("subnormal in fp16 (x3e-7)", 3e-7f));
  {  // rows EQUAL to a query: val ~ -|q|^2, the bound's worst case (the suffix term is tight)
    Family f = clustered("rows equal to the query", 1.0f);
    for (int r = 0; r < n_rows; ++r) f.rows[r] = f.queries[r % n_q];
    fams.push_back(f);
  }
  {  // the whole distance in the PREFIX: row = query except in the first 64 columns
    Family f = clustered("distance in the prefix", 1.0f);
    for (int r = 0; r < n_rows; ++r) { f.rows[r] = f.queries[r % n_q]; for (int j = 0; j < 64; ++j) f.rows[r][j] += 0.05f * (float)((r + j) % 7 - 3); }
    fams.push_back(f);
  }
  {  // the whole distance in the SUFFIX: row = query except in the last 64 columns
    Family f = clustered("distance in the suffix", 1.0f);
    for (int r = 0; r < n_rows; ++r) { f.rows[r] = f.queries[r % n_q]; for (int j = d - 64; j < d; ++j) f.rows[r][j] += 0.05f * (float)((r + j) % 7 - 3); }
    fams.push_back(f);
  }
  unsigned long long triples = 0, violations = 0;
  double closest = 1e300;
  std::vector<int> perm(d);
  for (const Family& f : fams) {
    // what the handle measures over its stored rows: max |x|^2 (ordered f32 sum) and max sum (x - fp16(x))^2
    std::vector<float> xn(n_rows);
    float xmax2 = 0.0f, R2 = 0.0f;
    for (int r = 0; r < n_rows; ++r) {
      float a = 0.0f, rr = 0.0f;
      for (int j = 0; j < d; ++j) { a = a + f.rows[r][j] * f.rows[r][j]; const float dl = f.rows[r][j] - f16r(f.rows[r][j]); rr = rr + dl * dl; }
      xn[r] = a; xmax2 = std::max(xmax2, a); R2 = std::max(R2, rr);
    }
    const float om = (float)(1.0 - prune_eps(d));
    for (int q = 0; q < n_q; ++q) {
      std::vector<float> qs(d), h(d);
      float qn = 0.0f, rq = 0.0f;
      for (int j = 0; j < d; ++j) {
        const float y = -2.0f * f.queries[q][j];
        qs[j] = f16r(y); h[j] = -0.5f * qs[j];
        qn = qn + f.queries[q][j] * f.queries[q][j];
        const float dl = y - qs[j]; rq = rq + dl * dl;
      }
      for (int c = 1; c < n_steps; ++c) {
        float hS2 = 0.0f;
        for (int j = d - 1; j >= 64 * c; --j) hS2 = hS2 + h[j] * h[j];
        const float tail = prune_tail_entry((double)hS2, (double)qn, (double)xmax2, (double)R2, (double)rq, (uint32_t)d);
        for (int r = 0; r < n_rows; ++r) {
          for (int j = 0; j < d; ++j) perm[j] = j;
          std::shuffle(perm.begin(), perm.begin() + 64 * c, g);
          std::shuffle(perm.begin() + 64 * c, perm.end(), g);
          float acc = 0.0f, mp = 0.0f;
          for (int i = 0; i < 64 * c; ++i) { const float xs = f16r(f.rows[r][perm[i]]); acc = acc + xs * qs[perm[i]]; mp = mp + xs * xs; }
          const float acc_p = acc;
          for (int i = 64 * c; i < d; ++i) acc = acc + f16r(f.rows[r][perm[i]]) * qs[perm[i]];
          const float val = acc + xn[r];
          const float lb = prune_lower(acc_p, mp, om, tail);
          ++triples;
          if (lb > val) { if (++violations <= 5) std::printf("VIOLATION %s q %d c %d r %d: bound %.9g > val %.9g\n", f.name, q, c, r, lb, val); }
          if (std::isfinite(lb) && std::isfinite(val)) closest = std::min(closest, ((double)val - (double)lb) / ((double)qn + (double)xmax2));
        }
      }
    }
    std::printf("%s: ok so far (%llu triples, smallest (val - bound) / (|q|^2 + max|x|^2) = %.3g)\n", f.name, triples, closest);
  }
  std::printf("TRIPLES %llu VIOLATIONS %llu\n", triples, violations);
  return violations ? 1 : 0;
}
