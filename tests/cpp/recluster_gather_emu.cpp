// Host emulation of tiles_to_live_rows_kernel (vers_amd/csrc/ivf_build.hip): the kernel's own text -- cut out of the source between its two
// marker comments by tests/test_recluster_kernel_host.py into kernel_snip.h -- runs as 256 std::threads per block with the barriers as
// std::barrier, on buffers sized exactly (an AddressSanitizer build sees any access outside them), and X' is compared bit for bit with a
// plain restatement: live row r of list c, holding vec id v, is row rank[v] of X'; columns >= d are zeros; nothing else is written.
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define __global__
#define __launch_bounds__(x)
struct Idx { uint32_t x; };
static thread_local Idx threadIdx, blockIdx;
static f32x4* g_lds;
static std::barrier<>* g_block_bar;
static void lds_barrier() { g_block_bar->arrive_and_wait(); }
constexpr uint32_t kGatherCols4 = 64;
namespace vers {
#include "kernel_snip.h"
}

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// lists (offset in rows, capacity, length): lengths 1, 63, 64, 65 (a second tile of one row), 0 (never visited) and 130 (two whole tiles + 2)
struct List { uint32_t off, cap, len; };

int run(uint32_t ld, uint32_t d, uint32_t pitch) {
  const std::vector<List> lists = {{0, 64, 1}, {64, 128, 63}, {192, 128, 64}, {320, 128, 65}, {448, 64, 0}, {512, 192, 130}};
  const uint32_t cap_rows = 704;
  std::vector<vers::GatherJob> tiles;  // one job per occupied tile, as the host makes them: the tile, its rows below the list's length
  for (uint32_t c = 0; c < lists.size(); ++c)
    for (uint32_t t = 0; t < (lists[c].len + 63) / 64; ++t) tiles.push_back({lists[c].off / 64 + t, std::min(64u, lists[c].len - t * 64)});
  std::mt19937 rng(ld * 31 + d);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::vector<float> src((size_t)cap_rows * ld);
  for (auto& v : src) v = nd(rng);
  auto at = [&](uint32_t row, uint32_t c) -> float& { return src[(size_t)(row / 64) * 64 * ld + ((size_t)(c / 4) * 64 + row % 64) * 4 + c % 4]; };
  // vec ids: the live rows take the ids 1 .. n_total - 2 that are not multiples of 5, shuffled over the rows -- id 0, the last id and every fifth
  // id are holes of the rank table; slack rows hold NaN / 1e30 in every column and a row_ids entry that LOOKS live (an id of a live row elsewhere,
  // or 0xFFFFFFFF): a kernel that trusted it would overwrite that row of X'
  uint32_t m = 0;
  for (auto& l : lists) m += l.len;
  std::vector<uint32_t> pool;
  for (uint32_t v = 1; pool.size() < m; ++v)
    if (v % 5) pool.push_back(v);
  const uint64_t n_total = (uint64_t)pool.back() + 2;  // the last id (n_total - 1) is a hole
  std::shuffle(pool.begin(), pool.end(), rng);
  std::vector<uint32_t> row_ids(cap_rows, 0xFFFFFFFFu);
  std::vector<uint64_t> rank(n_total + 1, 0);
  std::vector<uint8_t> live(n_total, 0);
  uint32_t next = 0;
  for (auto& l : lists)
    for (uint32_t r = 0; r < l.cap; ++r) {
      const uint32_t row = l.off + r;
      if (r < l.len) { row_ids[row] = pool[next++]; live[row_ids[row]] = 1; }
      else {
        for (uint32_t c = 0; c < ld; ++c) at(row, c) = (r & 1) ? NAN : 1e30f;
        row_ids[row] = (r % 3 == 0) ? 0xFFFFFFFFu : pool[(row * 7) % m];
      }
    }
  for (uint32_t c = d; c < ld; ++c)
    for (auto& l : lists)
      for (uint32_t r = 0; r < l.len; ++r) at(l.off + r, c) = 77.0f;  // what a tile holds past d must not reach X'
  for (uint64_t v = 0; v < n_total; ++v) rank[v + 1] = rank[v] + live[v];
  if (rank[n_total] != m) { printf("bad test\n"); return 1; }
  const float kGuard = -7.0f;
  std::vector<float> out((size_t)m * pitch, kGuard);
  std::vector<f32x4> lds(64 * 65 + 16);  // [64][kGatherCols4 + 1] float4s | 64 destinations
  g_lds = lds.data();
  for (uint32_t b = 0; b < tiles.size(); ++b) {
    std::barrier<> bb(256);
    g_block_bar = &bb;
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < 256; ++t)
      th.emplace_back([&, t, b] {
        threadIdx.x = t; blockIdx.x = b;
        vers::tiles_to_live_rows_kernel(src.data(), ld, d, pitch, tiles.data(), row_ids.data(), rank.data(), n_total, m, out.data());
      });
    for (auto& t : th) t.join();
  }
  int bad = 0;
  std::vector<uint8_t> seen(m, 0);
  for (auto& l : lists)
    for (uint32_t r = 0; r < l.len; ++r) {
      const uint32_t row = l.off + r, v = row_ids[row];
      const uint64_t j = rank[v];
      seen[j] = 1;
      for (uint32_t c = 0; c < pitch; ++c) {
        const float want = c < d ? at(row, c) : 0.0f;
        if (bits(out[j * pitch + c]) != bits(want)) { if (!bad) printf("row %u (vec id %u -> %llu) column %u\n", row, v, (unsigned long long)j, c); ++bad; }
      }
    }
  for (uint32_t j = 0; j < m; ++j)
    if (!seen[j]) ++bad;
  for (float v : out)
    if (v != v || v == 1e30f || v == kGuard || v == 77.0f) { ++bad; break; }  // slack, an unwritten element, a tile's padding
  printf("ld %u d %u pitch %u: %s\n", ld, d, pitch, bad ? "MISMATCH" : "ok");
  return bad;
}

int main() {
  int bad = 0;
  bad += run(64, 1, 4);        // one column of data in a 16-byte piece
  bad += run(64, 64, 64);      // d == ld
  bad += run(64, 33, 36);      // d < pitch < ld
  bad += run(320, 300, 300);   // two column passes, the second ragged
  bad += run(320, 318, 320);   // padding columns inside the last float4
  bad += run(768, 768, 768);   // three whole passes
  bad += run(1536, 1530, 1532);
  return bad ? 1 : 0;
}
