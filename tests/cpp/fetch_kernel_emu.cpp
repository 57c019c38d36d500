// Host emulation of fetch_tiles_kernel (vers_amd/csrc/fetch.hip.h): the kernel's own text -- cut out of the source between its two marker
// comments by tests/test_fetch_kernel_host.py into kernel_snip.h -- runs as 256 std::threads per block with the barriers as std::barrier, on
// buffers sized exactly (an AddressSanitizer build sees any access outside them), and the output is compared bit for bit with a plain
// restatement: request i for storage row r receives the d floats of r, a request for an id in no list receives d zeros, nothing else is
// written.  argv[1] = T, the library's threshold between the direct and the LDS form: the requests put 1, T - 1, T and 64 wanted rows on
// tiles of their own, so both forms run whatever T is; every layout also runs with T = 1 (always LDS) and T = 1000 (never).
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <thread>
#include <vector>
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define __global__
#define __device__
#define __launch_bounds__(x)
struct Idx { uint32_t x; };
static thread_local Idx threadIdx, blockIdx;
static f32x4* g_lds;
static std::barrier<>* g_block_bar;
static void lds_barrier() { g_block_bar->arrive_and_wait(); }
constexpr uint32_t kFetchCols4 = 64;
namespace vers {
#include "kernel_snip.h"
}

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
constexpr uint32_t kNone = 0xFFFFFFFFu;

// lists (offset in rows, capacity, length): lengths 1, 63, 64, 65 (a second tile of one row), 0 and 130 (two whole tiles + 2)
struct List { uint32_t off, cap, len; };

int run(uint32_t ld, uint32_t d, uint32_t pitch, uint32_t T, uint32_t lds_min, bool aligned) {
  const std::vector<List> lists = {{0, 64, 1}, {64, 128, 63}, {192, 128, 64}, {320, 128, 65}, {448, 64, 0}, {512, 192, 130}};
  const uint32_t cap_rows = 704;
  std::mt19937 rng(ld * 31 + d + lds_min);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::vector<float> src((size_t)cap_rows * ld);
  for (auto& v : src) v = nd(rng);
  auto at = [&](uint32_t row, uint32_t c) -> float& { return src[(size_t)(row / 64) * 64 * ld + ((size_t)(c / 4) * 64 + row % 64) * 4 + c % 4]; };
  // slack rows hold NaN / 1e30 in every column (their row_ids entries may look live: the gather never reads row_ids, and what a slack row
  // holds gets as far as LDS at most); the tiles' padding columns hold 77
  for (auto& l : lists)
    for (uint32_t r = 0; r < l.cap; ++r)
      for (uint32_t c = 0; c < ld; ++c) {
        if (r >= l.len) at(l.off + r, c) = (r & 1) ? NAN : 1e30f;
        else if (c >= d) at(l.off + r, c) = 77.0f;
      }
  // the wanted storage rows: 1 of list 0's tile | every row of list 2's tile (64) | T - 1 rows of list 5's first tile, T of its second, its
  // last two rows | list 1: rows 0, 31 and 62, row 31 TWICE (a repeated id: two destinations) | list 3: row 0 and its 65th row | two requests
  // for ids in no list
  std::vector<uint32_t> want;
  want.push_back(0);
  for (uint32_t r = 0; r < 64; ++r) want.push_back(192 + r);
  for (uint32_t r = 0; r + 1 < std::min(T, 65u); ++r) want.push_back(512 + (r * 5) % 64);
  for (uint32_t r = 0; r < std::min(T, 64u); ++r) want.push_back(576 + (r * 3) % 64);
  want.push_back(640); want.push_back(641);
  want.push_back(64); want.push_back(95); want.push_back(126); want.push_back(95);
  want.push_back(320); want.push_back(384);
  want.push_back(kNone); want.push_back(kNone);
  std::shuffle(want.begin(), want.end(), rng);
  const uint32_t n = (uint32_t)want.size();
  // the device's preparation, restated: (storage row, request) pairs in a stable ascending sort, a job per touched tile, each request for
  // an id in no list a job of its own
  std::vector<uint32_t> order(n);
  for (uint32_t i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return want[a] < want[b]; });
  std::vector<uint32_t> skeys(n), svals(n), job_begin;
  for (uint32_t p = 0; p < n; ++p) { skeys[p] = want[order[p]]; svals[p] = order[p]; }
  for (uint32_t p = 0; p < n; ++p)
    if (p == 0 || skeys[p] == kNone || (skeys[p] >> 6) != (skeys[p - 1] >> 6)) job_begin.push_back(p);
  const float kGuard = -7.0f;
  const size_t out_floats = (size_t)n * pitch;
  // (operator new[] returns 16-byte aligned storage; the buffer ends where the output ends.  An output that is not 16-byte aligned takes
  // the float-by-float stores.)
  float* base = new float[out_floats + (aligned ? 0 : 1)];
  float* out = aligned ? base : base + 1;
  if (((uintptr_t)out % 16 == 0) != aligned) { printf("bad test\n"); return 1; }
  for (size_t i = 0; i < out_floats; ++i) out[i] = kGuard;
  const int vec = aligned && pitch % 4 == 0 ? 1 : 0;
  std::vector<f32x4> lds(64 * 65);  // [64][kFetchCols4 + 1] float4s
  g_lds = lds.data();
  for (uint32_t b = 0; b < job_begin.size(); ++b) {
    std::barrier<> bb(256);
    g_block_bar = &bb;
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < 256; ++t)
      th.emplace_back([&, t, b] {
        threadIdx.x = t; blockIdx.x = b;
        vers::fetch_tiles_kernel(src.data(), ld, d, job_begin.data(), (uint32_t)job_begin.size(), n, skeys.data(), svals.data(), lds_min, out, pitch, vec);
      });
    for (auto& t : th) t.join();
  }
  int bad = 0;
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t c = 0; c < pitch; ++c) {
      const float wantv = c >= d ? kGuard : (want[i] == kNone ? 0.0f : at(want[i], c));
      if (bits(out[(size_t)i * pitch + c]) != bits(wantv)) { if (!bad) printf("request %u (row %u) column %u\n", i, want[i], c); ++bad; }
    }
  for (size_t i = 0; i < out_floats; ++i)
    if (out[i] != out[i] || out[i] == 1e30f || out[i] == 77.0f) { ++bad; break; }  // slack, a tile's padding
  delete[] base;
  printf("ld %u d %u pitch %u lds_min %u %s: %s\n", ld, d, pitch, lds_min, aligned ? "aligned" : "unaligned", bad ? "MISMATCH" : "ok");
  return bad;
}

int main(int argc, char** argv) {
  const uint32_t T = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 64u;
  int bad = 0;
  for (uint32_t lds_min : {T, 1u, 1000u}) {
    bad += run(64, 1, 4, T, lds_min, true);        // one column of data in a 16-byte piece
    bad += run(64, 1, 1, T, lds_min, true);        // ... at pitch 1
    bad += run(320, 300, 304, T, lds_min, true);   // two column passes, the second ragged; padding behind every row
    bad += run(320, 300, 303, T, lds_min, false);  // an output the 16-byte stores cannot serve
    bad += run(768, 768, 776, T, lds_min, true);   // three whole passes
  }
  return bad ? 1 : 0;
}
