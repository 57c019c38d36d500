// Host emulation of compact_tiles_kernel (vers_amd/csrc/ivf_build.hip): the kernel's own text -- cut out of the source by
// tests/test_compact_kernel_host.py into kernel_snip.h -- runs as 256 std::threads per block with the barriers as std::barrier, on buffers
// sized exactly (an AddressSanitizer build sees any access outside them), and every output is compared bit for bit with a
// straightforward restatement: the f32 tile, row_to_f16's shadow layout, the row-major rows, row_ids, xnorm and both maxima.
#include <atomic>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
#define __global__
#define __launch_bounds__(x)
struct Idx { uint32_t x; };
static thread_local Idx threadIdx, blockIdx;
static f32x4* g_lds;
static std::barrier<>* g_block_bar;
static std::barrier<>* g_wave_bar[4];
static uint32_t g_slot[256];
static void lds_barrier() { g_block_bar->arrive_and_wait(); }
static int __shfl_xor(int v, int o) {
  const uint32_t t = threadIdx.x;
  g_slot[t] = (uint32_t)v;
  g_wave_bar[t >> 6]->arrive_and_wait();
  const int r = (int)g_slot[t ^ (uint32_t)o];
  g_wave_bar[t >> 6]->arrive_and_wait();
  return r;
}
static uint32_t atomicMax(uint32_t* p, uint32_t v) {
  auto* a = reinterpret_cast<std::atomic<uint32_t>*>(p);
  uint32_t old = a->load();
  while (old < v && !a->compare_exchange_weak(old, v)) {}
  return old;
}
static float __fadd_rn(float a, float b) { return a + b; }
static float __fmul_rn(float a, float b) { return a * b; }
static uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
constexpr uint32_t kGatherCols4 = 64;
namespace vers {
#include "kernel_snip.h"
}
using vers::CompactJob;

int run(uint32_t ld, bool with_h, bool with_rm, int special) {
  const uint32_t src_tiles = 7, dst_tiles = 5;
  std::vector<CompactJob> jobs = {{5, 0}, {1, 3}, {6, 2}};
  std::vector<float> src((size_t)src_tiles * 64 * ld), dst((size_t)dst_tiles * 64 * ld, -7.0f), rm((size_t)dst_tiles * 64 * ld, -7.0f), xn(dst_tiles * 64, -1.0f);
  std::vector<uint16_t> sh((size_t)dst_tiles * 64 * ld, 0x1234);
  std::vector<uint32_t> sid(src_tiles * 64), did(dst_tiles * 64, 0xFFFFFFFFu), misc(16, 0);
  std::mt19937 rng(ld * 7 + special);
  std::normal_distribution<float> nd(0.f, 1.f);
  for (auto& v : src) v = nd(rng) * (rng() % 50 == 0 ? 1e-6f : 1.0f);
  for (size_t i = 0; i < sid.size(); ++i) sid[i] = (uint32_t)(1000 + i);
  for (uint32_t r = 40; r < 64; ++r) sid[6 * 64 + r] = 0xFFFFFFFFu;  // a last tile: rows 40.. hold no vector
  auto at = [&](std::vector<float>& a, uint32_t tile, uint32_t r, uint32_t c) -> float& { return a[(size_t)tile * 64 * ld + ((size_t)(c / 4) * 64 + r) * 4 + c % 4]; };
  for (uint32_t c = 0; c < ld; ++c) at(src, 6, 50, c) = NAN;              // slack rows may hold anything
  for (uint32_t c = 0; c < ld; ++c) at(src, 6, 51, c) = 1e30f;
  if (special == 1) at(src, 1, 3, 5) = 7e4f;                              // beyond fp16
  if (special == 2) at(src, 5, 9, 2) = NAN;                               // a NaN row that holds a vector
  std::vector<f32x4> lds(64 * 65);
  g_lds = lds.data();
  for (uint32_t b = 0; b < jobs.size(); ++b) {
    std::barrier<> bb(256), w0(64), w1(64), w2(64), w3(64);
    g_block_bar = &bb; g_wave_bar[0] = &w0; g_wave_bar[1] = &w1; g_wave_bar[2] = &w2; g_wave_bar[3] = &w3;
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < 256; ++t)
      th.emplace_back([&, t, b] {
        threadIdx.x = t; blockIdx.x = b;
        vers::compact_tiles_kernel(jobs.data(), ld, src.data(), sid.data(), dst.data(), did.data(), with_h ? sh.data() : nullptr, with_rm ? rm.data() : nullptr, xn.data(),
                                   misc.data(), misc.data() + 2);
      });
    for (auto& t : th) t.join();
  }
  // references
  int bad = 0;
  uint32_t xmax = 0, rmax = 0;
  std::vector<bool> written(dst_tiles, false);
  for (auto& jb : jobs) {
    written[jb.dst] = true;
    for (uint32_t r = 0; r < 64; ++r) {
      const uint32_t id = sid[jb.src * 64 + r];
      if (did[jb.dst * 64 + r] != id) { ++bad; printf("id\n"); }
      float ax = 0.f, ar = 0.f;
      for (uint32_t c = 0; c < ld; ++c) {
        const float v = at(src, jb.src, r, c);
        uint32_t a, b2;
        memcpy(&a, &v, 4); memcpy(&b2, &at(dst, jb.dst, r, c), 4);
        if (a != b2) { ++bad; }
        if (with_rm) { memcpy(&b2, &rm[((size_t)jb.dst * 64 + r) * ld + c], 4); if (a != b2) ++bad; }
        if (with_h) {
          const _Float16 hv = (_Float16)v;
          uint16_t hb; memcpy(&hb, &hv, 2);
          const uint32_t j = c / 8;
          const size_t off = (size_t)jb.dst * 64 * ld + ((size_t)((j >> 1) * 2 + (r >> 5)) * 64 + (j & 1) * 32 + (r & 31)) * 8 + c % 8;
          if (sh[off] != hb) ++bad;
        }
        ax = ax + v * v;
        const float dl = v - (float)(_Float16)v;
        ar = ar + dl * dl;
      }
      const bool hv = id != 0xFFFFFFFFu;
      const float want = hv ? ax : 0.0f;
      uint32_t a, b2; memcpy(&a, &want, 4); memcpy(&b2, &xn[jb.dst * 64 + r], 4);
      if (a != b2) { ++bad; printf("xnorm tile %u row %u\n", jb.dst, r); }
      if (hv && ax == ax) xmax = std::max(xmax, __float_as_uint(ax));
      if (hv && with_h && ar == ar) rmax = std::max(rmax, __float_as_uint(ar));
    }
  }
  if (misc[0] != xmax || misc[2] != rmax || misc[1] != 0) { ++bad; printf("maxima %x %x want %x %x\n", misc[0], misc[2], xmax, rmax); }
  for (uint32_t t = 0; t < dst_tiles; ++t)
    if (!written[t]) {
      for (size_t i = (size_t)t * 64 * ld; i < (size_t)(t + 1) * 64 * ld; ++i)
        if (dst[i] != -7.0f || rm[i] != -7.0f || sh[i] != 0x1234) { ++bad; break; }
      for (uint32_t r = 0; r < 64; ++r) if (xn[t * 64 + r] != -1.0f || did[t * 64 + r] != 0xFFFFFFFFu) ++bad;
    }
  if (!with_rm) for (float v : rm) if (v != -7.0f) { ++bad; break; }
  if (!with_h) for (uint16_t v : sh) if (v != 0x1234) { ++bad; break; }
  printf("ld %u shadow %d rowmajor %d special %d: %s (xmax bits %x, rmax bits %x)\n", ld, with_h, with_rm, special, bad ? "MISMATCH" : "ok", misc[0], misc[2]);
  return bad;
}
int main() {
  int bad = 0;
  for (uint32_t ld : {64u, 320u, 768u})
    for (int sp = 0; sp < 3; ++sp) bad += run(ld, true, true, sp);
  bad += run(128, false, true, 0);
  bad += run(128, true, false, 0);
  bad += run(1536, true, true, 0);
  return bad ? 1 : 0;
}
