// head_stream_probe.hip -- how fast can a launch of the head filter's shape (head_filter.hip.h) stream int8 tile prefixes, as a function
// of the schedule of its loads?  
//
// The filter's shape and nothing else: blocks of 4 waves, two per CU (two waves per SIMD); a block strides over quads of 26 tiles, a
// wave per segment of 7 | 7 | 6 | 6 tiles; a tile is H = 384 columns x 64 rows of int8 (24 KiB) of which the first 256 columns are
// read in four 4 KiB steps (4 x 16 bytes per lane); M v_mfma_i32_32x32x32_i8 per step against an operand in LDS; a dependent VALU
// chain per tile where the filter computes its verdict; and per quad a serial prologue -- a chain of five dependent loads, a 24 KiB
// gather into LDS and three barriers -- where the filter stages the quad's queries.
//   schedule a: the filter as round 13 left it -- one step in flight during a step's math, none during the verdict, none during the prologue
//   schedule b: a ring of R slots that crosses tile boundaries: a slot is issued again as soon as its step is consumed, the slot of a
//               tile's last step after the verdict (the filter needs that slot for the steps a surviving tile reads on demand)
//   schedule c: b with the first R loads of the wave's next segment issued ahead of the prologue
//   hipcc --offload-arch=gfx950 -O3 -std=c++20 -o head_stream_probe head_stream_probe.hip && ./head_stream_probe [quads]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;

constexpr unsigned kTileSteps = 6, kFirst = 4;   // H = 384: six 4 KiB steps per tile, four of them read
constexpr unsigned kQuadTiles = 26, kChain = 5, kTab = 1u << 16;
constexpr unsigned kQBytes = 64u * 384u;         // the quad's operands in LDS: 64 queries x H

template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {  // f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>)
  [&]<int... i>(std::integer_sequence<int, i...>) { (f(std::integral_constant<int, i>{}), ...); }(std::make_integer_sequence<int, N>{});
}
__device__ __forceinline__ unsigned seg_first(unsigned w) { return w * 7u - (w == 3u ? 1u : 0u); }  // 0 | 7 | 14 | 20
__device__ __forceinline__ unsigned seg_tiles(unsigned w) { return w < 2u ? 7u : 6u; }

template <int SCHED, int R, int M>   // SCHED 0 | 1 | 2 = a | b | c; M = MFMAs per 1 KiB piece (1 | 2: 4 | 8 per step)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void head_stream_kernel(const u32x4* base, const unsigned* table, const u32x4* q8,
                                                                                                       unsigned n_quads, float* sink) {
  __shared__ __attribute__((aligned(16))) unsigned char qb[kQBytes];
  __shared__ unsigned idx_l[64];
  const unsigned lane = threadIdx.x & 63u, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  i32x16 acc[2] = {};
  float vsum = 0.0f;
  u32x4 ring[R][4];
  const u32x4* sp = nullptr;  // the wave's segment (+ lane)
  unsigned n_tiles = 0;
  auto segment = [&](unsigned q) {
    sp = base + ((size_t)q * kQuadTiles + seg_first(wid)) * (kTileSteps * 256u) + lane;
    n_tiles = seg_tiles(wid);
  };
  auto issue = [&](auto stag, unsigned p) {  // stream position p of the segment: (tile, step) = (p / 4, p % 4), clamped to the last one
    constexpr int s = decltype(stag)::value;
    const unsigned pc = p < n_tiles * kFirst ? p : n_tiles * kFirst - 1u;
    const u32x4* a = sp + (size_t)((pc / kFirst) * kTileSteps + (pc % kFirst)) * 256u;
#pragma unroll
    for (int i = 0; i < 4; ++i) ring[s][i] = __builtin_nontemporal_load(a + i * 64);
  };
  auto consume = [&](auto stag, unsigned step) {
    constexpr int s = decltype(stag)::value;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const i32x4 b = *reinterpret_cast<const i32x4*>(qb + ((size_t)((step * 4u + (unsigned)i) * 64u + lane)) * 16u);
      const i32x4 a = __builtin_bit_cast(i32x4, ring[s][i]);
#pragma unroll
      for (int m = 0; m < M; ++m) acc[(i + m) & 1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc[(i + m) & 1], 0, 0, 0);
    }
  };
  auto verdict = [&]() {  // a few hundred cycles of dependent VALU on what the MFMAs left
    float x = (float)(acc[0][0] + acc[1][5]);
#pragma unroll
    for (int i = 0; i < 40; ++i) x = x * 1.0001f + 0.5f;
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    vsum += x;
  };
  auto prologue = [&](unsigned q) {  // the quad change: a chain of dependent loads per query slot, a gather into LDS, three barriers
    __syncthreads();
    if (threadIdx.x < 64u) {
      unsigned idx = q * 64u + threadIdx.x;
      for (unsigned k = 0; k < kChain; ++k) idx = table[(idx * 2654435761u + k) & (kTab - 1u)];
      idx_l[threadIdx.x] = idx;
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < kQBytes / 16u; i += 256u)
      *reinterpret_cast<u32x4*>(qb + (size_t)i * 16u) = q8[(size_t)(idx_l[i / 24u] & 1023u) * 24u + i % 24u];
    __syncthreads();
  };
  if constexpr (SCHED == 2) {
    if (blockIdx.x < n_quads) {
      segment(blockIdx.x);
      static_for<R>([&](auto r) { issue(r, (unsigned)decltype(r)::value); });
    }
  }
  for (unsigned q = blockIdx.x; q < n_quads; q += gridDim.x) {
    prologue(q);
    if constexpr (SCHED == 0) {
      segment(q);
      for (unsigned t = 0; t < n_tiles; ++t) {
        issue(std::integral_constant<int, 0>{}, t * kFirst);
        issue(std::integral_constant<int, 1>{}, t * kFirst + 1u);  consume(std::integral_constant<int, 0>{}, 0u);
        issue(std::integral_constant<int, 0>{}, t * kFirst + 2u);  consume(std::integral_constant<int, 1>{}, 1u);
        issue(std::integral_constant<int, 1>{}, t * kFirst + 3u);  consume(std::integral_constant<int, 0>{}, 2u);
        consume(std::integral_constant<int, 1>{}, 3u);
        verdict();
      }
    } else {
      if constexpr (SCHED == 1) {
        segment(q);
        static_for<R>([&](auto r) { issue(r, (unsigned)decltype(r)::value); });
      }
      // R tiles per trip so that every slot index is a constant: step s of the trip's k-th tile sits in slot (4 k + s) % R
      for (unsigned t0 = 0; t0 < n_tiles; t0 += R) {
        static_for<R>([&](auto kt) {
          constexpr int k = decltype(kt)::value;
          const unsigned t = t0 + (unsigned)k;
          if (t >= n_tiles) return;
          static_for<4>([&](auto st) {
            constexpr int s = decltype(st)::value, slot = (4 * k + s) % R;
            consume(std::integral_constant<int, slot>{}, (unsigned)s);
            if constexpr (s == 3) verdict();
            issue(std::integral_constant<int, slot>{}, t * kFirst + (unsigned)s + (unsigned)R);
          });
        });
      }
      if constexpr (SCHED == 2) {  // the next segment's first loads go out before the barriers of the quad change
        if (q + gridDim.x < n_quads) {
          segment(q + gridDim.x);
          static_for<R>([&](auto r) { issue(r, (unsigned)decltype(r)::value); });
        }
      }
    }
  }
  float t = vsum;
  for (int e = 0; e < 16; ++e) t += (float)(acc[0][e] + acc[1][e]);
  if (t == 12345.678f) sink[threadIdx.x] = t;
}

template <int SCHED, int R, int M>
void run(const char* name, const u32x4* base, const unsigned* table, const u32x4* q8, unsigned n_quads, float* sink, int n_cu) {
  hipEvent_t a, b;
  CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
  float best = 1e30f, sum = 0.0f;
  const int reps = 10;
  for (int i = 0; i < reps + 2; ++i) {
    CK(hipEventRecord(a, nullptr));
    hipLaunchKernelGGL((head_stream_kernel<SCHED, R, M>), dim3(2 * n_cu), dim3(256), 0, nullptr, base, table, q8, n_quads, sink);
    CK(hipEventRecord(b, nullptr));
    CK(hipEventSynchronize(b));
    float ms = 0.0f;
    CK(hipEventElapsedTime(&ms, a, b));
    if (i >= 2) { best = std::min(best, ms); sum += ms; }
  }
  CK(hipGetLastError());
  const double bytes = (double)n_quads * kQuadTiles * kFirst * 4096.0;
  printf("%-46s mean %7.1f us  min %7.1f us  -> %5.2f TB/s (mean) %5.2f TB/s (best)\n", name, sum / reps * 1e3, best * 1e3, bytes / (sum / reps * 1e-3) / 1e12,
         bytes / (best * 1e-3) / 1e12);
  fflush(stdout);
}

int main(int argc, char** argv) {
  const unsigned n_quads = argc > 1 ? (unsigned)atoi(argv[1]) : 4096u;  // 4096 x 26 tiles x 16 KiB read = 1.74 GB (cfg3: 3978 cold quads, ~103 k tiles)
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const int n_cu = prop.multiProcessorCount;
  const size_t buf_bytes = (size_t)n_quads * kQuadTiles * kTileSteps * 4096u;
  u32x4 *base, *q8; unsigned* table; float* sink;
  CK(hipMalloc(&base, buf_bytes)); CK(hipMemset(base, 0x01, buf_bytes));
  std::vector<unsigned> tab(kTab);
  unsigned seed = 12345u;
  for (unsigned i = 0; i < kTab; ++i) { seed = seed * 1664525u + 1013904223u; tab[i] = seed >> 8; }
  CK(hipMalloc(&table, kTab * 4)); CK(hipMemcpy(table, tab.data(), kTab * 4, hipMemcpyHostToDevice));
  CK(hipMalloc(&q8, 1024u * 384u)); CK(hipMemset(q8, 0x02, 1024u * 384u));
  CK(hipMalloc(&sink, 4096 * 4));
  printf("%d CUs; %u quads x %u tiles; %.2f GB read of a %.2f GB head; at 6.3 TB/s: %.0f us\n", n_cu, n_quads, kQuadTiles, (double)n_quads * kQuadTiles * kFirst * 4096.0 / 1e9,
         (double)buf_bytes / 1e9, (double)n_quads * kQuadTiles * kFirst * 4096.0 / 6.3e12 * 1e6);
#define RUN(S, R, M) run<S, R, M>("schedule " #S " (0 a | 1 b | 2 c)  ring " #R "  MFMA/piece " #M, base, table, q8, n_quads, sink, n_cu)
  RUN(0, 2, 2); RUN(0, 2, 1);
  RUN(1, 2, 2); RUN(1, 3, 2); RUN(1, 4, 2);
  RUN(2, 2, 2); RUN(2, 3, 2); RUN(2, 4, 2);
  RUN(2, 4, 1);
  return 0;
}
