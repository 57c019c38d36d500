// item_loop.hip.h -- how a block of the range and filtered list-scan kernels comes by its work items: scan_kernel's grid and hand-out
// (scan.hip.h; that kernel keeps its own copy, with the phase stamps in it), once for range_scan_kernel, filter_scan_kernel and
// filter_range_scan_kernel.
#pragma once
#include <type_traits>

#include "scan.hip.h"

namespace vers {

// item(it, v) for every item of the block's waves that has rows, v.qb ready to read.
//   QG == 1: waves are independent, a static stride over the items.
//   QG  > 1: items come in QUADS that share one query block (Src pads with empty items): the block's four waves stage it into LDS once
//            and each takes its own item of the quad.  Quads are handed out through `next_quad` (zeroed by the launcher; nullptr = a static
//            stride), one agent-scope atomic per quad and one LDS word to spread it.  `item` runs between barriers, never around one: a
//            padding item skips it, wave-uniformly.
// The callers' lambdas are __attribute__((always_inline)), here and in filter_walk.hip.h: a closure's operator() inside a template is
// linkonce_odr, so the inliner weighs its size instead of taking the one call site -- left out of line, the QG = 16 top-k kernel went from
// 239 VGPRs to 256 + AGPRs + scratch and lost a wave per SIMD (profiles/r26_summary.txt).
template <int QG, class Src, class F>
__device__ __forceinline__ void for_each_item(const Src& src, uint32_t ld, uint32_t* next_quad, int wid, F&& item) {
  const uint32_t n_items = src.n_items();
  if constexpr (QG == 1) {
    const uint32_t n_waves = gridDim.x * kWavesPerBlock;
    for (uint32_t it = blockIdx.x * kWavesPerBlock + wid; it < n_items; it += n_waves) {
      ItemView<QG> v;
      src.get(it, v);
      if (v.nrows == 0) continue;
      item(it, v);
    }
  } else {
    static_assert(QG == 8 || QG == 16, "query groups are 1, 8 or 16 wide");
    static_assert(kWavesPerBlock == 4, "items are padded to quads");
    extern __shared__ __attribute__((aligned(16))) float qlds[];
    const uint32_t n_quads = n_items / 4;
    const uint32_t n4 = ld * (QG / 4);  // float4s of one query block
    uint32_t* nq_lds = reinterpret_cast<uint32_t*>(qlds + (size_t)ld * QG);  // one word behind the query block
    for (uint32_t b0 = blockIdx.x;; b0 += gridDim.x) {
      uint32_t bi = b0;
      if (next_quad != nullptr) {
        if (threadIdx.x == 0) *nq_lds = atomicAdd(next_quad, 1u);
        __syncthreads();
        bi = *nq_lds;  // every wave reads it before the next write: two barriers follow below
      }
      if (bi >= n_quads) break;  // block-uniform
      const uint32_t it = bi * 4 + wid;
      ItemView<QG> v;
      src.get(it, v);  // v.qb / v.nq are the same for the four items of the quad
      __syncthreads();  // the previous quad's readers are done with the LDS block
      const f32x4* g = reinterpret_cast<const f32x4*>(v.qb);
      for (uint32_t i = threadIdx.x; i < n4; i += kWave * kWavesPerBlock) reinterpret_cast<f32x4*>(qlds)[i] = g[i];
      __syncthreads();
      v.qb = qlds;
      if (v.nrows == 0) continue;  // padding item (wave-uniform; barriers are outside)
      item(it, v);
    }
  }
}

// range search's dispatch on the live query pairs of a batched item, in steps of two (tile_chunk_compute reads two pairs per ds_read_b128):
// f(std::integral_constant<int, NP>), wave-uniform
template <int QG, class F>
__device__ __forceinline__ void with_pairs_by_two(uint32_t nq, F&& f) {
  const uint32_t np = ((nq + 3) >> 2) << 1;
  if constexpr (QG == 8) {
    if (np <= 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 4>{});
  } else {
    switch (np) {
      case 2: f(std::integral_constant<int, 2>{}); break;
      case 4: f(std::integral_constant<int, 4>{}); break;
      case 6: f(std::integral_constant<int, 6>{}); break;
      default: f(std::integral_constant<int, 8>{}); break;
    }
  }
}

}  // namespace vers
