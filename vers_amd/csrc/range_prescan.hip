// range_prescan.hip -- the kernels of range_prescan.hip.h and their launches: the matrix-core pre-filter of the probed range search and its
// exact finish.  A translation unit of its own (vers_amd/build.py compiles it without packed f32 VALU operations).
#define VERS_RANGE_PRESCAN_KERNELS
#include "range_prescan.hip.h"

namespace vers {

int32_t launch_range_cut(const float* qp, uint32_t ldq, uint32_t ld, uint32_t b, const uint32_t* misc, const float* radius, int metric, float* cut, hipStream_t st) {
  hipLaunchKernelGGL(range_cut_kernel, dim3((b + 3) / 4), dim3(256), 0, st, qp, ldq, ld, b, misc, radius, metric, cut);
  VERS_HIP_TRY(hipGetLastError());
  return VERS_OK;
}

int32_t launch_range_pair_tiles(const uint32_t* pj_list, const uint32_t* list_len, uint64_t n_pairs, uint32_t* tiles, hipStream_t st) {
  hipLaunchKernelGGL(range_pair_tiles_kernel, dim3((unsigned)((n_pairs + 1 + 255) / 256)), dim3(256), 0, st, pj_list, list_len, n_pairs, tiles);
  VERS_HIP_TRY(hipGetLastError());
  return VERS_OK;
}

template <int QG>
static int32_t launch_prefilter(int metric, const IvfSrc<QG>& src, const RangePreParams& p, uint32_t blocks, hipStream_t st) {
  return with_metric(metric, [&](auto m) -> int32_t {
    return launch_scan(range_prefilter_kernel<QG, decltype(m)::value, IvfSrc<QG>>, blocks, kWavesPerBlock, range_prefilter_lds_bytes(p.ld), st, src, p);
  });
}
int32_t launch_range_prefilter(int metric, const IvfSrc<8>& src, const RangePreParams& p, uint32_t blocks, hipStream_t st) { return launch_prefilter<8>(metric, src, p, blocks, st); }
int32_t launch_range_prefilter(int metric, const IvfSrc<16>& src, const RangePreParams& p, uint32_t blocks, hipStream_t st) { return launch_prefilter<16>(metric, src, p, blocks, st); }

int32_t launch_range_exact(int metric, bool fill, const RangeExactParams& e, const RangeParams& p, uint32_t blocks, hipStream_t st) {
  const size_t lds = range_exact_lds_bytes(e.ld);
  return with_metric(metric, [&](auto m) -> int32_t {
    constexpr int M = decltype(m)::value;
    if (fill) return launch_scan(range_exact_kernel<M, true>, blocks, kWavesPerBlock, lds, st, e, p);
    return launch_scan(range_exact_kernel<M, false>, blocks, kWavesPerBlock, lds, st, e, p);
  });
}

int32_t launch_range_stats_fold(const unsigned long long* pre_slots, uint32_t pre_waves, const unsigned long long* exact_slots, uint32_t exact_waves,
                                unsigned long long* total, hipStream_t st) {
  hipLaunchKernelGGL(range_stats_fold_kernel, dim3(1), dim3(256), 0, st, pre_slots, pre_waves, exact_slots, exact_waves, total);
  VERS_HIP_TRY(hipGetLastError());
  return VERS_OK;
}

}  // namespace vers
