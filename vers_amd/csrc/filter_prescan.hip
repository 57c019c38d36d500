// filter_prescan.hip -- the kernels of filter_prescan.hip.h and their launches: the matrix-core scan of a filtered top-k search's allowed rows
// and the filtered fallback.  A translation unit of its own (vers_amd/build.py compiles it without packed f32 VALU operations).
#define VERS_FILTER_PRESCAN_KERNELS
#include "filter_prescan.hip.h"

namespace vers {

int32_t launch_filter_pre_begin(const uint32_t* pj_list, const uint32_t* list_len, uint64_t n_pairs, uint32_t seg_rows, uint32_t* pj_nq, unsigned long long* total, hipStream_t st) {
  hipLaunchKernelGGL(filter_pre_begin_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, st, pj_list, list_len, n_pairs, seg_rows, pj_nq, total);
  VERS_HIP_TRY(hipGetLastError());
  return VERS_OK;
}

template <int QG>
static int32_t launch_fp(int metric, const IvfSrc<QG>& src, const FilterPreParams& p, uint32_t blocks, hipStream_t st) {
  return with_metric(metric, [&](auto m) -> int32_t {
    return ivf::launch_scan_timed(filter_prescan_kernel<QG, decltype(m)::value, IvfSrc<QG>>, blocks, kWavesPerBlock, filter_prescan_lds_bytes(p.ld), st, src, p);
  });
}
int32_t launch_filter_prescan(int metric, const IvfSrc<8>& src, const FilterPreParams& p, uint32_t blocks, hipStream_t st) { return launch_fp<8>(metric, src, p, blocks, st); }
int32_t launch_filter_prescan(int metric, const IvfSrc<16>& src, const FilterPreParams& p, uint32_t blocks, hipStream_t st) { return launch_fp<16>(metric, src, p, blocks, st); }

int32_t launch_filter_fallback(int metric, const FilterFbParams& a, uint32_t blocks, hipStream_t st) {
  const size_t lds = (size_t)a.ld * sizeof(float) + (size_t)kFpFbWaves * kWave * sizeof(uint64_t);
  return with_metric(metric, [&](auto m) -> int32_t { return launch_scan(filter_fallback_kernel<decltype(m)::value>, blocks, kFpFbWaves, lds, st, a); });
}

}  // namespace vers
