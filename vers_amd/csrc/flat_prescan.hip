// flat_prescan.hip -- the kernels of flat_prescan.hip.h and their launches: the matrix-core scan of a flat batch over the fp16 shadow.
// A translation unit of its own; the exact finish behind it is launched where it lives (ivf_search.hip: flat_shadow_search_batch).
#define VERS_FLAT_PRESCAN_KERNELS
#include "flat_prescan.hip.h"
#include "scan_launch.hip.h"

namespace vers {

int32_t launch_flat_pre_begin(const FlatPreTables& t, uint32_t b, uint32_t n_segs, uint32_t n, hipStream_t st) {
  hipLaunchKernelGGL(flat_pre_begin_kernel, dim3((b + 255u) / 256u), dim3(256), 0, st, t, b, n_segs, n);
  VERS_HIP_TRY(hipGetLastError());
  return VERS_OK;
}

int32_t launch_flat_prescan(const FlatPreArgs& a, const FlatPrePlan& p, hipStream_t st) {
  const uint32_t blocks = p.n_segs * p.n_qb;
  if (p.nq == 64u) {
    return p.lo ? launch_scan(flat_prescan_kernel<2, true>, blocks, (int)p.waves, p.lds, st, a)
                : launch_scan(flat_prescan_kernel<2, false>, blocks, (int)p.waves, p.lds, st, a);
  }
  return p.lo ? launch_scan(flat_prescan_kernel<1, true>, blocks, (int)p.waves, p.lds, st, a)
              : launch_scan(flat_prescan_kernel<1, false>, blocks, (int)p.waves, p.lds, st, a);
}

}  // namespace vers
