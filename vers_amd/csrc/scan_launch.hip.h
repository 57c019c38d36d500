// scan_launch.hip.h -- how the host launches the scan engine's kernels (scan.hip.h, range.hip.h, filter.hip.h), whichever handle owns the
// rows: the dispatch from a run-time metric / query-group width to the kernel instantiation, the launch itself, and the fill of a segment
// source from a segment plan (seg_plan.hpp).  Templates and generic lambdas only: nothing here costs a call a heap allocation or a HIP call.
#pragma once
#include <type_traits>

#include "scan.hip.h"

namespace vers {

// f(std::integral_constant<int, METRIC>): the caller names its kernel template once, for the launch attribute and the launch alike
template <class F>
inline int32_t with_metric(int metric, F&& f) {
  return metric ? f(std::integral_constant<int, 1>{}) : f(std::integral_constant<int, 0>{});
}

// f(std::integral_constant<int, QG>) for the width among Q0, QS... that QG names; the last one listed is the default.  The list is the
// caller's: only the widths it names are instantiated (planned list scans 1 / 8 / 16, segment scans 1 / 8, the matrix-core scan's three).
template <int Q0, int... QS, class F>
inline int32_t with_qg(int QG, F&& f) {
  if constexpr (sizeof...(QS) == 0) return f(std::integral_constant<int, Q0>{});
  else return QG == Q0 ? f(std::integral_constant<int, Q0>{}) : with_qg<QS...>(QG, f);
}

// kern<<<blocks, waves x 64, lds, st>>>(args...) behind its launch attribute (dynamic LDS beyond 48 KiB)
template <class K, class... A>
inline int32_t launch_scan(K kern, uint32_t blocks, int waves, size_t lds, hipStream_t st, const A&... args) {
  if (int32_t rc = scan_prepare_launch(kern, lds)) return rc;
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(kWave * waves), lds, st, args...);
  VERS_HIP_TRY(hipGetLastError());
  return VERS_OK;
}

// a segment source (SegSrc / FlatSrc: the same fields) over `n` rows cut as `sp` says; k keys per (query, segment) slot of `partials`
template <class Src>
inline Src make_seg_src(const float* rows, uint64_t n, uint32_t ld, const SegPlan& sp, const float* queries, uint32_t ldq, uint32_t b, uint64_t* partials,
                        uint32_t k, const uint32_t* ids) {
  Src src;
  src.rows = rows; src.n = n; src.ld = ld; src.seg_rows = sp.seg_rows; src.n_segs = sp.n_segs; src.n_segs_pad = sp.n_segs_pad;
  src.queries = queries; src.ldq = ldq; src.b = b; src.partials = partials; src.k = k; src.ids = ids;
  return src;
}

}  // namespace vers
