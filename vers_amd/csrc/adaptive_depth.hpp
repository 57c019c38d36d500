// adaptive_depth.hpp -- the depth rule of the adaptive filtered search (filter_adaptive.hip.h), without a HIP dependency: the plan kernel
// applies it rank by rank on the device, tests/cpp/adaptive_depth_demo.cpp restates a query's walk with it under the host compiler.
//
// A query's lists are L_0, L_1, ... in ranking order, a_j = live rows of L_j its bitmap allows, A_j = a_0 + ... + a_{j-1} (the allowed rows
// BEFORE rank j).  With P_min = min(nprobe_min, k), P_max = min(nprobe_max, k) the query probes the smallest P in [P_min, P_max] with
// A_P >= min_allowed, or P_max: rank j is visited exactly when j < P_min, or j < P_max and the ranks before it have not yet brought
// min_allowed rows in reach.  A_j never decreases, so the visited ranks are a prefix and their number is the depth P_q.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VERS_ADAPTIVE_HD __host__ __device__
#else
#define VERS_ADAPTIVE_HD
#endif

namespace vers {

// (p_min <= p_max, both already clamped to the number of lists)
VERS_ADAPTIVE_HD inline bool adaptive_rank_visited(uint32_t j, uint32_t allowed_before, uint32_t p_min, uint32_t p_max, uint32_t min_allowed) {
  return j < p_min || (j < p_max && allowed_before < min_allowed);
}

}  // namespace vers
