// flat_audit.hip (libvers_hip_test.so) -- TEST HOOKS: the flat corpus' single query on its fp16 shadow (flat1h_kernel + the inverted lists'
// exact finish, flat_shadow_search1 in ivf_search.hip).  That path keeps its own max |x|^2 and R^2 (flat_shadow_derive) and leaves the f32
// scan in charge -- silently -- whenever the shadow does not fit or is unusable; results are the oracle's either way.  These hooks hand back
// whether the shadow exists, the maxima and the failed-certificate count as the device holds them, and every (row, val) the scan left in
// its slots with the bound the certificate charges it, so that tests/test_certificate_single_gpu.py can hold each against the reference's
// ordered chain, as vers_ivf_test_last_vals does for the inverted lists.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "../common.hpp"      // fail, VERS_HIP_TRY, kKeyMax
#include "../flat_handle.hpp"  // struct vers_flat, FlatShadow, flat_shadow_usable
#include "../prescan.hip.h"    // pre_bound, kPreMaxKp; order_bits_to_f32_bits (scan.hip.h)
#include "../util.hip.h"       // DeviceGuard
#include "../../../include/vers_hip_audit.h"

using namespace vers;

extern "C" {

int32_t vers_flat_test_shadow_state(vers_flat_t* h, double* out_state8) {
  if (!h || !out_state8) return fail(VERS_ERR_INVALID, "vers_flat_test_shadow_state: bad arguments");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  VERS_HIP_TRY(hipDeviceSynchronize());
  const FlatShadow& s = h->shadow;
  const bool present = h->n != 0 && s.rows_built == h->n && s.rows_h != nullptr && s.misc != nullptr;
  uint32_t misc[4] = {0, 0, 0, 0};
  if (present) VERS_HIP_TRY(hipMemcpy(misc, s.misc, sizeof(misc), hipMemcpyDeviceToHost));
  float xmax2, r2;
  std::memcpy(&xmax2, &misc[0], 4); std::memcpy(&r2, &misc[2], 4);
  out_state8[0] = present ? 1.0 : 0.0; out_state8[1] = present ? s.n_slots : 0u; out_state8[2] = xmax2; out_state8[3] = r2;
  out_state8[4] = misc[1]; out_state8[5] = h->ld; out_state8[6] = (double)h->n; out_state8[7] = (double)s.rows_built;
  return VERS_OK;
}

int32_t vers_flat_test_last_vals(vers_flat_t* h, const float* query, uint32_t top_k, uint32_t metric, uint64_t* out_vec_ids, float* out_vals,
                                 double* out_bound, uint32_t cap, uint32_t* out_n, double* out_info8) {
  if (!h || !query || !out_n || metric > VERS_METRIC_COSDIST || (cap && (!out_vec_ids || !out_vals || !out_bound)))
    return fail(VERS_ERR_INVALID, "vers_flat_test_last_vals: bad arguments");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  VERS_HIP_TRY(hipDeviceSynchronize());
  const FlatShadow& s = h->shadow;
  if (!flat_shadow_usable(s, h->n, h->ld, top_k) || s.misc == nullptr || s.slots == nullptr)
    return fail(VERS_ERR_INVALID, "vers_flat_test_last_vals: a single query with this top_k does not take the fp16 shadow on this handle");
  const uint32_t kp = std::min<uint32_t>(kPreMaxKp, top_k + std::max<uint32_t>(24, top_k));  // (as flat_shadow_search1 cuts its slots)
  std::vector<uint64_t> keys((size_t)s.n_slots * kp);
  VERS_HIP_TRY(hipMemcpy(keys.data(), s.slots, keys.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  uint32_t misc[4] = {0, 0, 0, 0};
  VERS_HIP_TRY(hipMemcpy(misc, s.misc, sizeof(misc), hipMemcpyDeviceToHost));
  float xmax2, r2;
  std::memcpy(&xmax2, &misc[0], 4); std::memcpy(&r2, &misc[2], 4);
  double qn = 0.0;
  for (uint32_t j = 0; j < h->d; ++j) qn += (double)query[j] * (double)query[j];
  const PreBound pb = pre_bound(qn, (double)xmax2, (double)r2, h->ld, (int)metric, 1);
  if (out_info8) { out_info8[0] = qn; out_info8[1] = xmax2; out_info8[2] = r2; out_info8[3] = pb.global; out_info8[4] = pb.common; out_info8[5] = kp; out_info8[6] = 1; out_info8[7] = metric; }
  uint32_t n = 0;
  for (const uint64_t key : keys) {
    if (key == kKeyMax) continue;
    if (n < cap) {
      const uint32_t vb = order_bits_to_f32_bits((uint32_t)(key >> 32));
      float v; std::memcpy(&v, &vb, 4);
      out_vec_ids[n] = (uint32_t)key; out_vals[n] = v; out_bound[n] = pb.of((double)v);  // (the corpus is ONE list: sequence number = storage row = vec id)
    }
    ++n;
  }
  *out_n = n;
  return VERS_OK;
}

}  // extern "C"
