// audit.hip (libvers_hip_test.so) -- TEST HOOKS: the values behind the coarse quantiser's and the k-means assign pass's certificates.
//
// Both certificates rest on E, a bound on |approximate value - reference distance| (gemm.hip.h).  These hooks hand back what the
// kernels actually computed -- the approximate values, the second-best values and tile minima that the assign pass's certificate
// and its tile re-scan decide by, and the E each kernel charged -- so that tests/test_certificate_coarse_assign_gpu.py can hold
// every one of them against the reference's ordered chains.
#include <vector>

#include "../gemm.hip.h"
#include "../ivf_src.hip.h"
#include "../../../include/vers_hip_audit.h"

using namespace vers;

extern "C" {

int32_t vers_ivf_test_last_coarse(vers_ivf_t* h, uint32_t q, float* out_g, uint32_t cap, uint32_t* out_k, double* out_info8) {
  if (!h || !out_k || (cap && !out_g)) return fail(VERS_ERR_INVALID, "bad arguments");
  std::shared_lock<std::shared_mutex> lk(h->index);
  UseLastWs use_ws(h);
  if (!use_ws.ok || !W->last_coarse.valid) return fail(VERS_ERR_INVALID, "vers_ivf_test_last_coarse: no batched search ran the coarse quantiser on the matrix cores");
  const auto lc = W->last_coarse;
  if (q >= lc.b) return fail(VERS_ERR_INVALID, "vers_ivf_test_last_coarse: no such query in the last batch");
  DeviceGuard g(h->device);
  VERS_HIP_TRY(hipDeviceSynchronize());
  const uint32_t k = h->k;
  if (cap) VERS_HIP_TRY(hipMemcpy(out_g, W->gbuf.as<float>() + (uint64_t)q * h->k_pad, (size_t)(cap < k ? cap : k) * 4, hipMemcpyDeviceToHost));
  float qe[2] = {0.0f, 0.0f};
  VERS_HIP_TRY(hipMemcpy(qe, W->coarse_qe.as<float>() + 2 * (uint64_t)q, 8, hipMemcpyDeviceToHost));
  *out_k = k;
  if (out_info8) {
    out_info8[0] = qe[0]; out_info8[1] = lc.cmax2; out_info8[2] = h->ldq; out_info8[3] = h->metric;
    out_info8[4] = lc.x3; out_info8[5] = kX3Slack; out_info8[6] = qe[1]; out_info8[7] = lc.P;
  }
  return VERS_OK;
}

int32_t vers_test_assign_filter(int32_t device, const float* X, uint32_t n, uint32_t ldx, const float* C, uint32_t k, uint32_t ldc, uint32_t d,
                                int32_t metric, uint32_t mode, uint32_t* out_cand, float* out_g2, float* out_e, uint8_t* out_queued, float* out_thr,
                                float* out_part_v1, uint32_t* out_part_c1, float* out_part_v2, uint32_t* out_assign, float* out_mind,
                                uint32_t* out_info10) {
  if (!X || !C || n == 0 || (mode < 4 && n > 131072u) || k < 2 || d == 0 || ldx < d || ldc < d || (ldx | ldc) % 4 || mode > 4 || (metric != 0 && metric != 1) ||
      !out_cand || !out_g2 || !out_queued || !out_thr || !out_part_v1 || !out_part_c1 || !out_part_v2 || !out_assign || !out_mind)
    return fail(VERS_ERR_INVALID, "vers_test_assign_filter: bad arguments (k >= 2; a forced filter: 1 <= n <= 131072 points, one batch)");
  const uint32_t k_pad = round_up(k, kGemmBM), ldq = round_up(d, kColAlign);
  if (mode >= 2 && k_pad % kGemmWide != 0) return fail(VERS_ERR_INVALID, "vers_test_assign_filter: the fp16 single product needs k_pad % 256 == 0");
  if (mode == 3 && !gemm_h_ok(ldq)) return fail(VERS_ERR_INVALID, "vers_test_assign_filter: dist_gemm_h_kernel needs d_pad % 128 == 0");
  DeviceGuard g(device);
  int n_cu = 0;
  VERS_HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
  int32_t rc = VERS_OK;
  {
    KMeansScratch ws;
    AssignProbe pr;
    DevBuf dX, dC, dA, dM, dE;
    if ((rc = dX.reserve((size_t)n * ldx * 4)) || (rc = dC.reserve((size_t)k * ldc * 4)) || (rc = dA.reserve((size_t)n * 4)) ||
        (rc = dM.reserve((size_t)n * 4)) || (rc = dE.reserve((size_t)n * 4)) || (rc = ws.status.reserve(16)))
      return rc;
    VERS_HIP_TRY(hipMemcpy(dX.p, X, (size_t)n * ldx * 4, hipMemcpyHostToDevice));
    VERS_HIP_TRY(hipMemcpy(dC.p, C, (size_t)k * ldc * 4, hipMemcpyHostToDevice));
    VERS_HIP_TRY(hipMemset(ws.status.p, 0, 16));
    VERS_HIP_TRY(hipMemset(dE.p, 0xFF, (size_t)n * 4));  // (NaN: a point whose E was never written fails the test)
    pr.e_dev = dE.as<float>();
    ws.force_filter = mode == 4 ? -1 : (int)mode;
    ws.probe = &pr;
    if ((rc = km_assign_mfma(dX.as<float>(), ldx, n, dC.as<float>(), ldc, k, d, dA.as<uint32_t>(), dM.as<float>(), ws, n_cu, nullptr, metric))) return rc;
    VERS_HIP_TRY(hipDeviceSynchronize());
    if (mode < 4 && pr.batches != 1) return fail(VERS_ERR_INVALID, "vers_test_assign_filter: the pass did not run as one batch");
    VERS_HIP_TRY(hipMemcpy(out_assign, dA.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    VERS_HIP_TRY(hipMemcpy(out_mind, dM.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (out_e) VERS_HIP_TRY(hipMemcpy(out_e, dE.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    uint32_t status = 0;
    VERS_HIP_TRY(hipMemcpy(&status, ws.status.p, 4, hipMemcpyDeviceToHost));
    if (pr.batches == 1) {  // (several batches: the per-batch values are gone)
      memcpy(out_cand, pr.best.data(), (size_t)n * 4);
      memcpy(out_g2, pr.g2.data(), (size_t)n * 4);
      memcpy(out_part_v1, pr.part_v1.data(), pr.part_v1.size() * 4);
      memcpy(out_part_c1, pr.part_c1.data(), pr.part_c1.size() * 4);
      memcpy(out_part_v2, pr.part_v2.data(), pr.part_v2.size() * 4);
    }
    memset(out_queued, 0, n);
    const float nan = __builtin_nanf("");
    for (uint32_t i = 0; i < n; ++i) out_thr[i] = nan;
    for (size_t e = 0; e < pr.queue.size(); ++e) {
      const uint32_t i = pr.queue[e];
      if (i >= n) return fail(VERS_ERR_INVALID, "vers_test_assign_filter: a queue entry out of range");
      out_queued[i] = 1;
      if (e < pr.thr.size()) out_thr[i] = pr.thr[e];
    }
    if (out_info10) {
      const uint32_t info[10] = {(uint32_t)(k_pad / kGemmBM), pr.wide, pr.hi_only, pr.used_h, pr.tile_rescan, (uint32_t)pr.queue.size(), pr.n_full, status,
                                 pr.batches, (uint32_t)mode};
      memcpy(out_info10, info, sizeof(info));
    }
  }
  return rc;
}

}  // extern "C"
