/* vers_hip_audit.h -- TEST HOOKS that audit the coarse quantiser's and the k-means assign pass's certificates value by value
 * (tests/test_certificate_coarse_assign_gpu.py), and the flat corpus' single query on its fp16 shadow
 * (tests/test_certificate_single_gpu.py).  Like include/vers_hip_test.h's hooks they live in libvers_hip_test.so, which
 * links against libvers_hip.so and takes its handles; the product library exports none of them (tests/test_abi.py). */
#ifndef VERS_HIP_AUDIT_H
#define VERS_HIP_AUDIT_H
#include "vers_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* TEST HOOK: the coarse quantiser of the most recent batched search on this handle, if it ran on the matrix cores: query q's approximate
 * row G[0..k) (|c|^2 - 2 <q, c>, or -<q, c> for the cosine distance) as the selection read it (up to cap values), *out_k = k.
 * out_info8: |q|^2 and E as the selection kernel computed them ([0], [6]), the max |c|^2 it charged, d_pad, metric, 1 if the contraction
 * was bf16x3 (0: f32), the slack constant charged for bf16x3 (gemm.hip.h kX3Slack), P.  The certificate holds if | G + |q|^2 - D_ref | <= E
 * (cosine: | 1 + G - D_ref | <= E) for every centroid. */
int32_t vers_ivf_test_last_coarse(vers_ivf_t* h, uint32_t q, float* out_g, uint32_t cap, uint32_t* out_k, double* out_info8);
/* TEST HOOK: one batch (n <= 131072) of the matrix-core k-means assign pass with its own scratch, the filter forced by `mode`: 0 the f32
 * MFMA, 1 bf16x3, 2 one fp16 product by the register-staged wide kernel, 3 one fp16 product by the LDS-DMA kernel (2, 3: k rounded up to
 * 128 must be a multiple of 256; 3: d rounded up to 64 a multiple of 128), 4 whatever the options pick (any n; several batches leave the
 * per-batch values -- candidate, g2, the triples -- unwritten).  X [n][ldx], C [k][ldc] host rows (ldx, ldc multiples of 4,
 * padding columns zero).  Per point: the candidate and the second-smallest approximate value g2 (assign_argmin_merge_kernel), the E
 * assign_rescore_kernel charged (out_e nullable), queued = 1 if the certificate left it open, fb_thr (NaN unless queued for the tile
 * re-scan); per (tile of 128 centroids, point), [n_tiles][n]: the tile's smallest value, its centroid, the second smallest; the final
 * assignment and minimum distance.  out_info10: n_tiles, wide kernel, single fp16 product, LDS-DMA kernel, tile re-scan (of the last
 * batch), points queued, points sent to the full exact scan, status word, batches, mode. */
int32_t vers_test_assign_filter(int32_t device, const float* X, uint32_t n, uint32_t ldx, const float* C, uint32_t k, uint32_t ldc, uint32_t d,
                                int32_t metric, uint32_t mode, uint32_t* out_cand, float* out_g2, float* out_e, uint8_t* out_queued, float* out_thr,
                                float* out_part_v1, uint32_t* out_part_c1, float* out_part_v2, uint32_t* out_assign, float* out_mind,
                                uint32_t* out_info10);
/* TEST HOOK: the fp16 shadow a flat handle's single queries stream (flat1h_kernel), as the device holds it.  out_state8: [0] 1 if the
 * shadow is present (derived from all n rows), 0 if the f32 scan is in charge (no memory for it, an element overflows fp16, n == 0,
 * option "shadow" = 0); [1] partial slots; [2] max |x|^2 and [3] R^2 = max |x - fp16(x)|^2 over the rows, the f32 values widened; [4] the
 * running count of single queries whose certificate failed since the upload; [5] ld; [6] n; [7] rows the shadow was derived from.
 * [1] .. [4] are 0 while the shadow is absent. */
int32_t vers_flat_test_shadow_state(vers_flat_t* h, double* out_state8);
/* TEST HOOK: the raw pre-filter values of the most recent single-query search on this handle, which must have run on the shadow with
 * this top_k (and `query`, `metric`): every non-empty key of the scan's partial slots (kp = min(64, top_k + max(24, top_k)) keys per slot)
 * as (row = vec id, val exactly as the certificate saw it, the bound the certificate charges that candidate), with the conventions of
 * vers_ivf_test_last_vals (include/vers_hip_test.h): | val + |q|^2 - D_ref | <= bound (cosine: | 1 + val - D_ref |).  |q|^2 is summed
 * here in double from `query` (d host floats).  out_info8: |q|^2, max |x|^2, R^2, the bound for rows outside the slots, its
 * candidate-independent part, kp, 1 (the shadow code charged), metric.  *out_n = values available (may exceed cap).  VERS_ERR_INVALID
 * if a single query with this top_k would not take the shadow on this handle. */
int32_t vers_flat_test_last_vals(vers_flat_t* h, const float* query, uint32_t top_k, uint32_t metric, uint64_t* out_vec_ids, float* out_vals,
                                 double* out_bound, uint32_t cap, uint32_t* out_n, double* out_info8);
#ifdef __cplusplus
}
#endif
#endif /* VERS_HIP_AUDIT_H */
