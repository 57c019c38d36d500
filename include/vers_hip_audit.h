/* vers_hip_audit.h -- TEST HOOKS that audit the coarse quantiser's and the k-means assign pass's certificates value by value
 * (tests/test_certificate_coarse_assign_gpu.py).  Like include/vers_hip_test.h's hooks they live in libvers_hip_test.so, which
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
#ifdef __cplusplus
}
#endif
#endif /* VERS_HIP_AUDIT_H */
