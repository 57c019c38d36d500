// ball_filter.hip.h -- sub-cluster balls of the inverted lists and the kernel that rules cold quads out with them before the int8 head's
// filter reads a byte of their rows.
//
// A cold list is read only to prove that none of its rows passes a threshold.  The head filter (head_filter.hip.h) proves it from 256
// int8 columns of every row; the proof here needs no row at all.  At derive time (ivf_build.hip: build_balls) every list is cut into
// <= kBallMax sub-clusters, each with a centre s_j (fp16), a radius r_j over its shadow rows, the smallest stored |x|^2 m_j and sn_j >=
// |s_j|; ball_lower (prescan.hip.h) bounds the val of every row of the sub-cluster from <s_j, q'> alone.  ball_filter_kernel runs between
// the scan's launch over the hot quads and head_filter_kernel: a block per cold quad computes the dot products of the group's queries
// against the list's centres on the matrix cores, and a quad whose every sub-cluster clears every query's threshold -- as the hot
// launch left it -- gets what the head filter gives a dead quad (kKeyMax in its partial slots, kQuadDead, its tiles counted as
// abandoned).  The quads that survive are appended to a compact list, which head_filter_kernel strides over.  All quads of a (list,
// group) see the same thresholds (the hot launch has finished) and the same centres, so each of them RECOMPUTES the same dot products and
// arrives at the same verdict (about one quad per unit at the flagship shapes; redundant work on lists of many quads).
#pragma once
#include "prescan.hip.h"

namespace vers {

constexpr uint32_t kBallMax = 32;         // sub-clusters per list at most: one M tile of v_mfma_f32_32x32x16_f16
constexpr uint32_t kBallMaxRows = 8192;   // rows of a list the derive pass's LDS arrays hold; a longer list gets no balls
constexpr int kBallDeriveThreads = 256;
constexpr uint32_t kBallSample = 256;     // rows of the strided sample the derive pass tries first
constexpr uint32_t kBallMaxLd = 1856;    // the derive block's centres [kBallMax][ld] fp16 + its row arrays fit the CU's 160 KB of LDS up to here
inline size_t ball_derive_lds_bytes(uint32_t ld) { return (size_t)kBallMaxRows * 5u + (size_t)kBallMax * ld * 2u + (8u + 8u * kBallMax) * 4u; }
static_assert((size_t)kBallMaxRows * 5u + (size_t)kBallMax * kBallMaxLd * 2u + (8u + 8u * kBallMax) * 4u <= 160u * 1024u, "the derive block fits a CU's LDS");

// ---- the derive pass ---------------------------------------------------------------------------------------------------------------------
// 8 columns (group g) of storage row R of the fp16 shadow (rows_to_f16_kernel's layout, prescan.hip.h)
static __device__ __forceinline__ f16x8_t ball_row8(const uint16_t* rows_h, uint32_t ld, uint64_t R, uint32_t g) {
  const uint32_t rr = (uint32_t)(R & 63);
  return *reinterpret_cast<const f16x8_t*>(rows_h + (R >> 6) * 64ull * ld + ((uint64_t)((g >> 1) * 2u + (rr >> 5)) * 64u + (g & 1u) * 32u + (rr & 31u)) * 8u);
}

// A block per list (slot order).  Stored rows [off, off + len) only.  Output: cent [slot * kBallMax + o][ld] fp16, ballf [..][3] = r | m
// (NaN: open) | sn, ball_cnt[slot] = sub-clusters kept (0: no balls for the list).
//   (1) leaders by farthest point (f32 squared distances, running minimum and its leader per row in LDS) until the largest minimum is
//       <= cut2 or kBallMax leaders; the cap reached above the cut: no balls
//   (2) centres = fp16 of the mean of the rows nearest to each leader
//   (3) rows re-assigned to the nearest centre; r_j from f64 sums, rounded up; m_j = min xnorm; empty sub-clusters dropped
// Whatever (1) and (2) find, the bound holds: only r_j and m_j must be true of the final assignment.
static __global__ __launch_bounds__(kBallDeriveThreads) void ball_derive_kernel(const uint16_t* rows_h, uint32_t ld, const uint32_t* slot_off, const uint32_t* slot_len,
                                                                              const float* xnorm, const uint32_t* misc, float cut_rel2, uint16_t* cent, float* ballf,
                                                                              uint32_t* ball_cnt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ball_lds[];
  float* mind = reinterpret_cast<float*>(ball_lds);                                     // [kBallMaxRows]; after (1): the mean's partial sums
  _Float16* cl = reinterpret_cast<_Float16*>(ball_lds + (size_t)kBallMaxRows * 4u);     // [kBallMax][ld]
  uint8_t* lab = ball_lds + (size_t)kBallMaxRows * 4u + (size_t)kBallMax * ld * 2u;     // [kBallMaxRows]
  uint32_t* sm = reinterpret_cast<uint32_t*>(ball_lds + (size_t)kBallMaxRows * 5u + (size_t)kBallMax * ld * 2u);  // 8 + 8 * kBallMax words
  float* red_v = reinterpret_cast<float*>(sm);      // [4] per-wave maxima
  uint32_t* red_i = sm + 4;                         // [4] their rows
  uint32_t* nrow = sm + 8;                          // [kBallMax][4] rows per (sub-cluster, slice of the rows)
  uint32_t* r_bits = sm + 8 + kBallMax * 4u;        // [kBallMax] radius bits
  uint32_t* m_bits = r_bits + kBallMax;             // [kBallMax] min |x|^2 bits
  uint32_t* open_f = m_bits + kBallMax;             // [kBallMax]
  uint32_t* omap = open_f + kBallMax;               // [kBallMax] output index or 0xFFFFFFFF
  const uint32_t L = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const uint32_t len = slot_len[L];
  const uint64_t off = slot_off[L];
  const uint32_t G8 = ld / 8u;
  if (len == 0u || len > kBallMaxRows) {  // (block-uniform)
    if (tid == 0) ball_cnt[L] = 0u;
    return;
  }
  const float cut2 = cut_rel2 * __uint_as_float(misc[0]);  // (cut / 1000)^2 xmax2
  // (1) over the rows 0, stride, 2 stride, ... (n of them) of the list; returns true when the cap was reached above the cut
  uint32_t k = 0;
  auto leaders = [&](uint32_t n, uint32_t stride) {
  __syncthreads();
  for (uint32_t i = tid; i < n; i += kBallDeriveThreads) { mind[i] = __builtin_inff(); lab[i] = 0; }
  uint32_t leader = 0;
  bool capped = false;
  for (uint32_t it = 0; it < kBallMax; ++it) {
    __syncthreads();
    for (uint32_t g = tid; g < G8; g += kBallDeriveThreads) *reinterpret_cast<f16x8_t*>(cl + (size_t)it * ld + 8u * g) = ball_row8(rows_h, ld, off + (uint64_t)leader * stride, g);
    __syncthreads();
    float best = -1.0f;
    uint32_t best_i = 0;
    for (uint32_t i = tid; i < n; i += kBallDeriveThreads) {
      float d2 = 0.0f;
      for (uint32_t g = 0; g < G8; ++g) {
        const f16x8_t x = ball_row8(rows_h, ld, off + (uint64_t)i * stride, g);
        const f16x8_t c = *reinterpret_cast<const f16x8_t*>(cl + (size_t)it * ld + 8u * g);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float dl = (float)x[e] - (float)c[e];
          d2 += dl * dl;
        }
      }
      if (!(d2 == d2)) d2 = 0.0f;  // (a NaN row stays where it is: its |x|^2 is not finite and its sub-cluster is open)
      float mi = mind[i];
      if (d2 < mi) { mi = d2; mind[i] = d2; lab[i] = (uint8_t)it; }
      if (mi > best) { best = mi; best_i = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, kWave);
      const uint32_t oi = (uint32_t)__shfl_xor((int)best_i, o, kWave);
      if (ov > best || (ov == best && oi < best_i)) { best = ov; best_i = oi; }
    }
    if (lane == 0) { red_v[wid] = best; red_i[wid] = best_i; }
    __syncthreads();
    best = red_v[0]; best_i = red_i[0];
    for (int w = 1; w < kBallDeriveThreads / 64; ++w)
      if (red_v[w] > best || (red_v[w] == best && red_i[w] < best_i)) { best = red_v[w]; best_i = red_i[w]; }
    k = it + 1u;
    if (!(best > cut2)) break;  // (block-uniform: every thread read the same four words)
    if (k == kBallMax) capped = true;
    leader = best_i;
  }
  return capped;
  };
  // A strided sample of kBallSample rows first: where already the sample needs more than kBallMax leaders above the cut -- rows without
  // cluster contrast -- the list gets no balls for a tenth of the full pass's reads.  (A choice of which lists get balls, not a proof
  // about the full list; either answer is sound.)
  bool capped = len > 2u * kBallSample && leaders(kBallSample, len / kBallSample);
  if (!capped) capped = leaders(len, 1u);
  if (capped) {  // (block-uniform) rows without contrast at this cut: the head filter handles the list as before
    if (tid == 0) ball_cnt[L] = 0u;
    return;
  }
  __syncthreads();
  // (2) thread = (8-column group, slice of the rows); the partial sums go where the minima were
  const uint32_t n_slice = G8 <= 64u ? 4u : (G8 <= 128u ? 2u : 1u);  // n_slice * G8 <= 256 threads; n_slice * ld <= kBallMaxRows floats
  float* psum = mind;
  for (uint32_t j = 0; j < k; ++j) {
    {
      const uint32_t g = tid % (kBallDeriveThreads / n_slice), sl = tid / (kBallDeriveThreads / n_slice);  // (G8 <= 256 / n_slice)
      float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      uint32_t cntj = 0;
      if (g < G8 && sl < n_slice)
        for (uint32_t i = sl; i < len; i += n_slice)
          if (lab[i] == (uint8_t)j) {
            const f16x8_t x = ball_row8(rows_h, ld, off + i, g);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += (float)x[e];
            ++cntj;
          }
      if (g < G8 && sl < n_slice) {
#pragma unroll
        for (int e = 0; e < 8; ++e) psum[(size_t)sl * ld + 8u * g + e] = acc[e];
        if (g == 0u) nrow[j * 4u + sl] = cntj;
      }
    }
    __syncthreads();
    uint32_t nj = 0;
    for (uint32_t s = 0; s < n_slice; ++s) nj += nrow[j * 4u + s];
    if (nj != 0u)  // (block-uniform; a leader that lost every row to an equal earlier one keeps its own row as centre and is dropped below)
      for (uint32_t c = tid; c < ld; c += kBallDeriveThreads) {
        float t = 0.0f;
        for (uint32_t s = 0; s < n_slice; ++s) t += psum[(size_t)s * ld + c];
        cl[(size_t)j * ld + c] = (_Float16)(t / (float)nj);
      }
    __syncthreads();
  }
  // (3) nearest centre per row in ONE pass over the rows: k running sums per thread
  if (tid < kBallMax) { r_bits[tid] = 0u; m_bits[tid] = 0x7F800000u; open_f[tid] = 0u; nrow[tid * 4u] = 0u; }
  __syncthreads();
  for (uint32_t i = tid; i < len; i += kBallDeriveThreads) {
    float d2[kBallMax];
#pragma unroll
    for (uint32_t j = 0; j < kBallMax; ++j) d2[j] = 0.0f;
    for (uint32_t g = 0; g < G8; ++g) {
      const f16x8_t x = ball_row8(rows_h, ld, off + i, g);
      float xf[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) xf[e] = (float)x[e];
#pragma unroll
      for (uint32_t j = 0; j < kBallMax; ++j)
        if (j < k) {  // (block-uniform)
          const f16x8_t c = *reinterpret_cast<const f16x8_t*>(cl + (size_t)j * ld + 8u * g);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float dl = xf[e] - (float)c[e];
            d2[j] += dl * dl;
          }
        }
    }
    uint32_t bj = 0;
    float bd = d2[0];
#pragma unroll
    for (uint32_t j = 1; j < kBallMax; ++j)
      if (j < k && d2[j] < bd) { bd = d2[j]; bj = j; }
    lab[i] = (uint8_t)bj;
    // the radius of the final assignment: f64 over the exact fp16 differences, rounded up
    double acc = 0.0;
    for (uint32_t g = 0; g < G8; ++g) {
      const f16x8_t x = ball_row8(rows_h, ld, off + i, g);
      const f16x8_t c = *reinterpret_cast<const f16x8_t*>(cl + (size_t)bj * ld + 8u * g);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const double dl = (double)(float)x[e] - (double)(float)c[e];
        acc += dl * dl;
      }
    }
    const float rr = prune_round_up(__builtin_sqrt(acc * (1.0 + 1e-12)) * (1.0 + 1e-12));
    const float xn = xnorm[off + i];
    if (rr >= 0.0f && rr < __builtin_inff() && xn >= 0.0f && xn < __builtin_inff()) {
      atomicMax(&r_bits[bj], __float_as_uint(rr));  // >= 0: bit order == value order
      atomicMin(&m_bits[bj], __float_as_uint(xn));
    } else {
      atomicOr(&open_f[bj], 1u);
    }
    atomicAdd(&nrow[bj * 4u], 1u);
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t o = 0;
    for (uint32_t j = 0; j < k; ++j) omap[j] = nrow[j * 4u] != 0u ? o++ : 0xFFFFFFFFu;
    ball_cnt[L] = o;
  }
  __syncthreads();
  for (uint32_t j = (uint32_t)wid; j < k; j += kBallDeriveThreads / 64) {  // a wave per sub-cluster: |s_j| in f64, the centre's row, its three floats
    const uint32_t o = omap[j];
    if (o == 0xFFFFFFFFu) continue;  // (wave-uniform)
    double s2 = 0.0;
    uint16_t* dst = cent + ((uint64_t)L * kBallMax + o) * ld;
    for (uint32_t c = (uint32_t)lane; c < ld; c += 64u) {
      const _Float16 v = cl[(size_t)j * ld + c];
      s2 += (double)(float)v * (double)(float)v;
      dst[c] = __builtin_bit_cast(uint16_t, v);
    }
#pragma unroll
    for (int of = 32; of > 0; of >>= 1) s2 += __shfl_xor(s2, of, kWave);
    if (lane == 0) {
      float* f = ballf + ((uint64_t)L * kBallMax + o) * 3u;
      f[0] = __uint_as_float(r_bits[j]);
      f[1] = open_f[j] != 0u ? __builtin_nanf("") : __uint_as_float(m_bits[j]);
      f[2] = prune_round_up(__builtin_sqrt(s2) * (1.0 + 1e-12));
    }
  }
}

// The derive pass writes at the cap (kBallMax places per list); this packs what it kept: cent [ball_off[slot] + j][ld], ballf likewise.
// A block per list slot.
static __global__ __launch_bounds__(256) void ball_pack_kernel(const uint16_t* cent_cap, const float* ballf_cap, const uint32_t* ball_cnt, const uint32_t* ball_off,
                                                             uint32_t ld, uint16_t* cent, float* ballf) {
  const uint32_t L = blockIdx.x, n = ball_cnt[L] < kBallMax ? ball_cnt[L] : kBallMax;
  const uint64_t o = ball_off[L];
  const u32x4* src = reinterpret_cast<const u32x4*>(cent_cap + (uint64_t)L * kBallMax * ld);
  u32x4* dst = reinterpret_cast<u32x4*>(cent + o * ld);
  for (uint32_t i = threadIdx.x; i < n * (ld / 8u); i += blockDim.x) dst[i] = src[i];  // (ld is a multiple of 64: rows are whole 16-byte pieces)
  for (uint32_t i = threadIdx.x; i < n * 3u; i += blockDim.x) ballf[o * 3u + i] = ballf_cap[(uint64_t)L * kBallMax * 3u + i];
}

// ---- the filter --------------------------------------------------------------------------------------------------------------------------
struct BallParams {
  const uint16_t* cent;      // [ball_off[slot] + j][ld] fp16 centres
  const float* ballf;        // [ball_off[slot] + j][3] r | m (NaN: open) | sn
  const uint32_t* ball_off;  // [slot] the list's first sub-cluster
  const uint32_t* ball_cnt;  // [slot] sub-clusters of the list (0: none)
  const uint16_t* qh16;      // [b][ld] q' = fp16(-2 q) (prune_table_kernel)
  const float* qball;        // [b][2] ball_bracket | nq'
  const uint32_t* bounds32;
  uint32_t ld, kp, n_steps;
  uint32_t min_quads;        // the pass engages when the cold region has at least so many quads; below: the survivor list is the identity
  uint32_t* surv;            // the cold quads left for the head filter, in any order
  uint32_t* n_surv;          // how many (zeroed with the planning tables)
  uint32_t* last;            // [2] units (list, group) tested | dead, this launch (zeroed with the planning tables)
  unsigned long long* tot;   // [2] the same over the handle's life
  // a quad ruled out here counts where one ruled out by the head filter counts (HeadParams::last / tot: quads tested | dead; PreParams'
  // steps without math | tiles abandoned); the quads left are counted as tested by the head filter itself
  uint32_t* head_last;
  unsigned long long* head_tot;
  uint32_t* prune_last;
  unsigned long long* prune_tot;
};
constexpr int kBallWaves = 4;

template <int NQ, class Src>
__global__ __launch_bounds__(kWave * kBallWaves) void ball_filter_kernel(Src src, BallParams bp) {
  constexpr int NT = NQ > 32 ? 2 : 1;     // query tiles of 32
  constexpr int KS = kBallWaves / NT;     // waves that share a query tile: each takes a contiguous share of the columns
  __shared__ float dsum[KS][NT * 32][kBallMax + 1];
  __shared__ uint32_t pair_l[NT * 32], qix_l[NT * 32];
  __shared__ float thr_l[NT * 32], br_l[NT * 32], nq_l[NT * 32];
  __shared__ uint32_t live_flag, tiles_l, ctr_l[4];  // ctr_l: units tested | units dead | quads dead | their tiles
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t n_quads = src.n_items() / 4u;
  const uint32_t hot_quads = src.hot_items() / 4u < n_quads ? src.hot_items() / 4u : n_quads;
  const uint32_t n_cold = n_quads - hot_quads;
  if (n_cold < bp.min_quads) {  // (kernel-uniform) the head filter would be a single round of blocks: the list is the identity
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_cold; i += gridDim.x * blockDim.x) bp.surv[i] = hot_quads + i;
    if (blockIdx.x == 0 && threadIdx.x == 0) *bp.n_surv = n_cold;
    return;
  }
  if (threadIdx.x < 4) ctr_l[threadIdx.x] = 0u;
  const uint32_t ld = bp.ld;
  for (uint32_t i = blockIdx.x; i < n_cold; i += gridDim.x) {
    const uint32_t bi = hot_quads + i;
    __syncthreads();  // the previous quad's operands and verdict are done with
    const ItemDesc d0 = src.items[4 * bi];
    const uint32_t c0 = src.cnt[d0.list] - d0.group * (uint32_t)NQ;
    const uint32_t nq = c0 < (uint32_t)NQ ? c0 : (uint32_t)NQ;
    const uint32_t kc = bp.ball_cnt[d0.list] < kBallMax ? bp.ball_cnt[d0.list] : kBallMax;
    const uint64_t b0 = bp.ball_off[d0.list];
    if (threadIdx.x == 0) { live_flag = kc == 0u ? 1u : 0u; tiles_l = 0u; }
    __syncthreads();
    if (threadIdx.x < nq) {
      const uint32_t pr = src.pair_of(4 * bi, (int)threadIdx.x);
      const uint32_t qix = pr / src.P;
      pair_l[threadIdx.x] = pr;
      qix_l[threadIdx.x] = qix;
      const uint32_t b32 = __hip_atomic_load(bp.bounds32 + src.slot_of_pair(pr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const float thr = b32 == 0xFFFFFFFFu ? __builtin_inff() : __uint_as_float(order_bits_to_f32_bits(b32));
      thr_l[threadIdx.x] = thr;
      br_l[threadIdx.x] = bp.qball[2u * qix];
      nq_l[threadIdx.x] = bp.qball[2u * qix + 1u];
      if (!(thr < __builtin_inff())) live_flag = 1u;  // (no threshold yet, or a NaN: nothing can be ruled out for this query)
    }
    __syncthreads();
    const bool dots = live_flag == 0u;  // (block-uniform)
    if (dots) {
      const int nt = wid % NT, ks = wid / NT;
      if ((uint32_t)(nt * 32) < nq) {  // (wave-uniform)
        const uint32_t n = (uint32_t)(lane & 31), kq = (uint32_t)(lane >> 5);
        const uint32_t jc = n < kc ? n : kc - 1u;  // (rows beyond the list's centres repeat the last one: their results are not read)
        const uint32_t qs = (uint32_t)(nt * 32) + n < nq ? (uint32_t)(nt * 32) + n : nq - 1u;
        const uint16_t* ap = bp.cent + (b0 + jc) * ld + 8u * kq;
        const uint16_t* bq = bp.qh16 + (uint64_t)qix_l[qs] * ld + 8u * kq;
        const uint32_t steps = ld / 16u / (uint32_t)KS;  // (ld is a multiple of 64)
        const uint32_t s0 = (uint32_t)ks * steps;
        f32x16_t acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
#pragma unroll 4
        for (uint32_t s = 0; s < steps; ++s) {
          const f16x8_t a = *reinterpret_cast<const f16x8_t*>(ap + (size_t)(s0 + s) * 16u);
          const f16x8_t b = *reinterpret_cast<const f16x8_t*>(bq + (size_t)(s0 + s) * 16u);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
        }
        // the lane's query column n of the tile, centres 8 (e >> 2) + 4 (lane >> 5) + (e & 3)
#pragma unroll
        for (int e = 0; e < 16; ++e) dsum[ks][nt * 32 + (int)n][8 * (e >> 2) + 4 * (int)kq + (e & 3)] = acc[e];
      }
      __syncthreads();
      if (threadIdx.x < nq) {
        const float thr = thr_l[threadIdx.x], br = br_l[threadIdx.x], nqp = nq_l[threadIdx.x];
        const float* f = bp.ballf + b0 * 3u;
        bool keep = false;
        for (uint32_t j = 0; j < kc; ++j) {
          float D = dsum[0][threadIdx.x][j];
#pragma unroll
          for (int s = 1; s < KS; ++s) D += dsum[s][threadIdx.x][j];
          keep |= !(ball_lower(f[3u * j + 1u], D, f[3u * j], f[3u * j + 2u], nqp, br, ld) > (double)thr);
        }
        if (keep) live_flag = 1u;
      }
    }
    if (threadIdx.x < 4) {  // the quad's tiles, by the source's own rule
      uint32_t row_s, nrows;
      src.seg_span(src.items[4 * bi + threadIdx.x], row_s, nrows);
      atomicAdd(&tiles_l, (nrows + kWave - 1) / kWave);
    }
    __syncthreads();
    const bool unit = (d0.seg >> 2) == 0u;  // the first quad of its (list, group) counts the unit
    if (live_flag == 0u) {  // (block-uniform) every sub-cluster of the list is ruled out for every query of the group
      const uint32_t kp = bp.kp;
      for (uint32_t e = threadIdx.x; e < nq * kp; e += kWave * kBallWaves) {
        const uint32_t qi = e / kp, x = e - qi * kp;
        (src.partials + ((uint64_t)pair_l[qi] * src.S_max + (d0.seg >> 2)) * src.k_keep)[x] = kKeyMax;  // (= src.out_quad(4 * bi, qi)[x])
      }
      if (threadIdx.x == 0) {
        const_cast<ItemDesc*>(src.items)[4 * bi].group = d0.group | kQuadDead;
        ctr_l[1] += unit ? 1u : 0u;
        ctr_l[2] += 1u;
        ctr_l[3] += tiles_l;
      }
    } else if (threadIdx.x == 0) {
      bp.surv[atomicAdd(bp.n_surv, 1u)] = bi;
    }
    if (threadIdx.x == 0 && unit) ctr_l[0] += 1u;
  }
  __syncthreads();
  if (threadIdx.x < 2 && ctr_l[threadIdx.x] != 0u) {
    atomicAdd(bp.last + threadIdx.x, ctr_l[threadIdx.x]);
    atomicAdd(bp.tot + threadIdx.x, (unsigned long long)ctr_l[threadIdx.x]);
  }
  if (threadIdx.x == 0 && ctr_l[2] != 0u) {  // as head_filter_kernel counts the quads it rules out
    atomicAdd(bp.head_last, ctr_l[2]);
    atomicAdd(bp.head_last + 1, ctr_l[2]);
    atomicAdd(bp.head_tot, (unsigned long long)ctr_l[2]);
    atomicAdd(bp.head_tot + 1, (unsigned long long)ctr_l[2]);
    atomicAdd(bp.prune_last + 1, ctr_l[3] * bp.n_steps);
    atomicAdd(bp.prune_last + 2, ctr_l[3]);
    atomicAdd(bp.prune_tot + 1, (unsigned long long)ctr_l[3] * bp.n_steps);
    atomicAdd(bp.prune_tot + 2, (unsigned long long)ctr_l[3]);
  }
}

}  // namespace vers
