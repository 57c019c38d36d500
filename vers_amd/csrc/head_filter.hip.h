// head_filter.hip.h -- the int8 head of the stored rows and the kernel that rules cold quads out with it before the list scan streams them.
//
// A cold tile (a list that is no query's nearest) is read by prescan_kernel_g only to prove that none of its rows passes a threshold:
// val ~ +1 against thresholds of ~ -0.6.  That proof needs little precision.  rows_h8 holds an int8 copy of the first H columns of every
// storage row (one scale for the whole index), in 64-row tiles like the shadow; a tile's head is contiguous and cut into 1 KiB pieces of
// 32 rows x 32 columns in the A-operand layout of v_mfma_i32_32x32x32_i8: piece (cb, h) = cb * 2 + h, lane l holds the 16 columns
// 32 cb + 16 (l >> 5) ... + 15 of row 32 h + (l & 31), so that one 16-byte load per lane feeds one MFMA.  A 64-column step is 4 KiB.
//
// head_filter_kernel runs between the scan's launch over the hot quads and its launch over the cold ones: a block per cold quad, a wave
// per segment.  From boundary 256 on, at every 64-column boundary, a wave tests head_lower (prescan.hip.h) for every live query column
// against the query's threshold as the hot lists left it; a tile is dead at the first boundary where all columns pass, a tile that is not
// dead by H makes the quad live and the block stops reading.  A quad whose tiles are all dead gets kKeyMax in its partial slots -- what
// write_out leaves for the later quads of a run -- and the mark the cold launch skips it by (kQuadDead).  Dropping a dead quad drops only
// rows whose val exceeds a threshold fold would have compared them with: the results stay bit-identical.
//
// Nearly every tile is decided at the first boundary, so a wave treats the first 256 columns of its segment's tiles as ONE stream and keeps
// a ring of kHeadRing 4 KiB steps of it in flight across tile ends and verdicts; its next segment's first loads go out before the barriers
// of the quad change (scripts/probe/head_stream_probe.hip).
#pragma once
#include "prescan.hip.h"

namespace vers {

typedef __attribute__((ext_vector_type(4))) int i32x4_t;
typedef __attribute__((ext_vector_type(16))) int i32x16_t;

constexpr uint32_t kHeadMinCols = 256, kHeadMaxCols = 512;  // H: a multiple of 64 in this range (the first test is at 256 columns)
constexpr uint32_t kHeadFirst = kHeadPrefix;                // the first boundary a wave tests at (prescan.hip.h: the prefix of the stream)
static_assert(kHeadFirst * 64u == kHeadMinCols, "the first test is at the smallest head");
constexpr uint32_t kHeadBnd = kHeadMaxCols / 64u - kHeadFirst + 1u;  // boundaries tested at most
constexpr int kHeadWaves = 4;                               // a wave per segment of the quad
// slots of the ring a wave keeps ahead in its stream of tile prefixes (head_stream_pos, prescan.hip.h): 2 or 4 -- a divisor of the prefix,
// so that the slot of a tile's step s is the constant s % kHeadRing.  scripts/probe/head_stream_probe.hip: 4 streams fastest.
constexpr int kHeadRing = 4;
static_assert(kHeadPrefix % kHeadRing == 0,"the ring's slots are indexed by the step within a tile's prefix");
template <int N, class F>
static __device__ __forceinline__ void head_static_for(F&& f) {  // f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>)
  if constexpr (N > 0) {
    head_static_for<N - 1>(f);
    f(std::integral_constant<int, N - 1>{});
  }
}

// ---- the derive pass (ivf_build.hip: build_head) ---------------------------------------------------------------------------------------
// element (r, c) of the blocked f32 rows as the shadow holds it: fp16, round to nearest even
static __device__ __forceinline__ float head_src(const float* rows, uint32_t ld, uint64_t r, uint32_t c) {
  return (float)(_Float16)rows[(r >> 6) * 64ull * ld + ((uint64_t)(c >> 2) * 64 + (r & 63)) * 4 + (c & 3)];
}
// max |x~| over the head columns of the stored rows (thread per row; a NaN is skipped here: its row's |x|^2 is not finite and its tile is never ruled out)
static __global__ void head_max_kernel(const float* rows, uint32_t ld, const uint32_t* row_ids, uint64_t n_rows, uint32_t H, uint32_t* max_bits) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  float m = 0.0f;
  if (r < n_rows && row_ids[r] != 0xFFFFFFFFu)
    for (uint32_t c = 0; c < H; ++c) {
      const float a = __builtin_fabsf(head_src(rows, ld, r, c));
      m = a > m ? a : m;
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(m, off, kWave);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0 && m > 0.0f) atomicMax(max_bits, __float_as_uint(m));  // m >= 0: bit order == value order
}
// the head itself (thread = row x 16 columns: one 16-byte piece entry) and nothing else; a storage row without a vector gets zeros
static __global__ void head_write_kernel(const float* rows, uint32_t ld, const uint32_t* row_ids, uint64_t n_rows, uint32_t H, const uint32_t* max_bits,
                                         int8_t* rows_h8) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t ch = H / 16u;
  const uint64_t r = t % n_rows;  // (consecutive threads: consecutive rows of one chunk -- the f32 loads and the 16-byte stores both coalesce)
  const uint32_t j = (uint32_t)(t / n_rows);
  if (j >= ch) return;
  const float sx = head_scale(__uint_as_float(*max_bits));
  const bool holds = row_ids[r] != 0xFFFFFFFFu;
  uint32_t w[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    uint32_t pk = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int32_t X = holds ? head_quant(head_src(rows, ld, r, 16u * j + 4u * u + e), sx) : 0;
      pk |= ((uint32_t)X & 0xFFu) << (8 * e);
    }
    w[u] = pk;
  }
  const uint32_t rr = (uint32_t)(r & 63);
  int8_t* dst = rows_h8 + (r >> 6) * 64ull * H + ((uint64_t)((j >> 1) * 2u + (rr >> 5)) * 64u + (j & 1u) * 32u + (rr & 31u)) * 16u;
  *reinterpret_cast<u32x4*>(dst) = u32x4{w[0], w[1], w[2], w[3]};
}
// Rh2 = max over the stored rows of sum over the head columns of (x~ - s_x X)^2 (thread per row, f64 sum, rounded UP to f32).  A row with a
// NaN is skipped like above; an infinite element makes s_x infinite and the head invalid.
static __global__ void head_resid_kernel(const float* rows, uint32_t ld, const uint32_t* row_ids, uint64_t n_rows, uint32_t H, const uint32_t* max_bits,
                                         uint32_t* rh2_bits) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows || row_ids[r] == 0xFFFFFFFFu) return;
  const float sx = head_scale(__uint_as_float(*max_bits));
  double acc = 0.0;
  for (uint32_t c = 0; c < H; ++c) {
    const float v = head_src(rows, ld, r, c);
    const double e = head_resid(v, sx, head_quant(v, sx));
    acc += e * e;
  }
  const float f = prune_round_up(acc * (1.0 + 1e-12));
  if (f == f) atomicMax(rh2_bits, __float_as_uint(f));  // f >= 0
}

// ---- the filter ------------------------------------------------------------------------------------------------------------------------
struct HeadParams {
  const int8_t* rows_h8;    // the head: [tile][H / 32][2][64 lanes] x 16 bytes
  const int8_t* q8;         // [b][H] the queries' int8 rows (prune_table_kernel)
  const float* qhead;       // [b][2] head_extra | s_n
  const float* prune_tab;   // [b][n_steps] prune_tail_entry per boundary
  const float* xnorm;
  const uint32_t* bounds32;
  const uint32_t* misc;     // pre_misc of the handle (kHeadMiscMax, kHeadMiscRh2)
  uint32_t H, n_steps, kp;
  float om;                 // 1 - eps of prune_lower
  uint32_t* last;           // [3] quads tested | quads dead | head steps read, this launch (zeroed with the planning tables)
  unsigned long long* tot;  // [3] the same over the handle's life
  // a quad ruled out is so many tiles the scan abandons before their first step: counted where the early abandon counts (PreParams)
  uint32_t* prune_last;           // [3] steps executed | steps without math | tiles abandoned
  unsigned long long* prune_tot;
  uint32_t* done;           // blocks that have added their counters (zeroed with `last`)
  uint32_t* watch;          // pinned: <- 1 by the launch's last block when fewer than 1/8 of the tested quads died (vers_ivf::head_watch)
  // the cold quads the ball filter left (ball_filter.hip.h), in any order, and how many; nullptr: every cold quad, hot_quads + i.  The quads
  // that filter ruled out are in `last` / `tot` already (tested and dead): the back-off goes by the merged counts
  const uint32_t* surv;
  const uint32_t* n_surv;
};
constexpr uint32_t kHeadBackoff = 64;  // batches the split scan sits out after such a launch

template <int NQ, class Src>
__global__ __launch_bounds__(kWave * kHeadWaves) __attribute__((amdgpu_waves_per_eu(2, 2))) void head_filter_kernel(Src src, HeadParams hp) {
  __shared__ __attribute__((aligned(16))) int8_t qb[(size_t)kPreQWide * kHeadMaxCols];  // B operands: [16-column chunk][NQ slots] x 16 bytes
  __shared__ uint32_t pair_l[kPreQWide], qix_l[kPreQWide];
  __shared__ float thr_l[kPreQWide], sn_l[kPreQWide], brk_l[kPreQWide][kHeadBnd];
  __shared__ uint32_t live_flag, tiles_l, ctr_l[4];  // ctr_l[3]: tiles of the quads ruled out
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t H = hp.H, hs = H / 64u, ch = H / 16u;
  const uint32_t n_quads = src.n_items() / 4u;
  const uint32_t hot_quads = src.hot_items() / 4u < n_quads ? src.hot_items() / 4u : n_quads;
  const float sx = head_scale(__uint_as_float(hp.misc[kHeadMiscMax]));
  const double Rh2 = (double)__uint_as_float(hp.misc[kHeadMiscRh2]);
  if (threadIdx.x < 4) ctr_l[threadIdx.x] = 0u;
  uint32_t steps_read = 0;  // (wave-uniform) 4 KiB steps requested, those dropped at a live verdict included
  // The wave's segment and its ring.  The first kHeadFirst steps of the segment's tiles are one stream (head_stream_pos); slot s % R holds
  // step s of the current tile and is issued again -- R positions on, usually the next tile's -- as soon as the step's math has read it, so
  // that loads stay in flight through a tile's last math, its verdict and into the next tile.  Only the slot of the prefix's LAST step
  // waits for the verdict: the steps a tile that survives the first test reads on demand go through it, and the given-up tile's own later
  // steps are never in flight.  Every load of the ring is unconditional; a position past the segment's end re-reads its last step.
  constexpr int R = kHeadRing, kLastSlot = (int)(kHeadFirst - 1u) % R;
  u32x4 ring[R][4];
  uint32_t n_tiles = 0, nrows = 0, row_s = 0;  // (wave-uniform)
  const u32x4* sp = nullptr;                   // the segment's head (+ lane)
  float xn_next = 0.0f;                        // |x|^2 of the lane's row of the tile the ring is about to reach
  auto issue = [&](auto stag, uint32_t p) {    // stream position p of the segment (n_tiles != 0) -> slot
    constexpr int sl = decltype(stag)::value;
    const HeadStreamPos at = head_stream_pos(p, n_tiles);
    const u32x4* a = sp + ((size_t)at.tile * hs + at.step) * 256u;
#pragma unroll
    for (int i = 0; i < 4; ++i) ring[sl][i] = __builtin_nontemporal_load(a + (size_t)i * 64u);
    steps_read += p < head_stream_len(n_tiles) ? 1u : 0u;
  };
  // a segment's rows from its descriptor, by the source's own rule (Src::seg_span, storage_row); a quad beyond the launch's: no tiles
  auto item_of = [&](uint32_t bi) { return bi < n_quads ? src.items[4 * bi + (uint32_t)wid] : ItemDesc{0u, 0u, kNoSeg}; };
  // the block's i-th quad: through the survivor list where there is one (one more indexed load, requested a quad ahead of its descriptor)
  const uint32_t* const surv = hp.surv;
  const uint32_t n_cold = surv != nullptr ? *hp.n_surv : n_quads - hot_quads;
  auto quad_at = [&](uint32_t i) { return i < n_cold ? (surv != nullptr ? surv[i] : hot_quads + i) : 0xFFFFFFFFu; };
  uint32_t q_cur = quad_at(blockIdx.x), q_nx = quad_at(blockIdx.x + gridDim.x);
  struct Seg { uint32_t nrows, row_s; };
  auto resolve = [&](const ItemDesc& d) {
    Seg sg;
    src.seg_span(d, sg.row_s, sg.nrows);
    return sg;
  };
  auto enter = [&](const Seg& sg) {  // make the segment the wave's own; its first R loads go out
    nrows = sg.nrows;
    row_s = sg.row_s;
    n_tiles = (nrows + kWave - 1) / kWave;
    sp = reinterpret_cast<const u32x4*>(hp.rows_h8 + (uint64_t)row_s * H) + lane;
    if (head_stream_len(n_tiles) != 0u) {  // (a segment without tiles has no position: nothing is issued)
      xn_next = hp.xnorm[(uint64_t)row_s + lane];
      head_static_for<R>([&](auto r) { issue(r, (uint32_t)decltype(r)::value); });
    }
  };
  enter(resolve(item_of(q_cur)));
  for (uint32_t i = blockIdx.x; i < n_cold; i += gridDim.x) {
    const uint32_t bi = q_cur;
    // the next quad's segment: its descriptor is requested here, resolved behind the staging barriers and entered at the end of this
    // quad's tiles -- none of the three dependent loads stands between the last tile and the next segment's first loads
    const ItemDesc d_next = item_of(q_nx);
    q_cur = q_nx;
    q_nx = quad_at(i + 2u * gridDim.x);
    __syncthreads();  // the previous quad's operands and verdict are done with
    const ItemDesc d0 = src.items[4 * bi];
    const uint32_t c0 = src.cnt[d0.list] - d0.group * (uint32_t)NQ;
    const uint32_t nq = c0 < (uint32_t)NQ ? c0 : (uint32_t)NQ;
    if (threadIdx.x == 0) { live_flag = 0u; tiles_l = 0u; }
    if (threadIdx.x < nq) {  // the quad's queries: pair, threshold as the hot lists left it, scale, brackets
      const uint32_t pr = src.pair_of(4 * bi, (int)threadIdx.x);
      const uint32_t qix = pr / src.P;
      pair_l[threadIdx.x] = pr;
      qix_l[threadIdx.x] = qix;
      const uint32_t b32 = __hip_atomic_load(hp.bounds32 + src.slot_of_pair(pr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      thr_l[threadIdx.x] = b32 == 0xFFFFFFFFu ? __builtin_inff() : __uint_as_float(order_bits_to_f32_bits(b32));
      sn_l[threadIdx.x] = hp.qhead[2u * qix + 1u];
      const double ex = (double)hp.qhead[2u * qix];
      for (uint32_t c = kHeadFirst; c <= hs; ++c)
        brk_l[threadIdx.x][c - kHeadFirst] = prune_round_up((double)hp.prune_tab[(uint64_t)qix * hp.n_steps + c] + ex);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nq * ch; i += kWave * kHeadWaves) {  // consecutive threads: consecutive 16 bytes of one query's row
      const uint32_t slot = i / ch, j = i - slot * ch;
      *reinterpret_cast<u32x4*>(qb + ((size_t)j * NQ + slot) * 16u) = *reinterpret_cast<const u32x4*>(hp.q8 + (uint64_t)qix_l[slot] * H + 16u * j);
    }
    __syncthreads();
    // a wave per segment of the quad: the segment was entered, and its first R steps requested, before the barriers above
    const Seg seg_next = resolve(d_next);
    if (lane == 0 && n_tiles != 0u) atomicAdd(&tiles_l, n_tiles);
    const int n = lane & 31;
    // The second query set's MFMAs run for every group of a 64-query block, also one of <= 32 queries: twice the matrix work for such a
    // group, on operand slots 32 .. 63 that the staging above did not write (integer products of whatever LDS holds; its columns are
    // masked out of the verdict: q < nq).  A block-uniform branch inside a step's math made the compiler keep the ring's new loads in registers of their own
    // and copy them at the loop's end, behind a wait for them -- and the matrix cores are far from being the limit here.
    constexpr bool two = NQ > 32;
    for (uint32_t t = 0; t < n_tiles; ++t) {
      if (__hip_atomic_load(&live_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0u) break;  // (wave-uniform: one LDS word)
      const uint32_t rows_t = nrows - t * kWave < (uint32_t)kWave ? nrows - t * kWave : (uint32_t)kWave;
      const float xn = xn_next;  // requested a tile ago; the next tile's (the last one's again behind it) goes out now
      xn_next = hp.xnorm[(uint64_t)row_s + (t + 1u < n_tiles ? t + 1u : t) * kWave + lane];
      const uint32_t p0 = t * kHeadFirst;  // the tile's first position in the stream
      i32x16_t acc[2][2];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[a][h][e] = 0;
      int nsq[2] = {0, 0};
      bool dead = false;  // (wave-uniform)
      // a tile can be dead only if its 64 |x|^2 are finite (the rule pre_prune applies)
      const bool finite = __ballot(!(__builtin_fabsf(xn) < __builtin_inff())) == 0;
      auto math = [&](auto stag, uint32_t s) {  // step s of the tile, from slot
        constexpr int b = decltype(stag)::value;
#pragma unroll
        for (int cbi = 0; cbi < 2; ++cbi) {
          const uint32_t j = (2u * s + (uint32_t)cbi) * 2u + (uint32_t)(lane >> 5);
          const i32x4_t b0 = *reinterpret_cast<const i32x4_t*>(qb + ((size_t)j * NQ + (uint32_t)(n & (NQ - 1))) * 16u);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const i32x4_t ar = __builtin_bit_cast(i32x4_t, ring[b][2 * cbi + h]);
            acc[0][h] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ar, b0, acc[0][h], 0, 0, 0);
#pragma unroll
            for (int u = 0; u < 4; ++u) nsq[h] = __builtin_amdgcn_sdot4(ar[u], ar[u], nsq[h], false);
          }
          if constexpr (two) {
              const i32x4_t b1 = *reinterpret_cast<const i32x4_t*>(qb + ((size_t)j * NQ + 32u + (uint32_t)n) * 16u);
#pragma unroll
              for (int h = 0; h < 2; ++h)
                acc[1][h] = __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4_t, ring[b][2 * cbi + h]), b1, acc[1][h], 0, 0, 0);
            }
        }
      };
      auto verdict = [&](uint32_t c) {  // c = columns consumed / 64 (>= kHeadFirst) -> true: the tile is dead at this boundary
        // sum of X^2 of whole rows (the lane's 16 columns per column block + the other k half's), minimum over the tile's live rows
        uint32_t nm = 0xFFFFFFFFu;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint32_t tot = (uint32_t)(nsq[h] + __shfl_xor(nsq[h], 32, kWave));
          if (32u * (uint32_t)h + (uint32_t)n < rows_t) nm = tot < nm ? tot : nm;
        }
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) {
          const uint32_t o = (uint32_t)__shfl_xor((int)nm, off, kWave);
          nm = o < nm ? o : nm;
        }
        const double nterm = head_norm_term(nm, sx, Rh2, (double)hp.om);
        bool keep = !finite;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          if (a == 1 && !two) break;  // (compile-time)
          const uint32_t q = (uint32_t)(a * 32 + n);
          // the lane's query column: rows 32 h + 8 (e >> 2) + 4 (lane >> 5) + (e & 3) of the tile
          int im = 0x7FFFFFFF;
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const uint32_t row = 32u * (uint32_t)h + 8u * (uint32_t)(e >> 2) + 4u * (uint32_t)(lane >> 5) + (uint32_t)(e & 3);
              if (row < rows_t) im = acc[a][h][e] < im ? acc[a][h][e] : im;
            }
          const int io = __shfl_xor(im, 32, kWave);
          im = io < im ? io : im;
          if (q < nq && q < (uint32_t)NQ)
            keep |= !(head_lower_dot(im, nterm, sx, sn_l[q], brk_l[q][c - kHeadFirst]) > (double)thr_l[q]);
        }
        return __ballot(keep) == 0;
      };
      // the prefix: every slot but the last goes out again the moment its step is consumed
      head_static_for<(int)kHeadFirst>([&](auto st) {
        constexpr int s = decltype(st)::value, sl = s % R;
        math(std::integral_constant<int, sl>{}, (uint32_t)s);
        if constexpr (s + 1 < (int)kHeadFirst) issue(std::integral_constant<int, sl>{}, p0 + (uint32_t)s + (uint32_t)R);
      });
      dead = verdict(kHeadFirst);
      // a tile that survives the first test (few do) reads its later steps on demand, one at a time, through the free slot: the next tile's
      // prefix waits in the other slots and is consumed afterwards, not fetched twice
      for (uint32_t s = kHeadFirst; !dead && s < hs; ++s) {
        const u32x4* a = sp + ((size_t)t * hs + s) * 256u;
#pragma unroll
        for (int i = 0; i < 4; ++i) ring[kLastSlot][i] = __builtin_nontemporal_load(a + (size_t)i * 64u);
        steps_read += 1u;
        math(std::integral_constant<int, kLastSlot>{}, s);
        dead = verdict(s + 1u);
      }
      issue(std::integral_constant<int, kLastSlot>{}, p0 + kHeadFirst - 1u + (uint32_t)R);
      if (!dead) {
        if (lane == 0) __hip_atomic_store(&live_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        break;
      }
    }
    // on to the wave's segment of the block's next quad, ahead of the barriers: what the ring still holds of this one -- re-reads of the
    // last step at a segment's end, up to R steps of the tiles a live verdict leaves unread -- is dropped
    enter(seg_next);
    __syncthreads();
    if (live_flag == 0u) {  // (block-uniform) every tile of the quad is ruled out for every query of the group
      const uint32_t kp = hp.kp;
      for (uint32_t i = threadIdx.x; i < nq * kp; i += kWave * kHeadWaves) {
        const uint32_t qi = i / kp, e = i - qi * kp;
        (src.partials + ((uint64_t)pair_l[qi] * src.S_max + (d0.seg >> 2)) * src.k_keep)[e] = kKeyMax;  // (= src.out_quad(4 * bi, qi)[e])
      }
      if (threadIdx.x == 0) {
        const_cast<ItemDesc*>(src.items)[4 * bi].group = d0.group | kQuadDead;
        ctr_l[1] += 1u;
        ctr_l[3] += tiles_l;
      }
    }
    if (threadIdx.x == 0) ctr_l[0] += 1u;
  }
  if (lane == 0 && steps_read != 0u) atomicAdd(&ctr_l[2], steps_read);
  __syncthreads();
  if (threadIdx.x < 3 && ctr_l[threadIdx.x] != 0u) {
    atomicAdd(hp.last + threadIdx.x, ctr_l[threadIdx.x]);
    atomicAdd(hp.tot + threadIdx.x, (unsigned long long)ctr_l[threadIdx.x]);
  }
  if (threadIdx.x == 0 && ctr_l[3] != 0u) {  // every step of those tiles ran no math
    atomicAdd(hp.prune_last + 1, ctr_l[3] * hp.n_steps);
    atomicAdd(hp.prune_last + 2, ctr_l[3]);
    atomicAdd(hp.prune_tot + 1, (unsigned long long)ctr_l[3] * hp.n_steps);
    atomicAdd(hp.prune_tot + 2, (unsigned long long)ctr_l[3]);
  }
  // the launch's verdict for the handle's back-off: by the block that finishes last, once every block's counters are in
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    if (atomicAdd(hp.done, 1u) == gridDim.x - 1u) {
      __threadfence();
      const uint32_t tested = __hip_atomic_load(hp.last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t died = __hip_atomic_load(hp.last + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (8u * died < (tested ? tested : 1u)) __hip_atomic_store(hp.watch, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

}  // namespace vers
