// ivf_build.hip -- everything that CHANGES the index: build_index (ivfflat.rs:102-136: k-means driver, best of attempts,
// inverted lists), the row-sharded build over processes, upload of the five fields after load_index, add (ivfflat.rs:200-213).
//
// Device layout (HBM): the reference keeps `values` in vec_id order and gathers list members
// through `ids` (ivfflat.rs:172-174).  Here rows are stored CLUSTER-MAJOR: list c occupies the
// contiguous rows [list_off[c], list_off[c]+list_len[c]) in the reference's list order
// (ascending vec_id for built rows, append order for added ones), followed by slack for `add`;
// row_ids[] maps a storage row back to its vec_id.  Lists start on 64-row boundaries and the rows
// themselves are held in lane-transposed 64-row tiles (scan.hip.h), so a list scan is one linear HBM
// stream of contiguous 1 KiB wave loads.
#include <chrono>
#include <thread>

#include "gemm.hip.h"
#include "ivf_handle.hpp"
#include "prescan.hip.h"
#include "ball_filter.hip.h"
#include "head_filter.hip.h"
#include "update_plan.hpp"

namespace vers {

// ---- storage construction ---------------------------------------------------------------------
// rows of X (vec_id order, row-major pitch ldx) -> cluster-major storage in lane-transposed tiles;
// grid-stride over (sorted position, float4 column)
// (columns >= d of X are the caller's padding and may hold anything: they are stored as zeros)
__global__ void gather_rows_kernel(const float* X, uint32_t ldx, uint32_t d, uint32_t ld, const uint32_t* sorted_ids,
                                   const uint32_t* assign, const uint32_t* starts, const uint32_t* list_off,
                                   const uint8_t* owner, uint32_t rank, uint64_t n, float* rows, uint32_t* row_ids) {
  const uint32_t ld4 = ld / 4, ldx4 = ldx / 4;
  const uint64_t total = n * ld4;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p = i / ld4;
    const uint32_t c4 = (uint32_t)(i % ld4);
    const uint32_t id = sorted_ids[p];
    const uint32_t c = assign[id];
    if (owner != nullptr && owner[c] != rank) continue;  // another GPU's list
    const uint64_t dst = (uint64_t)list_off[c] + (p - starts[c]);
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (c4 < ldx4 && c4 * 4 < d) {
      v = reinterpret_cast<const f32x4*>(X + (uint64_t)id * ldx)[c4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (c4 * 4 + u >= d) v[u] = 0.0f;
    }
    *reinterpret_cast<f32x4*>(rows + blocked_index(dst, c4 * 4, ld)) = v;
    if (c4 == 0) row_ids[dst] = id;
  }
}

// The same placement, one BLOCK per destination tile of 64 storage rows: the 64 source rows are read as they lie (3 KB
// contiguous each), turned through LDS 64 float4 columns at a time, and written as the tile's contiguous 1 KiB pieces.
// (gather_rows_kernel above writes every float4 to its own piece: 16 useful bytes per 64-byte sector and a stride of 1 KiB
// between consecutive threads -- 69 ms for N = 10M x 768, 0.9 TB/s, the largest serial-looking kernel of build_index.)
// tile_list[t] = the list tile t belongs to (lists start on tile boundaries); rows of the tile past the list's length are
// written as zeros (slack for `add`), their row_ids stay 0xFFFFFFFF.
constexpr uint32_t kGatherCols4 = 64;  // float4 columns per pass: 64 rows x 65 float4 = 66.5 KB of LDS
// row_src != nullptr (the receive side of the row-sharded build): storage row r holds source row row_src[r] of X (0xFFFFFFFF: none)
// and its vec id is src_ids[that row]; otherwise the source of a row follows from the cluster-sorted order (sorted_ids / starts).
__global__ __launch_bounds__(256) void gather_tiles_kernel(const float* X, uint32_t ldx, uint32_t d, uint32_t ld, const uint32_t* sorted_ids,
                                                           const uint32_t* starts, const uint32_t* list_off, const uint32_t* list_len,
                                                           const uint32_t* tile_list, float* rows, uint32_t* row_ids,
                                                           const uint32_t* row_src = nullptr, const uint32_t* src_ids = nullptr) {
  extern __shared__ __attribute__((aligned(16))) f32x4 tl[];  // [64][kGatherCols4 + 1]
  __shared__ uint32_t s_id[kWave];
  const uint32_t t = blockIdx.x, c = tile_list[t];
  const uint32_t row0 = t * 64u, in_list0 = row0 - list_off[c], len = list_len[c];
  const uint32_t n_valid = in_list0 < len ? (len - in_list0 < 64u ? len - in_list0 : 64u) : 0u;
  if (threadIdx.x < 64) {
    uint32_t id = 0xFFFFFFFFu;
    if (threadIdx.x < n_valid) id = row_src ? row_src[row0 + threadIdx.x] : sorted_ids[starts[c] + in_list0 + threadIdx.x];
    s_id[threadIdx.x] = id;
    if (id != 0xFFFFFFFFu) row_ids[row0 + threadIdx.x] = src_ids ? src_ids[id] : id;
  }
  __syncthreads();
  const uint32_t ld4 = ld / 4, ldx4 = ldx / 4;
  f32x4* tile = reinterpret_cast<f32x4*>(rows + (uint64_t)t * 64ull * ld);
  constexpr uint32_t kPitch = kGatherCols4 + 1;
  for (uint32_t c0 = 0; c0 < ld4; c0 += kGatherCols4) {
    const uint32_t nc = ld4 - c0 < kGatherCols4 ? ld4 - c0 : kGatherCols4;
    for (uint32_t i = threadIdx.x; i < 64u * kGatherCols4; i += 256u) {  // a row's float4s by consecutive threads
      const uint32_t r = i / kGatherCols4, j = i % kGatherCols4, c4 = c0 + j;
      f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
      const uint32_t id = s_id[r];
      if (j < nc && id != 0xFFFFFFFFu && c4 < ldx4 && c4 * 4 < d) {
        v = reinterpret_cast<const f32x4*>(X + (uint64_t)id * ldx)[c4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (c4 * 4 + u >= d) v[u] = 0.0f;  // (columns >= d of X are the caller's padding and may hold anything)
      }
      tl[r * kPitch + j] = v;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 64u * nc; i += 256u) {  // a piece's 64 rows by consecutive threads: 1 KiB contiguous
      const uint32_t j = i / 64u, r = i % 64u;
      tile[(uint64_t)(c0 + j) * 64 + r] = tl[r * kPitch + j];
    }
    __syncthreads();
  }
}

// vers_ivf_add: the ranked list and the stream's status word in one place (one copy back), the word cleared; and the call's three
// table updates (vec id of the new storage row, the list's length by centroid and by slot)
__global__ void add_fetch_kernel(const uint64_t* probe, uint32_t* st_word, uint64_t* out) {
  out[0] = probe[0];
  out[1] = *st_word;
  *st_word = 0u;
}
__global__ void add_tables_kernel(uint32_t* row_id, uint32_t vid, uint32_t* list_len, uint32_t* slot_len, uint32_t len) {
  if (row_id != nullptr) *row_id = vid;
  *list_len = len;
  *slot_len = len;
}

// one padded row (ld floats, row-major) -> storage row `dst` of the blocked matrix
__global__ void scatter_row_kernel(const float* row, uint32_t ld, uint64_t dst, float* rows) {
  const uint32_t c4 = blockIdx.x * blockDim.x + threadIdx.x;
  if (c4 < ld / 4)
    *reinterpret_cast<f32x4*>(rows + blocked_index(dst, c4 * 4, ld)) = reinterpret_cast<const f32x4*>(row)[c4];
}

__global__ void gather_init_kernel(const float* X, uint32_t ldx, uint32_t d, uint32_t ldc, const uint32_t* idx, uint32_t k, float* C) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)k * ldc) return;
  const uint32_t j = (uint32_t)(i % ldc);
  C[i] = j < d ? X[(uint64_t)idx[i / ldc] * ldx + j] : 0.0f;
}

// device-resident `assignments` (usize = u64 in the reference) -> the u32 the kernels use; *bad != 0: one of them is >= k
__global__ void u64_to_u32_checked_kernel(const uint64_t* in, uint64_t n, uint64_t k, uint32_t* out, uint32_t* bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t v = in[i];
  if (v >= k) *bad = 1u;
  out[i] = (uint32_t)v;
}

__global__ void u32_to_u64_kernel(const uint32_t* in, uint64_t n, uint64_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[i];
}


// ---- streamed upload (vers_ivf_upload_begin / _chunk / _end): chunk placement -------------------------------------------
// One BLOCK per 64 consecutive positions of a chunk's cluster-sorted order: the source rows are read as they lie (3 KB
// contiguous each), turned through LDS 64 float4 columns at a time (as gather_tiles_kernel), and written into the
// lane-transposed tiles of their lists -- consecutive sorted positions of one list are consecutive storage rows, so the 64
// rows' float4s of a column are runs of contiguous 16-byte pieces.  Row p of the sorted order (source row id = sorted_ids[p],
// list c) goes to position fill[c] + (p - starts[c]) of list c: the chunks arrive in ascending vec id, so a list fills in
// the reference's order (ivfflat.rs:123-127).  Rows of lists another rank owns are skipped; a row past its list's announced
// length is skipped too (advance_fill_kernel reports it).  vec id = ids32[id] (host path: only the owned rows were sent) or
// first + id.
__global__ __launch_bounds__(256) void place_chunk_kernel(const float* X, uint32_t ldx, uint32_t d, uint32_t ld, const uint32_t* sorted_ids,
                                                          const uint32_t* assign, const uint32_t* starts, const uint32_t* list_off,
                                                          const uint32_t* list_len, const uint32_t* fill, const uint8_t* owner, uint32_t rank,
                                                          const uint32_t* ids32, uint32_t first, uint32_t n, float* rows, uint32_t* row_ids) {
  extern __shared__ __attribute__((aligned(16))) f32x4 tl[];  // [64][kGatherCols4 + 1]
  __shared__ uint32_t s_src[kWave], s_dst[kWave];
  __shared__ uint32_t s_any;
  if (threadIdx.x == 0) s_any = 0u;
  __syncthreads();
  if (threadIdx.x < 64) {
    const uint32_t p = blockIdx.x * 64u + threadIdx.x;
    uint32_t src = 0xFFFFFFFFu, dst = 0u;
    if (p < n) {
      const uint32_t id = sorted_ids[p], c = assign[id];
      if (owner == nullptr || owner[c] == rank) {
        const uint32_t pos = fill[c] + (p - starts[c]);
        if (pos < list_len[c]) {
          src = id;
          dst = list_off[c] + pos;
          row_ids[dst] = ids32 ? ids32[id] : first + id;
          s_any = 1u;
        }
      }
    }
    s_src[threadIdx.x] = src;
    s_dst[threadIdx.x] = dst;
  }
  __syncthreads();
  if (!s_any) return;
  const uint32_t ld4 = ld / 4, ldx4 = ldx / 4;
  constexpr uint32_t kPitch = kGatherCols4 + 1;
  for (uint32_t c0 = 0; c0 < ld4; c0 += kGatherCols4) {
    const uint32_t nc = ld4 - c0 < kGatherCols4 ? ld4 - c0 : kGatherCols4;
    for (uint32_t i = threadIdx.x; i < 64u * kGatherCols4; i += 256u) {  // a row's float4s by consecutive threads
      const uint32_t r = i / kGatherCols4, j = i % kGatherCols4, c4 = c0 + j;
      f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
      const uint32_t id = s_src[r];
      if (j < nc && id != 0xFFFFFFFFu && c4 < ldx4 && c4 * 4 < d) {
        v = reinterpret_cast<const f32x4*>(X + (uint64_t)id * ldx)[c4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (c4 * 4 + u >= d) v[u] = 0.0f;  // (columns >= d of X are the caller's padding and may hold anything)
      }
      tl[r * kPitch + j] = v;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 64u * nc; i += 256u) {  // a column's 64 rows by consecutive threads
      const uint32_t j = i / 64u, r = i % 64u;
      if (s_src[r] != 0xFFFFFFFFu) *reinterpret_cast<f32x4*>(rows + blocked_index((uint64_t)s_dst[r], (c0 + j) * 4, ld)) = tl[r * kPitch + j];
    }
    __syncthreads();
  }
}

// after a chunk is placed: fill[c] += its rows of list c (owned lists), seen[c] += them (every list, when the chunk held
// ALL its rows); *bad |= 2 when a list received more rows than begin announced
__global__ void advance_fill_kernel(const uint32_t* counts, uint32_t k, const uint8_t* owner, uint32_t rank, const uint32_t* list_len, uint32_t* fill,
                                    uint32_t* seen, uint32_t* bad) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= k) return;
  const uint32_t cnt = counts[c];
  if (seen) seen[c] += cnt;
  if (owner == nullptr || owner[c] == rank) {
    const uint64_t f = (uint64_t)fill[c] + cnt;
    if (f > list_len[c]) { *bad |= 2u; fill[c] = list_len[c]; }
    else fill[c] = (uint32_t)f;
  }
}


// ---- vers_ivf_add_batch: placement of a staged chunk and the derived arrays of the tiles it touched -------------------------------
// One job per destination tile of 64 storage rows: rows [lo, hi) of tile `tile` receive the chunk's rows sorted[src], sorted[src + 1], ...
// (the cluster-sorted order of the chunk: one list's new rows are consecutive there, in ascending vec id).  The other rows of the tile --
// the list's existing rows in front, slack behind -- keep their bits.
struct AddTileJob {
  uint32_t tile, lo, hi, src;
};

// One BLOCK per job, as gather_tiles_kernel: the new rows are read as they lie (whole rows of the staged chunk, zero-padded to ldx),
// the rest of a partly new tile is read back in its own 1 KiB pieces, and every float4 column of the tile is written as one whole
// 1 KiB piece from LDS.  row_ids[new row] = vid0 + its index in the chunk.
__global__ __launch_bounds__(256) void add_tiles_kernel(const float* X, uint32_t ldx, uint32_t d, uint32_t ld, const AddTileJob* jobs,
                                                        const uint32_t* sorted, uint32_t vid0, float* rows, uint32_t* row_ids) {
  extern __shared__ __attribute__((aligned(16))) f32x4 tl[];  // [64][kGatherCols4 + 1]
  __shared__ uint32_t s_src[kWave];
  const AddTileJob jb = jobs[blockIdx.x];
  if (threadIdx.x < 64) {
    uint32_t src = 0xFFFFFFFFu;
    if (threadIdx.x >= jb.lo && threadIdx.x < jb.hi) {
      src = sorted[jb.src + (threadIdx.x - jb.lo)];
      row_ids[(uint64_t)jb.tile * 64 + threadIdx.x] = vid0 + src;
    }
    s_src[threadIdx.x] = src;
  }
  __syncthreads();
  const bool partial = jb.lo > 0 || jb.hi < 64;
  const uint32_t ld4 = ld / 4, ldx4 = ldx / 4;
  f32x4* tile = reinterpret_cast<f32x4*>(rows + (uint64_t)jb.tile * 64ull * ld);
  constexpr uint32_t kPitch = kGatherCols4 + 1;
  for (uint32_t c0 = 0; c0 < ld4; c0 += kGatherCols4) {
    const uint32_t nc = ld4 - c0 < kGatherCols4 ? ld4 - c0 : kGatherCols4;
    for (uint32_t i = threadIdx.x; i < 64u * kGatherCols4; i += 256u) {  // the new rows: a row's float4s by consecutive threads
      const uint32_t r = i / kGatherCols4, j = i % kGatherCols4, c4 = c0 + j;
      const uint32_t id = s_src[r];
      if (j >= nc || id == 0xFFFFFFFFu) continue;
      f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
      if (c4 < ldx4 && c4 * 4 < d) v = reinterpret_cast<const f32x4*>(X + (uint64_t)id * ldx)[c4];  // (the stage's padding is zero)
      tl[r * kPitch + j] = v;
    }
    if (partial)
      for (uint32_t i = threadIdx.x; i < 64u * nc; i += 256u) {  // the rows that stay: read back piece by piece
        const uint32_t j = i / 64u, r = i % 64u;
        if (s_src[r] == 0xFFFFFFFFu) tl[r * kPitch + j] = tile[(uint64_t)(c0 + j) * 64 + r];
      }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 64u * nc; i += 256u) {  // a piece's 64 rows by consecutive threads: 1 KiB contiguous
      const uint32_t j = i / 64u, r = i % 64u;
      tile[(uint64_t)(c0 + j) * 64 + r] = tl[r * kPitch + j];
    }
    __syncthreads();
  }
}

// the chunk's rows per list onto both length tables (every list: a sharded rank counts the rows it does not store, as vers_ivf_add)
__global__ void add_counts_kernel(const uint32_t* counts, uint32_t k, const uint32_t* list_slot, uint32_t* list_len, uint32_t* slot_len) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= k || counts[c] == 0) return;
  list_len[c] += counts[c];
  slot_len[list_slot[c]] += counts[c];
}

// assignments of the kept rows are cluster indices (< k) before anything is indexed by them; an out-of-range one is reported and
// replaced by 0 so that the grouping stays in bounds (the chunk is then refused before its placement)
__global__ void add_check_assign_kernel(uint32_t* a, uint32_t n, uint32_t k, uint32_t* bad) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && a[i] >= k) { a[i] = 0u; *bad = 1u; }
}

// rows [0, ld) of the chunk's source pitch -> the zero-padded stage [n][ldx] (the caller's columns d .. ld_src-1 may hold anything)
__global__ void add_stage_rows_kernel(const float* src, uint64_t ld_src, uint32_t d, uint32_t ldx, uint64_t n, float* dst) {
  const uint32_t ldx4 = ldx / 4;
  const uint64_t total = n * ldx4;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = i / ldx4;
    const uint32_t c4 = (uint32_t)(i % ldx4);
    f32x4 v = reinterpret_cast<const f32x4*>(src + r * ld_src)[c4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (c4 * 4 + u >= d) v[u] = 0.0f;
    reinterpret_cast<f32x4*>(dst + r * ldx)[c4] = v;
  }
}

// Tile-list forms of refresh_norms' kernels: row i of the list is storage row tiles[i / 64] * 64 + i % 64 (same per-row bodies, prescan.hip.h)
__global__ void rows_to_f16_tiles_kernel(const float* rows, uint32_t ld, const uint32_t* tiles, uint64_t n_rows, uint16_t* rows_h) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t g8 = ld / 8;
  const uint64_t i = t / g8;
  if (i >= n_rows) return;
  row_to_f16(rows, ld, (uint64_t)tiles[i >> 6] * 64 + (i & 63), (uint32_t)(t % g8), rows_h);
}
__global__ void shadow_residual_tiles_kernel(const float* rows, uint32_t ld, const uint32_t* row_ids, const uint32_t* tiles, uint64_t n_rows,
                                             uint32_t* rmax2_bits) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  const uint64_t r = (uint64_t)tiles[i >> 6] * 64 + (i & 63);
  if (row_ids[r] == 0xFFFFFFFFu) return;
  row_shadow_residual(rows, ld, r, rmax2_bits);
}
__global__ void row_norms_tiles_kernel(const float* rows, uint32_t ld, const uint32_t* row_ids, const uint32_t* tiles, uint64_t n_rows, float* xnorm,
                                       uint32_t* xmax2_bits) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  row_norm_blocked(rows, ld, row_ids, (uint64_t)tiles[i >> 6] * 64 + (i & 63), xnorm, xmax2_bits);
}
// The row-major copy (vers_ivf::rows_rm, all ld columns as refresh_norms writes it) of the listed tiles: one BLOCK per tile, gather_tiles_kernel
// backwards -- the tile's 1 KiB pieces are read as they lie, turned through LDS 64 float4 columns at a time, and every row leaves as one
// contiguous run.  (Until the removal work a thread per element read its float out of a 16-byte piece 1 KiB from its neighbour's: 37.7 ms for
// the 155 k tiles a removal of 65,536 random ids touches at cfg3 -- three times the compaction itself.)
__global__ __launch_bounds__(256) void tiles_to_rowmajor_kernel(const float* in, uint32_t ld, const uint32_t* tiles, float* out) {
  extern __shared__ __attribute__((aligned(16))) f32x4 tl[];  // [64][kGatherCols4 + 1]
  const uint64_t t = tiles[blockIdx.x];
  const uint32_t ld4 = ld / 4;
  const f32x4* tile = reinterpret_cast<const f32x4*>(in + t * 64ull * ld);
  f32x4* rm = reinterpret_cast<f32x4*>(out + t * 64ull * ld);
  constexpr uint32_t kPitch = kGatherCols4 + 1;
  for (uint32_t c0 = 0; c0 < ld4; c0 += kGatherCols4) {
    const uint32_t nc = ld4 - c0 < kGatherCols4 ? ld4 - c0 : kGatherCols4;
    for (uint32_t i = threadIdx.x; i < 64u * nc; i += 256u) {  // a piece's 64 rows by consecutive threads: 1 KiB contiguous
      const uint32_t j = i / 64u, r = i % 64u;
      tl[r * kPitch + j] = tile[(uint64_t)(c0 + j) * 64 + r];
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 64u * kGatherCols4; i += 256u) {  // a row's float4s by consecutive threads
      const uint32_t r = i / kGatherCols4, j = i % kGatherCols4;
      if (j < nc) rm[(uint64_t)r * ld4 + c0 + j] = tl[r * kPitch + j];
    }
    __syncthreads();
  }
}

// ---- vers_ivf_recluster: the tiled list storage back to the live rows in ascending vec id ------------------------------------------------
// [recluster gather kernel: begin] (tests/test_recluster_kernel_host.py runs the text between the two markers on the host)
// One job per OCCUPIED tile, made on the host from the lists' offsets and lengths (vers_ivf::tile_list is not used: a re-layout leaves it
// stale): the tile and how many of its rows lie below its list's length.
struct GatherJob {
  uint32_t tile, n_valid;  // storage row / 64 | 1 .. 64
};
// One BLOCK per occupied tile (jobs[blockIdx.x]), tiles_to_rowmajor_kernel with a destination per ROW: the tile's 1 KiB pieces are read as
// they lie, turned through LDS kGatherCols4 float4 columns at a time, and every live row r of the tile -- r < n_valid: below its list's
// length -- leaves as one contiguous run to row rank[row_ids[r]] of X' (pitch floats a row, a multiple of 4, <= ld).  Columns d .. pitch - 1
// are written as zeros whatever the tile holds there; a row past the list's length is written nowhere, so what slack holds (NaN, anything)
// reaches nothing.  Only the f32 tiles are read.  The destinations of the tile's 64 rows sit behind the [64][kGatherCols4 + 1] float4s of
// the dynamic LDS.
__global__ __launch_bounds__(256) void tiles_to_live_rows_kernel(const float* in, uint32_t ld, uint32_t d, uint32_t pitch, const GatherJob* jobs,
                                                                 const uint32_t* row_ids, const uint64_t* rank, uint64_t n_total, uint64_t m,
                                                                 float* out) {
  extern __shared__ __attribute__((aligned(16))) f32x4 tl[];  // [64][kGatherCols4 + 1] | u32 [64]
  constexpr uint32_t kPitch = kGatherCols4 + 1;
  uint32_t* s_dst = reinterpret_cast<uint32_t*>(tl + 64u * kPitch);
  const uint64_t t = jobs[blockIdx.x].tile;
  const uint32_t n_valid = jobs[blockIdx.x].n_valid;
  if (threadIdx.x < 64u) {
    uint32_t dst = 0xFFFFFFFFu;
    if (threadIdx.x < n_valid) {
      const uint32_t v = row_ids[t * 64ull + threadIdx.x];
      if (v < n_total && rank[v] < m) dst = (uint32_t)rank[v];
    }
    s_dst[threadIdx.x] = dst;
  }
  const uint32_t p4 = pitch / 4;
  const f32x4* tile = reinterpret_cast<const f32x4*>(in + t * 64ull * ld);
  f32x4* xo = reinterpret_cast<f32x4*>(out);
  for (uint32_t c0 = 0; c0 < p4; c0 += kGatherCols4) {
    const uint32_t nc = p4 - c0 < kGatherCols4 ? p4 - c0 : kGatherCols4;
    for (uint32_t i = threadIdx.x; i < 64u * nc; i += 256u) {  // a piece's 64 rows by consecutive threads: 1 KiB contiguous
      const uint32_t j = i / 64u, r = i % 64u;
      tl[r * kPitch + j] = tile[(uint64_t)(c0 + j) * 64 + r];
    }
    lds_barrier();  // (the first pass: s_dst too)
    for (uint32_t i = threadIdx.x; i < 64u * kGatherCols4; i += 256u) {  // a row's float4s by consecutive threads
      const uint32_t r = i / kGatherCols4, j = i % kGatherCols4;
      const uint32_t dst = s_dst[r];
      if (j < nc && dst != 0xFFFFFFFFu) {
        f32x4 v = tl[r * kPitch + j];
        const uint32_t col = (c0 + j) * 4u;
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (col + u >= d) v[u] = 0.0f;
        xo[(uint64_t)dst * p4 + c0 + j] = v;
      }
    }
    lds_barrier();
  }
}
// [recluster gather kernel: end]
// One bit's worth (a u32 the device scan sums) per vec id that is in some list: a row counts when it lies below its list's length -- what a
// slack row's row_ids entry happens to hold is never looked at.  One thread per (job, row).
__global__ void recluster_live_kernel(const GatherJob* jobs, uint32_t n_jobs, const uint32_t* row_ids, uint64_t n_total, uint32_t* live) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)n_jobs * 64u) return;
  const GatherJob jb = jobs[i >> 6];
  if ((uint32_t)(i & 63u) >= jb.n_valid) return;
  const uint32_t v = row_ids[(uint64_t)jb.tile * 64u + (i & 63u)];
  if (v < n_total) live[v] = 1u;
}
// L[rank[v]] = v for every live vec id (rank = the exclusive prefix over `live`)
__global__ void recluster_order_kernel(const uint32_t* live, const uint64_t* rank, uint64_t n_total, uint64_t m, uint32_t* L) {
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n_total && live[v] && rank[v] < m) L[rank[v]] = (uint32_t)v;
}
// install_index on X' wrote row_ids as positions in X': every entry that holds a vector becomes its vec id
__global__ void recluster_relabel_kernel(uint32_t* row_ids, uint64_t cap_rows, const uint32_t* L, uint64_t m) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= cap_rows) return;
  const uint32_t p = row_ids[r];
  if (p != 0xFFFFFFFFu) row_ids[r] = p < m ? L[p] : 0xFFFFFFFFu;
}
// out_assignments of the call, indexed by vec id: the cluster of position rank[v] of X' for a live id, 0 for an id in no list
__global__ void recluster_assign_out_kernel(const uint32_t* live, const uint64_t* rank, const uint32_t* a, uint64_t n_total, uint64_t m, uint64_t* out) {
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n_total) out[v] = live[v] && rank[v] < m ? a[rank[v]] : 0ull;
}

// ---- vers_ivf_compact: whole tiles move to a tighter storage plan, every derived array written from the one read -------------------------
// Lists start on tile boundaries and a removal has already closed the gaps inside a list, so the ceil(len / 64) tiles of an owned list
// move as they lie: one job = one tile, from the old storage to the new one.
struct CompactJob {
  uint32_t src, dst;  // tile indices (storage row / 64) in the old and in the new plan
};
// One BLOCK per job.  The tile's 1 KiB pieces are read ONCE, kGatherCols4 float4 columns per pass (a tile of d = 768 is 196 KB: more than
// the CU's LDS), and from that one read leave as
//   * the destination f32 tile, whole pieces, straight from the registers that loaded them;
//   * the row-major rows (dst_rm != nullptr), whole-row runs out of LDS -- tiles_to_rowmajor_kernel's second half;
//   * the fp16 shadow tile (dst_h != nullptr) in row_to_f16's A-operand layout, the same conversion, one 1 KiB piece per wave store;
//   * |x|^2 (wave 0, a row per lane) and the fp16 residual (wave 1, a row per lane; only with a shadow, as refresh_norms): the f32
//     chains of row_norm_blocked / row_shadow_residual over the columns in storage order, the accumulator staying in its register from
//     pass to pass -- the same sums bit for bit.  Both maxima: one atomicMax per block after a reduction over the wave that holds them.
// A row whose row_ids entry is 0xFFFFFFFF (slack inside a list's last tile) moves like the others -- nothing may depend on what it
// holds -- but gets xnorm 0.0f and raises no maximum.  row_ids of the tile are copied by the same block.
// The barriers order LDS traffic only: nothing a block writes to memory is read by it, its stores stay in flight across the passes.
__global__ __launch_bounds__(256) void compact_tiles_kernel(const CompactJob* jobs, uint32_t ld, const float* src_rows, const uint32_t* src_ids,
                                                            float* dst_rows, uint32_t* dst_ids, uint16_t* dst_h, float* dst_rm, float* xnorm,
                                                            uint32_t* xmax2_bits, uint32_t* rmax2_bits) {
  extern __shared__ __attribute__((aligned(16))) f32x4 tl[];  // [64][kGatherCols4 + 1]
  const CompactJob jb = jobs[blockIdx.x];
  const uint32_t tid = threadIdx.x, ld4 = ld / 4;
  const f32x4* in = reinterpret_cast<const f32x4*>(src_rows + (uint64_t)jb.src * 64ull * ld);
  f32x4* out = reinterpret_cast<f32x4*>(dst_rows + (uint64_t)jb.dst * 64ull * ld);
  f32x4* rm = dst_rm ? reinterpret_cast<f32x4*>(dst_rm + (uint64_t)jb.dst * 64ull * ld) : nullptr;
  uint16_t* sh = dst_h ? dst_h + (uint64_t)jb.dst * 64ull * ld : nullptr;
  uint32_t my_id = 0xFFFFFFFFu;  // waves 0 and 1: the vec id of row tid % 64
  if (tid < 128u) my_id = src_ids[(uint64_t)jb.src * 64ull + (tid & 63u)];
  if (tid < 64u) dst_ids[(uint64_t)jb.dst * 64ull + tid] = my_id;
  float acc = 0.0f;  // wave 0: |x|^2 of row tid, wave 1: residual of row tid - 64
  constexpr uint32_t kPitch = kGatherCols4 + 1;
  for (uint32_t c0 = 0; c0 < ld4; c0 += kGatherCols4) {
    const uint32_t nc = ld4 - c0 < kGatherCols4 ? ld4 - c0 : kGatherCols4;  // (ld is a multiple of 64: nc is a multiple of 16)
    for (uint32_t i = tid; i < 64u * nc; i += 256u) {  // a piece's 64 rows by consecutive threads: 1 KiB contiguous in, 1 KiB contiguous out
      const uint32_t j = i / 64u, r = i % 64u;
      const f32x4 v = in[(uint64_t)(c0 + j) * 64 + r];
      out[(uint64_t)(c0 + j) * 64 + r] = v;
      tl[r * kPitch + j] = v;
    }
    lds_barrier();
    if (rm)
      for (uint32_t i = tid; i < 64u * kGatherCols4; i += 256u) {  // a row's float4s by consecutive threads
        const uint32_t r = i / kGatherCols4, j = i % kGatherCols4;
        if (j < nc) rm[(uint64_t)r * ld4 + c0 + j] = tl[r * kPitch + j];
      }
    if (sh)
      for (uint32_t i = tid; i < 32u * nc; i += 256u) {  // a shadow piece (16 columns x 32 rows) by the 64 lanes of a wave
        const uint32_t piece = i / 64u, l = i % 64u;
        const uint32_t r = (piece & 1u) * 32u + (l & 31u), g = (piece >> 1) * 2u + (l >> 5);  // row, group of 8 columns of this pass
        f16x8_t o;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x4 x = tl[r * kPitch + 2u * g + h];
#pragma unroll
          for (int u = 0; u < 4; ++u) o[4 * h + u] = (_Float16)x[u];  // v_cvt_f16_f32: RNE, inf / NaN preserved (row_to_f16)
        }
        *reinterpret_cast<f16x8_t*>(sh + ((uint64_t)(c0 / 2u) * 64u + i) * 8u) = o;  // piece (c0 / 4 + piece / 2, piece % 2), lane l
      }
    if (tid < 64u) {
      const f32x4* row = tl + tid * kPitch;
      for (uint32_t j = 0; j < nc; ++j) {
        const f32x4 v = row[j];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __fadd_rn(acc, __fmul_rn(v[u], v[u]));
      }
    } else if (tid < 128u && sh) {
      const f32x4* row = tl + (tid - 64u) * kPitch;
      for (uint32_t j = 0; j < nc; ++j) {
        const f32x4 v = row[j];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float dlt = v[u] - (float)(_Float16)v[u];
          acc = __fadd_rn(acc, __fmul_rn(dlt, dlt));
        }
      }
    }
    lds_barrier();
  }
  if (tid < 128u) {
    const bool holds_vector = my_id != 0xFFFFFFFFu;
    if (tid < 64u) xnorm[(uint64_t)jb.dst * 64ull + tid] = holds_vector ? acc : 0.0f;
    uint32_t top = holds_vector && acc == acc ? __float_as_uint(acc) : 0u;  // acc >= 0: bit order == value order
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const uint32_t other = (uint32_t)__shfl_xor((int)top, o);
      top = other > top ? other : top;
    }
    if ((tid & 63u) == 0 && top != 0u && (tid < 64u || sh)) atomicMax(tid < 64u ? xmax2_bits : rmax2_bits, top);
  }
}

// ---- vers_ivf_remove_batch: marking and in-place compaction of the lists that lose rows ------------------------------------------------
// The ids of a call become one bit per vec id; *bad != 0: one of them is >= n_total (nothing of the index has been written by then).
__global__ void remove_mark_ids_kernel(const uint64_t* ids, uint64_t m, uint64_t n_total, uint32_t* bitmap, uint32_t* bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint64_t v = ids[i];
  if (v >= n_total) { *bad = 1u; return; }
  atomicOr(&bitmap[v >> 5], 1u << (v & 31));
}

// One pass over row_ids: a stored row whose vec id is marked counts for its list and lowers the list's first tile that loses a row.
// The list of a storage row comes from the CURRENT offsets (the last list with list_off <= r: lists without storage -- another rank's --
// share their offset with the next one that has some), not from tile_list, which a re-layout leaves stale.
__global__ void remove_scan_rows_kernel(const uint32_t* row_ids, uint64_t cap_rows, const uint32_t* bitmap, uint64_t n_total, const uint32_t* list_off,
                                        uint32_t k, uint32_t* rm_cnt, uint32_t* first_tile) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < cap_rows; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t id = row_ids[r];
    if (id == 0xFFFFFFFFu || id >= n_total || !((bitmap[id >> 5] >> (id & 31)) & 1u)) continue;
    uint32_t lo = 0, hi = k;
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (list_off[mid] <= r) lo = mid;
      else hi = mid;
    }
    atomicAdd(&rm_cnt[lo], 1u);
    atomicMin(&first_tile[lo], (uint32_t)(r >> 6));
  }
}

// One list that loses rows: its first storage row (a tile boundary), its length before the call, its first tile (list-relative) with a marked row.
struct RemoveJob {
  uint32_t off, len, first;
};
constexpr uint32_t kRmWaves = 8;  // waves per block of remove_compact_kernel
constexpr uint32_t kRmCols4 = 4;  // float4 columns a wave holds in registers per step

// One BLOCK per job walks the list's tiles in ascending order from `first`.  Destination row j takes the j-th surviving row s(j): s is
// monotone and s(j) >= j, so the sources of a destination tile lie in that tile or behind it and the move is safe IN PLACE --
//   map  : the block gathers the next 64 survivors (windows of row_ids from the first source not yet consumed, a ballot scan over the
//          bitmap test) into LDS; row_ids[j0 .. j0+64) are written after the window reads (later windows start at s(j0+63)+1 >= j0+64).
//   rows : source and destination are both tile layout, and a float4 COLUMN of a tile is its own 1 KiB piece: rows move within their
//          column only.  Each wave owns the columns == its index (mod kRmWaves x kRmCols4 groups): it reads the 64 sources of a destination
//          piece (mostly runs of consecutive 16-byte pieces) into registers and then writes the whole 1 KiB piece -- all loads of a piece
//          precede its stores in the one wave that touches that column, and no other wave ever does.  One barrier pair per tile (the map).
// Rows [new length, old length) become slack: row_ids 0xFFFFFFFF and zeros, as gather_tiles_kernel writes it.
__global__ __launch_bounds__(kRmWaves * 64) void remove_compact_kernel(const RemoveJob* jobs, const uint32_t* bitmap, uint64_t n_total, uint32_t ld,
                                                                       float* rows, uint32_t* row_ids) {
  __shared__ uint32_t s_src[kWave], s_id[kWave], s_wsum[kRmWaves];
  __shared__ uint32_t s_pos;
  const RemoveJob jb = jobs[blockIdx.x];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t ld4 = ld / 4;
  f32x4* const base4 = reinterpret_cast<f32x4*>(rows) + (uint64_t)jb.off * ld4;  // tile t of the list: base4 + t * 64 * ld4
  uint32_t* const ids = row_ids + jb.off;
  uint32_t pos = jb.first * 64u;  // first source row (list-relative) not yet consumed; the same in every thread
  for (uint32_t j0 = jb.first * 64u; j0 < jb.len; j0 += 64u) {
    uint32_t have = 0;
    while (have < 64u && pos < jb.len) {
      const uint32_t idx = pos + tid;
      const uint32_t id = idx < jb.len ? ids[idx] : 0xFFFFFFFFu;
      const bool surv = id != 0xFFFFFFFFu && (id >= n_total || !((bitmap[id >> 5] >> (id & 31)) & 1u));
      const unsigned long long mask = __ballot(surv);
      const uint32_t pre = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      if (lane == 0) s_wsum[wv] = (uint32_t)__popcll(mask);
      __syncthreads();
      uint32_t woff = 0, total = 0;
#pragma unroll
      for (uint32_t w = 0; w < kRmWaves; ++w) {
        const uint32_t s = s_wsum[w];
        if (w < wv) woff += s;
        total += s;
      }
      const uint32_t p = have + woff + pre;
      if (surv && p < 64u) { s_src[p] = idx; s_id[p] = id; }
      if (surv && p == 63u) s_pos = idx + 1u;
      __syncthreads();
      if (have + total >= 64u) { pos = s_pos; have = 64u; }
      else { pos += kRmWaves * 64u; have += total; }
    }
    if (tid < 64u && tid >= have) s_src[tid] = 0xFFFFFFFFu;
    __syncthreads();
    if (tid < 64u) ids[j0 + tid] = s_src[tid] != 0xFFFFFFFFu ? s_id[tid] : 0xFFFFFFFFu;  // (j0 + 63 < round_up(len, 64) <= the list's capacity)
    const uint32_t src = s_src[lane], src0 = src != 0xFFFFFFFFu ? src : 0u;
    const f32x4* const sp = base4 + (uint64_t)(src0 >> 6) * 64u * ld4 + (src0 & 63u);
    f32x4* const dp = base4 + (uint64_t)(j0 >> 6) * 64u * ld4 + lane;
    for (uint32_t cb = wv * kRmCols4; cb < ld4; cb += kRmWaves * kRmCols4) {
      f32x4 v[kRmCols4];
#pragma unroll
      for (uint32_t u = 0; u < kRmCols4; ++u) {
        v[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (src != 0xFFFFFFFFu && cb + u < ld4) v[u] = sp[(uint64_t)(cb + u) * 64u];
      }
      __builtin_amdgcn_wave_barrier();  // every load of the pieces above is issued before the first store below
#pragma unroll
      for (uint32_t u = 0; u < kRmCols4; ++u)
        if (cb + u < ld4) dp[(uint64_t)(cb + u) * 64u] = v[u];
    }
    __syncthreads();  // the map of this tile is read by every wave until here
  }
}

// ---- vers_ivf_update_batch: mark, locate, overwrite in place, backward merge of the lists that gain rows (update_plan.hpp) ---------------
// slot[v] = index of the update of vec id v in the call (upd::kNone: none).  *bad |= 1: an id >= n_total; |= 2: an id twice (the exchange
// found the slot taken).  Nothing of the index has been written by then.
__global__ void update_mark_kernel(const uint64_t* ids, uint64_t m, uint64_t n_total, uint32_t* slot, uint32_t* bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint64_t v = ids[i];
  if (v >= n_total) { atomicOr(bad, 1u); return; }
  if (atomicExch(&slot[v], (uint32_t)i) != upd::kNone) atomicOr(bad, 2u);
}

// One pass over row_ids, as remove_scan_rows_kernel: a stored row whose vec id has update i either stays (its list is a32[i]: rel[i] = its
// position in the list) or moves: its bit in the removal bitmap, one more row leaving its list (and the list's first tile, list-relative,
// that loses one -- what remove_compact_kernel consumes), one more entering list a32[i], and the pair ((new list, vec id), i) appended for
// the sort.  Updates never met keep status 2 (the id is in no list).  Positions are list-relative: a re-layout may follow.
__global__ void update_locate_kernel(const uint32_t* row_ids, uint64_t cap_rows, const uint32_t* slot, uint64_t n_total, const uint32_t* list_off, uint32_t k,
                                     const uint32_t* a32, uint8_t* status, uint32_t* rel, uint32_t* bitmap, uint32_t* out_cnt, uint32_t* first_tile,
                                     uint32_t* in_cnt, uint32_t* n_mv, uint32_t mv_cap, uint64_t* mv_key, uint64_t* mv_val, uint32_t* old_of) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < cap_rows; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t id = row_ids[r];
    if (id == upd::kNone || id >= n_total) continue;
    const uint32_t i = slot[id];
    if (i == upd::kNone) continue;
    const uint32_t c = upd::list_of_row(list_off, k, r), a = a32[i];
    const uint32_t p = (uint32_t)(r - list_off[c]);
    const uint8_t s = upd::classify(c, a);
    status[i] = s;
    if (old_of) old_of[i] = c;  // (a handle sharded by cluster: this rank's word of the where round)
    if (s == upd::kStayed) { rel[i] = p; continue; }
    atomicOr(&bitmap[id >> 5], 1u << (id & 31));
    atomicAdd(&out_cnt[c], 1u);
    atomicMin(&first_tile[c], p >> 6);
    atomicAdd(&in_cnt[a], 1u);
    const uint32_t j = atomicAdd(n_mv, 1u);
    if (j >= mv_cap) continue;  // (a vec id stored twice: the host sees the count and refuses)
    mv_key[j] = ((uint64_t)a << 32) | id;
    mv_val[j] = i;
  }
}

// A handle sharded by cluster, after the where round: table [world][n + 1] holds, per rank, the list every vec id of the call lies in THERE
// (0xFFFFFFFF: in no list of that rank).  Every rank derives the same from it --
//   gstatus[i]  stayed (the claimed list is a32[i]) / moved / skipped (no claimer): the call's out_status
//   g_out / g_in  rows leaving / entering every list, whoever owns it: the new GLOBAL lengths
// and its own part: lstatus[i] = stayed only where THIS rank is the claimer (rel[i] is valid: update_locate_kernel met the row), moved only
// where this rank owns the new list -- then the pair ((new list, vec id), i) is appended for the sort, the row comes from the CALL's rows,
// wherever the old one lay -- and skipped otherwise.  *bad |= 1: an id claimed twice; |= 2: a claim by a rank that does not own the list.
__global__ void update_resolve_kernel(const uint32_t* table, uint32_t world, uint32_t me, const uint64_t* ids, uint32_t n, const uint8_t* owner, uint32_t k,
                                      const uint32_t* a32, uint8_t* gstatus, uint8_t* lstatus, uint32_t* g_out, uint32_t* g_in, uint32_t* n_mv, uint64_t* mv_key,
                                      uint64_t* mv_val, uint32_t* bad) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t who = upd::kNone, old = upd::kNone;
  for (uint32_t r = 0; r < world; ++r) {
    const uint32_t w = table[(uint64_t)r * ((uint64_t)n + 1u) + i];
    if (w == upd::kNone) continue;
    if (who != upd::kNone) { atomicOr(bad, 1u); continue; }
    if (w >= k || (uint32_t)owner[w] != r) { atomicOr(bad, 2u); continue; }
    who = r;
    old = w;
  }
  const uint32_t a = a32[i];
  uint8_t g = upd::kSkipped, l = upd::kSkipped;
  if (who != upd::kNone && a < k) {
    g = upd::classify(old, a);
    if (g == upd::kStayed) {
      if (who == me) l = upd::kStayed;
    } else {
      atomicAdd(&g_out[old], 1u);
      atomicAdd(&g_in[a], 1u);
      if ((uint32_t)owner[a] == me) {
        l = upd::kMoved;
        const uint32_t j = atomicAdd(n_mv, 1u);
        if (j < n) {
          mv_key[j] = ((uint64_t)a << 32) | (uint32_t)ids[i];
          mv_val[j] = i;
        }
      }
    }
  }
  gstatus[i] = g;
  lstatus[i] = l;
}

// mv_row[i] = the place of update i among the movers sorted by (new list, vec id)
__global__ void update_mover_rows_kernel(const uint64_t* vals_sorted, uint32_t n_mv, uint32_t* mv_row) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n_mv) mv_row[(uint32_t)vals_sorted[q]] = q;
}

// The staged chunk X [m][ldx] (zero-padded; updates i0 .. i0 + m of the call): a row that stays goes over its storage row, 16-byte piece by
// piece (tile[c4 * 64 + r]: nothing else of the tile is read or written); a row that moves is copied to its place in the movers' stage
// S [n_mv][ldx], where the merge finds the rows of a list side by side in ascending vec id.
__global__ void update_place_kernel(const float* X, uint32_t ldx, uint32_t ld, uint64_t i0, uint32_t m, const uint8_t* status, const uint32_t* a32,
                                    const uint32_t* rel, const uint32_t* mv_row, const uint32_t* list_off, float* rows, float* S) {
  const uint32_t ld4 = ld / 4, ldx4 = ldx / 4;
  const uint64_t total = (uint64_t)m * ld4;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t il = t / ld4, i = i0 + il;
    const uint32_t c4 = (uint32_t)(t % ld4);
    const uint8_t s = status[i];
    if (s == upd::kSkipped) continue;
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (c4 < ldx4) v = reinterpret_cast<const f32x4*>(X + il * ldx)[c4];
    if (s == upd::kStayed) {
      const uint64_t r = (uint64_t)list_off[a32[i]] + rel[i];
      *reinterpret_cast<f32x4*>(rows + blocked_index(r, c4 * 4, ld)) = v;
    } else if (c4 < ldx4) {
      reinterpret_cast<f32x4*>(S + (uint64_t)mv_row[i] * ldx)[c4] = v;
    }
  }
}

// pos[q] = #ids of the mover's new list (after the movers that leave it are gone: mid_len) below its vec id
__global__ void update_positions_kernel(const uint64_t* keys_sorted, uint32_t n_mv, const uint32_t* list_off, const uint32_t* mid_len, const uint32_t* row_ids,
                                        uint32_t* pos) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_mv) return;
  const uint32_t c = (uint32_t)(keys_sorted[q] >> 32), v = (uint32_t)keys_sorted[q];
  pos[q] = upd::insertion_point(row_ids + list_off[c], mid_len[c], v);
}

// One list that gains rows: its first storage row, its length after the movers left, the rows entering and where they start in the sorted order.
struct MergeJob {
  uint32_t off, len, n_in, in0;
};

// One BLOCK per job walks the list's destination tiles in DESCENDING order, from the last tile of the merged list down to the tile of the
// first insertion point; tiles in front of it are not touched.  Destination row j takes upd::merge_source(j): an old row s <= j of the list
// or a new row of S.  Every destination is >= its source, so the sources of a tile lie in that tile or in front of it, where nothing has
// been written yet, and the move is safe IN PLACE with remove_compact_kernel's discipline --
//   map  : wave 0 computes the tile's 64 sources and reads their vec ids into LDS; row_ids of the tile are written after the barrier behind
//          those reads (the tiles still to come read only rows in front of this tile).
//   rows : a float4 COLUMN of a tile is its own 1 KiB piece and rows move within their column only.  Each wave owns its columns: it reads
//          the 64 sources of a destination piece into registers and then writes the whole piece -- all loads of a piece precede its stores in
//          the one wave that touches that column.
// Rows behind the merged list in its last tile are slack: row_ids 0xFFFFFFFF and zeros.
__global__ __launch_bounds__(kRmWaves * 64) void update_merge_kernel(const MergeJob* jobs, const uint32_t* pos_all, const uint64_t* keys_sorted, const float* S,
                                                                     uint32_t ldx, uint32_t ld, float* rows, uint32_t* row_ids) {
  __shared__ uint32_t s_src[kWave], s_id[kWave];
  const MergeJob jb = jobs[blockIdx.x];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t ld4 = ld / 4, ldx4 = ldx / 4;
  f32x4* const base4 = reinterpret_cast<f32x4*>(rows) + (uint64_t)jb.off * ld4;
  const f32x4* const S4 = reinterpret_cast<const f32x4*>(S) + (uint64_t)jb.in0 * ldx4;
  uint32_t* const ids = row_ids + jb.off;
  const uint32_t* const pos = pos_all + jb.in0;
  const uint32_t t_first = upd::merge_first_tile(pos), t_last = upd::merge_last_tile(jb.len, jb.n_in);
  for (uint32_t T = t_last + 1u; T-- > t_first;) {
    if (tid < 64u) {
      const uint32_t src = upd::merge_source(pos, jb.n_in, jb.len, T * 64u + tid);
      uint32_t id = upd::kNone;
      if (src != upd::kNone) id = (src & upd::kNewBit) ? (uint32_t)keys_sorted[jb.in0 + (src & ~upd::kNewBit)] : ids[src];
      s_src[tid] = src;
      s_id[tid] = id;
    }
    __syncthreads();
    if (tid < 64u) ids[T * 64u + tid] = s_id[tid];  // (T * 64 + 63 < round_up(len + n_in, 64) <= the list's capacity)
    const uint32_t src = s_src[lane];
    const bool is_new = src != upd::kNone && (src & upd::kNewBit) != 0u, is_old = src != upd::kNone && !is_new;
    const uint32_t s0 = is_old ? src : 0u, t0 = is_new ? (src & ~upd::kNewBit) : 0u;
    const f32x4* const sp = base4 + (uint64_t)(s0 >> 6) * 64u * ld4 + (s0 & 63u);
    const f32x4* const np = S4 + (uint64_t)t0 * ldx4;
    f32x4* const dp = base4 + (uint64_t)T * 64u * ld4 + lane;
    for (uint32_t cb = wv * kRmCols4; cb < ld4; cb += kRmWaves * kRmCols4) {
      f32x4 v[kRmCols4];
#pragma unroll
      for (uint32_t u = 0; u < kRmCols4; ++u) {
        v[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (is_old && cb + u < ld4) v[u] = sp[(uint64_t)(cb + u) * 64u];
        if (is_new && cb + u < ldx4) v[u] = np[cb + u];  // (the stage's padding is zero; columns >= ldx of a stored row are zero)
      }
      __builtin_amdgcn_wave_barrier();  // every load of the pieces above is issued before the first store below
#pragma unroll
      for (uint32_t u = 0; u < kRmCols4; ++u)
        if (cb + u < ld4) dp[(uint64_t)(cb + u) * 64u] = v[u];
    }
    __syncthreads();  // the map of this tile is read by every wave until here
  }
}

}  // namespace vers

namespace vers {
namespace ivf {

// test hook: every storage row that holds no vector (slack behind the lists, tile padding) gets `value` in all its columns,
// then the derived arrays (|x|^2, fp16 shadow, residual) are rebuilt -- what uninitialised device memory may look like
static __global__ void poison_slack_kernel(float* rows, uint32_t ld, const uint32_t* row_ids, uint64_t n_rows, float value) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t r = t / (ld / 4);
  const uint32_t j = (uint32_t)(t % (ld / 4));
  if (r >= n_rows || row_ids[r] != 0xFFFFFFFFu) return;
  reinterpret_cast<f32x4*>(rows + (r >> 6) * 64ull * ld)[(uint64_t)j * 64 + (r & 63)] = f32x4{value, value, value, value};
}
int32_t poison_slack(vers_ivf* h, float value, hipStream_t st) {
  if (h->cap_rows == 0) return VERS_OK;
  const uint64_t work = h->cap_rows * (h->ld / 4);
  hipLaunchKernelGGL(poison_slack_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, h->rows.as<float>(), h->ld,
                     (const uint32_t*)h->row_ids.as<uint32_t>(), h->cap_rows, value);
  VERS_HIP_TRY(hipGetLastError());
  return VERS_OK;
}

// The int8 head of the whole index (head_filter.hip.h) from the rows as the shadow rounds them: the maximum over the head columns of the
// stored rows -> the scale; the head; its measured residual.  H = option "pre_head_cols" (default 384) in multiples of 64, clipped to
// ld - 64 (a boundary needs a step left to save); no head below 256 columns, on a sharded handle, for the cosine distance or without
// the shadow.  Optional memory like the shadow: a failed allocation, or a non-finite maximum or residual, leaves head_valid false and
// every search as it was.  Synchronises st (build, compact and the test hooks: never a search).
int32_t build_head(vers_ivf* h, hipStream_t st) {
  h->head_valid = false;
  h->head_backoff = 0;
  if (h->head_watch) *h->head_watch = 0;
  uint32_t H = (uint32_t)std::max<int64_t>(0, std::min<int64_t>(opt_get("pre_head_cols", 384), kHeadMaxCols)) / 64u * 64u;
  if (h->ld >= 64u) H = std::min<uint32_t>(H, (h->ld - 64u) / 64u * 64u);
  else H = 0;
  const bool want = opt_get("pre_head", kPreHeadDefault) != 0 && H >= kHeadMinCols && h->world == 1 && h->metric == 0 && shadow_mode() != 0 && h->shadow_valid &&
                    h->pre_misc.p != nullptr && h->cap_rows != 0;
  if (!want) {
    h->rows_h8.release();
    h->head_cols = 0;
    return VERS_OK;
  }
  if (!h->head_ctr.p) {
    if (int32_t rc = h->head_ctr.reserve(64)) return rc;
    VERS_HIP_TRY(hipMemset(h->head_ctr.p, 0, 64));
  }
  if (!h->head_watch) {
    VERS_HIP_TRY(hipHostMalloc((void**)&h->head_watch, 64, hipHostMallocDefault));
    *h->head_watch = 0;
  }
  const size_t need = (size_t)h->cap_rows * H;
  if (need > h->rows_h8.cap) {
    h->rows_h8.release();
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    void* ph = nullptr;
    if (need + (size_t(4) << 30) <= free_b && hipMalloc(&ph, need) == hipSuccess) { h->rows_h8.p = ph; h->rows_h8.cap = need; dev_mem_account((int64_t)need); }
    else (void)hipGetLastError();
  }
  h->head_cols = H;
  if (h->rows_h8.p == nullptr) return VERS_OK;
  uint32_t* misc = h->pre_misc.as<uint32_t>();
  VERS_HIP_TRY(hipMemsetAsync(misc + kHeadMiscMax, 0, 2 * sizeof(uint32_t), st));
  const unsigned row_blocks = (unsigned)((h->cap_rows + 255) / 256);
  hipLaunchKernelGGL(head_max_kernel, dim3(row_blocks), dim3(256), 0, st, (const float*)h->rows.as<float>(), h->ld, (const uint32_t*)h->row_ids.as<uint32_t>(),
                     h->cap_rows, H, misc + kHeadMiscMax);
  hipLaunchKernelGGL(head_write_kernel, dim3((unsigned)((h->cap_rows * (H / 16u) + 255) / 256)), dim3(256), 0, st, (const float*)h->rows.as<float>(), h->ld,
                     (const uint32_t*)h->row_ids.as<uint32_t>(), h->cap_rows, H, (const uint32_t*)(misc + kHeadMiscMax), h->rows_h8.as<int8_t>());
  hipLaunchKernelGGL(head_resid_kernel, dim3(row_blocks), dim3(256), 0, st, (const float*)h->rows.as<float>(), h->ld, (const uint32_t*)h->row_ids.as<uint32_t>(),
                     h->cap_rows, H, (const uint32_t*)(misc + kHeadMiscMax), misc + kHeadMiscRh2);
  VERS_HIP_TRY(hipGetLastError());
  float mr[2] = {0.0f, 0.0f};
  VERS_HIP_TRY(hipMemcpyAsync(mr, misc + kHeadMiscMax, sizeof(mr), hipMemcpyDeviceToHost, st));
  VERS_HIP_TRY(hipStreamSynchronize(st));
  h->head_valid = std::isfinite(mr[0]) && std::isfinite(mr[1]) && std::isfinite(head_scale(mr[0]));
  return VERS_OK;
}

// The lists' sub-cluster balls (ball_filter.hip.h) from the fp16 shadow and the stored |x|^2: a block per list slot.  Wanted where the
// int8 head is wanted (squared L2, unsharded, a valid shadow) and option "pre_ball" is not 0; the cut of the farthest-point pass is option
// "pre_ball_cut" in thousandths of sqrt(max |x|^2) (default 900).  Optional memory like the head: a failed allocation -- of any of
// its buffers, the counters included -- leaves balls_valid false, silently.  The derive pass writes at the cap of 32 places per list into
// scratch; what it kept is packed into [sum of k_c][ld] with ball_off / ball_cnt per slot and the scratch released.  When fewer than 1/8 of the non-empty lists got balls -- rows without cluster contrast -- everything is released:
// such an index pays nothing per batch.  Synchronises st.
int32_t build_balls(vers_ivf* h, hipStream_t st) {
  h->balls_valid = false;
  h->ball_lists = 0;
  h->ball_sub = 0;
  const uint32_t k = h->k;
  const bool want = opt_get("pre_ball", kPreBallDefault) != 0 && opt_get("pre_head", kPreHeadDefault) != 0 && h->world == 1 && h->metric == 0 && shadow_mode() != 0 && h->shadow_valid &&
                    h->rows_bf.p != nullptr && h->pre_misc.p != nullptr && h->xnorm.p != nullptr && h->cap_rows != 0 && k != 0 && h->ld >= 64u && h->ld <= kBallMaxLd &&
                    h->slot_off.p != nullptr && h->slot_len.p != nullptr;
  auto drop = [&]() {
    (void)hipGetLastError();
    h->ball_cent.release();
    h->ball_f.release();
    h->ball_cnt.release();
    h->ball_off.release();
    return VERS_OK;
  };
  if (!want) return drop();
  // optional memory, every piece of it: whatever cannot be had leaves the handle without balls, silently
  auto optional = [&](DevBuf& b, size_t need) {
    if (need <= b.cap && b.p != nullptr) return true;
    b.release();
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    void* p = nullptr;
    if (need + (size_t(4) << 30) <= free_b && hipMalloc(&p, need) == hipSuccess) { b.p = p; b.cap = need; dev_mem_account((int64_t)need); return true; }
    (void)hipGetLastError();
    return false;
  };
  if (!h->ball_ctr.p) {
    if (!optional(h->ball_ctr, 64)) return drop();
    if (hipMemset(h->ball_ctr.p, 0, 64) != hipSuccess) { h->ball_ctr.release(); return drop(); }
  }
  // the derive pass writes at the cap, kBallMax places per list; what it kept is packed behind it and the cap-sized scratch released
  DevBuf cent_cap, f_cap;
  if (!optional(cent_cap, (size_t)k * kBallMax * h->ld * sizeof(uint16_t)) || !optional(f_cap, (size_t)k * kBallMax * 3 * sizeof(float)) ||
      !optional(h->ball_cnt, (size_t)k * sizeof(uint32_t)) || !optional(h->ball_off, (size_t)k * sizeof(uint32_t)))
    return drop();
  const double cut = (double)std::max<int64_t>(1, std::min<int64_t>(opt_get("pre_ball_cut", 900), 4000)) / 1000.0;
  const size_t lds = ball_derive_lds_bytes(h->ld);
  VERS_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(ball_derive_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(ball_derive_kernel, dim3(k), dim3(kBallDeriveThreads), lds, st, (const uint16_t*)h->rows_bf.as<uint16_t>(), h->ld, (const uint32_t*)h->slot_off.as<uint32_t>(),
                     (const uint32_t*)h->slot_len.as<uint32_t>(), (const float*)h->xnorm.as<float>(), (const uint32_t*)h->pre_misc.as<uint32_t>(), (float)(cut * cut),
                     cent_cap.as<uint16_t>(), f_cap.as<float>(), h->ball_cnt.as<uint32_t>());
  VERS_HIP_TRY(hipGetLastError());
  std::vector<uint32_t> cnt(k, 0u), len(k, 0u), boff(k, 0u);
  VERS_HIP_TRY(hipMemcpyAsync(cnt.data(), h->ball_cnt.p, (size_t)k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  VERS_HIP_TRY(hipMemcpyAsync(len.data(), h->slot_len.p, (size_t)k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  VERS_HIP_TRY(hipStreamSynchronize(st));
  uint32_t with = 0, non_empty = 0;
  uint64_t sub = 0;
  for (uint32_t c = 0; c < k; ++c) {
    non_empty += len[c] != 0u ? 1u : 0u;
    with += cnt[c] != 0u ? 1u : 0u;
    boff[c] = (uint32_t)sub;
    sub += std::min<uint32_t>(cnt[c], kBallMax);
  }
  if (with == 0u || 8ull * with < non_empty) return drop();
  if (!optional(h->ball_cent, (size_t)sub * h->ld * sizeof(uint16_t)) || !optional(h->ball_f, (size_t)sub * 3 * sizeof(float))) return drop();
  VERS_HIP_TRY(hipMemcpyAsync(h->ball_off.p, boff.data(), (size_t)k * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(ball_pack_kernel, dim3(k), dim3(256), 0, st, (const uint16_t*)cent_cap.as<uint16_t>(), (const float*)f_cap.as<float>(), (const uint32_t*)h->ball_cnt.as<uint32_t>(),
                     (const uint32_t*)h->ball_off.as<uint32_t>(), h->ld, h->ball_cent.as<uint16_t>(), h->ball_f.as<float>());
  VERS_HIP_TRY(hipGetLastError());
  VERS_HIP_TRY(hipStreamSynchronize(st));  // (boff and the scratch go out of scope here)
  h->ball_lists = with;
  h->ball_sub = sub;
  h->balls_valid = true;
  return VERS_OK;
}

// |x|^2 of storage rows [r_begin, r_end) for the matrix-core list scan; a full refresh also resets the maximum
int32_t refresh_norms(vers_ivf* h, uint64_t r_begin, uint64_t r_end, hipStream_t st) {
  if (int32_t rc = h->pre_misc.reserve(64)) return rc;
  if (!h->prune_ctr.p) {  // the list scan's early-abandon totals: zeroed HERE, synchronously, under the exclusive lock -- scans on any stream only ever add
    if (int32_t rc = h->prune_ctr.reserve(64)) return rc;
    VERS_HIP_TRY(hipMemset(h->prune_ctr.p, 0, 64));
  }
  const bool full = r_begin == 0 && r_end == h->cap_rows;
  if (full) {
    if (int32_t rc = h->xnorm.reserve((h->cap_rows ? h->cap_rows : 1) * sizeof(float))) return rc;
    VERS_HIP_TRY(hipMemsetAsync(h->pre_misc.p, 0, 64, st));
    for (auto& w : h->pool)  // a new index: ranked lists computed ahead belong to the old centroids (the caller holds the handle exclusively)
      for (auto& a : w->ahead) a.valid = false;
  }
  // fp16 shadow of the rows for the matrix-core list scan of batches (prescan.hip.h): on unless VERS_SHADOW=0 /
  // vers_set_option("shadow", 0) at build / upload time.
  const bool shadow = shadow_mode() != 0;
  if (full) h->shadow_valid = false;
  h->head_valid = false;  // rows change: a full refresh builds the int8 head again (below), a partial one leaves it invalid
  h->balls_valid = false;  // (the lists' balls likewise)
  if (shadow) {
    if (full) {
      const size_t need = (h->cap_rows ? h->cap_rows : 1) * (size_t)h->ld * sizeof(uint16_t);
      if (need > h->rows_bf.cap) {  // optional memory: without it (or with less than 4 GB left for the searches' scratch) the f32 rows stay in charge
        h->rows_bf.release();
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        void* pbf = nullptr;
        if (need + (size_t(4) << 30) <= free_b && hipMalloc(&pbf, need) == hipSuccess) { h->rows_bf.p = pbf; h->rows_bf.cap = need; dev_mem_account((int64_t)need); }
        else (void)hipGetLastError();
      }
      h->shadow_valid = h->rows_bf.p != nullptr && h->rows_bf.cap >= need;
      h->shadow_off = false; h->shadow_queries = 0;  // (the failure counter in pre_misc was just zeroed)
      if (!h->fail_watch) VERS_HIP_TRY(hipHostMalloc((void**)&h->fail_watch, 64, hipHostMallocDefault));
      *h->fail_watch = 0;
    }
    if (r_end > r_begin && h->shadow_valid) {
      const uint64_t work = (r_end - r_begin) * (h->ld / 8);
      hipLaunchKernelGGL(rows_to_f16_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, h->rows.as<float>(), h->ld, r_begin, r_end,
                         h->rows_bf.as<uint16_t>());
      hipLaunchKernelGGL(shadow_residual_kernel, dim3((unsigned)((r_end - r_begin + 255) / 256)), dim3(256), 0, st, h->rows.as<float>(), h->ld,
                         h->row_ids.as<uint32_t>(), r_begin, r_end, h->pre_misc.as<uint32_t>() + 2);
      VERS_HIP_TRY(hipGetLastError());
    }
  } else {
    h->shadow_valid = false;  // rows changed without their shadow following
    if (full) h->rows_bf.release();
  }
  {
    // option "rowmajor": -1 (default) = whenever it fits (vers_ivf::rows_rm) unless option "memory" is 1 (compact: ONE f32 copy of the
    // rows -- the tiles; the exact finish then gathers its survivors from them in 16-byte pieces), 0 never, 1 always
    const int rm_opt = (int)opt_get("rowmajor", -1);
    const int rm_mode = rm_opt < 0 && opt_get("memory", 0) == 1 ? 0 : rm_opt;
    if (full) {
      size_t free_b = 0, total_b = 0;
      (void)hipMemGetInfo(&free_b, &total_b);
      const size_t need = (h->cap_rows ? h->cap_rows : 1) * (size_t)h->ld * sizeof(float);
      const bool want = rm_mode == 1 || (rm_mode < 0 && need <= total_b / 4);
      if (!want || need > h->rows_rm.cap) h->rows_rm.release();
      if (want && h->rows_rm.p == nullptr) {  // optional memory: a failed allocation leaves the tile gather in charge
        void* prm = nullptr;
        if (need + (size_t(2) << 30) <= free_b && hipMalloc(&prm, need) == hipSuccess) { h->rows_rm.p = prm; h->rows_rm.cap = need; dev_mem_account((int64_t)need); }
        else (void)hipGetLastError();
      }
    }
    if (r_end > r_begin && h->rows_rm.p)
      if (int32_t rc = launch_from_blocked(h->rows.as<float>(), h->ld, r_begin, r_end - r_begin, h->ld, h->rows_rm.as<float>() + r_begin * (size_t)h->ld,
                                           h->ld, st))
        return rc;
  }
  if (r_end > r_begin) {
    hipLaunchKernelGGL(blocked_row_norms_kernel, dim3((unsigned)((r_end - r_begin + 255) / 256)), dim3(256), 0, st, h->rows.as<float>(), h->ld,
                       h->row_ids.as<uint32_t>(), r_begin, r_end, h->xnorm.as<float>(), h->pre_misc.as<uint32_t>());
    VERS_HIP_TRY(hipGetLastError());
  }
  if (full) {
    if (int32_t rc = build_head(h, st)) return rc;
    return build_balls(h, st);
  }
  return VERS_OK;
}

// ---- build: storage layout, row placement, k-means ------------------------------------------------------------
// host wall clock of a phase of build_index, added to BuildStats::*field on scope exit (vers_build_phases)
struct PhaseClock {
  double BuildStats::*field;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit PhaseClock(double BuildStats::*f) : field(f) {}
  ~PhaseClock() { build_stats_add(field, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()); }
};
// How the rows of a build are spread over processes.  comm == nullptr: one process holds all n rows.
struct BuildShard {
  const vers_comm_t* comm = nullptr;
  uint32_t rank = 0, world = 1;
  uint64_t row_begin = 0;  // global index of this process's first row
  uint64_t n_total = 0;    // rows over all processes
  const struct Agreement* agree = nullptr;  // (multi-process builds: made by build_common before the first collective)
};

int32_t comm_rc(int32_t rc, const char* what) {
  if (rc) return fail(VERS_ERR_COMM, std::string("vers_comm_t::") + what + " reported failure (status " + std::to_string(rc) + ")");
  return VERS_OK;
}

// Failure propagation of the row-sharded build: every callback is a rendezvous, so a rank that returned early (a failed
// allocation, a HIP error in its assign pass) would leave its peers blocked inside the next one -- under RCCL a spinning
// kernel until the watchdog fires.  At the points where a rank can fail on its own, right before the ranks next meet, all
// ranks exchange how they fared (one 4-byte all_gather) and LEAVE TOGETHER when anyone failed.  (What cannot be agreed on
// is a failure of the communicator itself: the host must abort the process group when any rank returns non-zero.)
// The 4 + 4 W bytes it needs are allocated ONCE per build, before the first collective (Agreement::init: a failure there is
// returned before any rank has entered a rendezvous -- the host aborts the group as for any non-zero return): agree() itself
// never allocates, and it ALWAYS enters the all_gather -- with its error code when the local staging copy failed -- so that
// an out-of-memory rank, the very situation it exists for, cannot strand its peers inside the collective.
struct Agreement {
  const vers_comm_t* cm = nullptr;
  uint32_t W = 1;
  DevBuf mine, all;
  int32_t init(const vers_comm_t* comm, uint32_t world) {
    cm = comm; W = world;
    if (cm == nullptr || W <= 1) return VERS_OK;
    if (int32_t rc = mine.reserve(16)) return rc;
    if (int32_t rc = all.reserve(16 * (size_t)W)) return rc;
    VERS_HIP_TRY(hipMemset(mine.p, 0, 16));
    return VERS_OK;
  }
  int32_t operator()(int32_t my_rc, const char* where) const {
    if (cm == nullptr || W <= 1) return my_rc;
    int32_t word = my_rc;
    bool staged = hipMemcpy(mine.p, &word, 4, hipMemcpyHostToDevice) == hipSuccess;
    if (!staged) {  // (the device is in trouble: say so with whatever still works, then meet the peers all the same)
      (void)hipGetLastError();
      staged = hipMemset(mine.p, 0xFF, 4) == hipSuccess;
      if (!staged) (void)hipGetLastError();
      if (!my_rc) my_rc = fail(VERS_ERR_HIP, "hipMemcpy failed while staging the agreement word");
    }
    if (int32_t rc = comm_rc(cm->all_gather(cm->ctx, mine.p, all.p, 4), "all_gather")) return my_rc ? my_rc : rc;
    std::vector<int32_t> got(W, 0);
    if (hipMemcpy(got.data(), all.p, 4 * (size_t)W, hipMemcpyDeviceToHost) != hipSuccess) return my_rc ? my_rc : fail(VERS_ERR_HIP, "hipMemcpy failed");
    if (my_rc) return my_rc;
    for (uint32_t r = 0; r < W; ++r)
      if (got[r]) return fail(VERS_ERR_COMM, std::string("rank ") + std::to_string(r) + " failed in " + where + " (status " + std::to_string(got[r]) + "): every rank leaves the build");
    return VERS_OK;
  }
};

// Storage plan from the GLOBAL list lengths: owners (LPT when sharded), offsets and capacities of the owned lists,
// device tables, zeroed row ids.
// The storage rule, shared by plan_storage and vers_ivf_compact: offsets and capacities of the lists this rank owns (h_owner / rank),
// lists in ascending order, each starting on a tile boundary; another rank's list gets no storage.  *total = storage rows.
// (all_mine: the plan of k lists this rank owns every one of, whatever h_owner says of the CURRENT lists -- vers_ivf_recluster sizes the
// storage of its new lists before the handle learns of them)
static int32_t plan_capacities(const vers_ivf* h, const uint32_t* lens, uint32_t k, std::vector<uint32_t>& offs, std::vector<uint32_t>& caps,
                               uint64_t* total, bool all_mine = false) {
  offs.assign(k, 0);
  caps.assign(k, 0);
  uint64_t off = 0;
  for (uint32_t c = 0; c < k; ++c) {
    const uint32_t len = lens[c];
    const bool mine = all_mine || h->h_owner[c] == h->rank;
    // slack for `add` behind the list: 1/16 of its length, at least 8 rows, then up to the tile boundary the next list starts on.
    // (Rounds 1-5 kept at least 64: at k = 65536 over 6.25M rows -- lists of ~95 rows -- that alone doubled the storage; a list
    // that outgrows its slack is re-laid-out with 1/8 of head-room, relayout().)
    const uint32_t cap = mine ? round_up(len + std::max<uint32_t>(8u, len / 16u), 64u) : 0u;
    offs[c] = (uint32_t)off;
    caps[c] = cap;
    off += cap;
    if (off > 0xFFFFFFFFull) return fail(VERS_ERR_INVALID, "more than 2^32-1 storage rows on one GPU");
  }
  *total = off;
  return VERS_OK;
}
// Slot tables from h_len / h_off: longest lists first (stable: ties by index); add() changes lengths by one at a time, the order is kept as it is
static int32_t write_slot_tables(vers_ivf* h, uint32_t k) {
  std::vector<uint32_t> ord(k), so(k ? k : 1), sl(k ? k : 1);
  for (uint32_t c = 0; c < k; ++c) ord[c] = c;
  std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return h->h_len[x] > h->h_len[y]; });
  h->h_slot.assign(k, 0);
  for (uint32_t i = 0; i < k; ++i) { h->h_slot[ord[i]] = i; so[i] = h->h_off[ord[i]]; sl[i] = h->h_len[ord[i]]; }
  if (int32_t rc = h->list_slot.reserve((k ? k : 1) * sizeof(uint32_t))) return rc;
  if (int32_t rc = h->slot_off.reserve((k ? k : 1) * sizeof(uint32_t))) return rc;
  if (int32_t rc = h->slot_len.reserve((k ? k : 1) * sizeof(uint32_t))) return rc;
  if (k) {
    VERS_HIP_TRY(hipMemcpy(h->list_slot.p, h->h_slot.data(), (size_t)k * 4, hipMemcpyHostToDevice));
    VERS_HIP_TRY(hipMemcpy(h->slot_off.p, so.data(), (size_t)k * 4, hipMemcpyHostToDevice));
    VERS_HIP_TRY(hipMemcpy(h->slot_len.p, sl.data(), (size_t)k * 4, hipMemcpyHostToDevice));
  }
  return VERS_OK;
}
// tile_list from h_off / h_cap / cap_rows
static int32_t write_tile_list(vers_ivf* h, uint32_t k) {
  std::vector<uint32_t> tl((size_t)(h->cap_rows / 64) ? (size_t)(h->cap_rows / 64) : 1, 0u);
  for (uint32_t c = 0; c < k; ++c)
    for (uint32_t r = 0; r < h->h_cap[c]; r += 64) tl[(h->h_off[c] + r) / 64] = c;
  if (int32_t rc = h->tile_list.reserve(tl.size() * sizeof(uint32_t))) return rc;
  VERS_HIP_TRY(hipMemcpy(h->tile_list.p, tl.data(), tl.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  return VERS_OK;
}

int32_t plan_storage(vers_ivf* h, const uint32_t* lens, uint32_t k, hipStream_t st) {
  h->h_len.assign(lens, lens + k);
  uint64_t off = 0;
  h->max_len = 0;
  h->h_owner.assign(k, 0);
  if (h->world > 1) {
    std::vector<uint64_t> l64(h->h_len.begin(), h->h_len.end());
    shard_plan(l64.data(), k, h->world, h->h_owner.data());
  }
  if (int32_t rc = plan_capacities(h, h->h_len.data(), k, h->h_off, h->h_cap, &off)) return rc;
  for (uint32_t c = 0; c < k; ++c) h->max_len = std::max(h->max_len, h->h_len[c]);
  if (int32_t rc = h->owner.reserve(k ? k : 1)) return rc;
  if (k) VERS_HIP_TRY(hipMemcpyAsync(h->owner.p, h->h_owner.data(), k, hipMemcpyHostToDevice, st));
  if (int32_t rc = write_slot_tables(h, k)) return rc;
  h->set_len_asc_prefix();
  h->cap_rows = off;
  if (int32_t rc = write_tile_list(h, k)) return rc;
  if (int32_t rc = h->rows.reserve((off ? off : 1) * (size_t)h->ld * sizeof(float))) return rc;
  if (int32_t rc = h->row_ids.reserve((off ? off : 1) * sizeof(uint32_t))) return rc;
  if (int32_t rc = h->list_off.reserve((k ? k : 1) * sizeof(uint32_t))) return rc;
  if (int32_t rc = h->list_len.reserve((k ? k : 1) * sizeof(uint32_t))) return rc;
  VERS_HIP_TRY(hipMemsetAsync(h->row_ids.p, 0xFF, (off ? off : 1) * sizeof(uint32_t), st));
  if (k) {
    VERS_HIP_TRY(hipMemcpyAsync(h->list_off.p, h->h_off.data(), (size_t)k * 4, hipMemcpyHostToDevice, st));
    VERS_HIP_TRY(hipMemcpyAsync(h->list_len.p, h->h_len.data(), (size_t)k * 4, hipMemcpyHostToDevice, st));
  }
  return VERS_OK;
}

// Everything of the index that derives from h->centroids and the stored rows: centroids in the scan layout and as
// MFMA operands, |c|^2, |x|^2.  The index is complete (and the stream idle) on return.
int32_t finish_index(vers_ivf* h, uint32_t k, uint64_t n_total, hipStream_t st) {
  VERS_HIP_TRY(hipStreamSynchronize(st));  // (the row placement queued ahead belongs to the install phase's clock)
  PhaseClock derive_clock(&BuildStats::derive_ms);
  if (int32_t rc = h->centroids_b.reserve(std::max<uint64_t>(1, blocked_floats(k, h->ld)) * sizeof(float))) return rc;
  if (int32_t rc = launch_to_blocked(h->centroids.as<float>(), h->ldx, h->d, k, h->centroids_b.as<float>(), h->ld, st)) return rc;
  h->k_pad = round_up(k ? k : 1, kGemmBN);
  if (int32_t rc = h->centroids_g.reserve((size_t)h->k_pad * h->ldq * sizeof(float))) return rc;
  if (int32_t rc = h->cnorm.reserve((size_t)h->k_pad * sizeof(float))) return rc;
  if (int32_t rc = h->coarse_stat.reserve(16)) return rc;
  VERS_HIP_TRY(hipMemsetAsync(h->centroids_g.p, 0, (size_t)h->k_pad * h->ldq * sizeof(float), st));
  VERS_HIP_TRY(hipMemsetAsync(h->coarse_stat.p, 0, 16, st));
  if (int32_t rc = launch_stage_queries(h->centroids.as<float>(), h->ldx, h->d, h->centroids_g.as<float>(), h->ldq, k, 1, st)) return rc;
  hipLaunchKernelGGL(row_norms_kernel, dim3((h->k_pad + 255) / 256), dim3(256), 0, st, h->centroids_g.as<float>(), h->ldq, k, h->k_pad,
                     h->cnorm.as<float>());
  VERS_HIP_TRY(hipGetLastError());
  {  // bf16 hi | lo halves of the same matrix: the N operand of the batched coarse quantiser's bf16x3 contraction
    const size_t ne = (size_t)h->k_pad * h->ldq;
    if (int32_t rc = h->centroids_gs.reserve(2 * ne * sizeof(uint16_t))) return rc;
    VERS_HIP_TRY(launch_split_bf16(h->centroids_g.as<float>(), ne, h->centroids_gs.as<__bf16>(), h->centroids_gs.as<__bf16>() + ne, st));
  }
  std::vector<float> cn(k ? k : 1, 0.0f);
  if (k) VERS_HIP_TRY(hipMemcpyAsync(cn.data(), h->cnorm.p, (size_t)k * sizeof(float), hipMemcpyDeviceToHost, st));
  VERS_HIP_TRY(hipStreamSynchronize(st));
  h->cmax2 = 0.0f;
  for (uint32_t c = 0; c < k; ++c) h->cmax2 = std::max(h->cmax2, cn[c]);  // NaN centroids never raise it; they fail the certificate
  h->k = k;
  h->n_total = n_total;
  {  // diagnosis (option "poison_slack_bits"): every new index starts with that value in the rows that hold no vector
    const int64_t poison = opt_get("poison_slack_bits", -1);  // (the f32 bit pattern: 0x7fc00000 NaN, 0x7f800000 inf, ...)
    if (poison >= 0 && h->cap_rows) {
      const uint32_t pbits = (uint32_t)poison;
      float v;
      std::memcpy(&v, &pbits, sizeof(v));
      const uint64_t work = h->cap_rows * (h->ld / 4);
      hipLaunchKernelGGL(poison_slack_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, h->rows.as<float>(), h->ld,
                         (const uint32_t*)h->row_ids.as<uint32_t>(), h->cap_rows, v);
      VERS_HIP_TRY(hipGetLastError());
    }
  }
  if (int32_t rc = refresh_norms(h, 0, h->cap_rows, st)) return rc;
  // |x|^2, max |x|^2 and the optional shadow were queued on `st`; searches run on other (possibly non-blocking)
  // streams and a certificate evaluated against a stale maximum would be unsound: the index is complete on return
  VERS_HIP_TRY(hipStreamSynchronize(st));
  return VERS_OK;
}

// install_index's steps around plan_storage, before finish_index.  group_for_install: the cluster-sorted order of the rows (sorted [n], counts |
// starts in h->km.counts) and the list lengths on the host; nothing of the index is touched.  place_rows: the rows into the tiles of the plan
// plan_storage has just made of those lengths, row_ids = the rows' positions in X.
static int32_t group_for_install(vers_ivf* h, uint64_t n, const uint32_t* d_assign, uint32_t k, DevBuf& sorted, std::vector<uint32_t>& lens, hipStream_t st) {
  if (int32_t rc = sorted.reserve((n ? n : 1) * sizeof(uint32_t))) return rc;
  if (int32_t rc = h->km.counts.reserve((2 * (size_t)k + 2) * sizeof(uint32_t))) return rc;
  uint32_t* counts = h->km.counts.as<uint32_t>();
  if (int32_t rc = km_group(d_assign, (uint32_t)n, k, sorted.as<uint32_t>(), counts, counts + k, h->km, st)) return rc;
  lens.assign(k ? k : 1, 0);
  if (k) VERS_HIP_TRY(hipMemcpyAsync(lens.data(), counts, (size_t)k * 4, hipMemcpyDeviceToHost, st));
  VERS_HIP_TRY(hipStreamSynchronize(st));
  return VERS_OK;
}
static int32_t place_rows(vers_ivf* h, const float* X, uint32_t ldx, uint64_t n, const uint32_t* d_assign, uint32_t k, const DevBuf& sorted,
                          hipStream_t st) {
  const uint32_t* starts = h->km.counts.as<uint32_t>() + k;
  if (n) {
    if (h->cap_rows >= 64) {  // whole destination tiles through LDS; (the float4-wise placement of round 1 is kept for indexes of less than one tile)
      const size_t lds = 64 * (size_t)(kGatherCols4 + 1) * sizeof(f32x4);
      if (int32_t rc = scan_prepare_launch(gather_tiles_kernel, lds)) return rc;
      hipLaunchKernelGGL(gather_tiles_kernel, dim3((unsigned)(h->cap_rows / 64)), dim3(256), lds, st, X, ldx, h->d, h->ld, sorted.as<uint32_t>(),
                         (const uint32_t*)starts, h->list_off.as<uint32_t>(), h->list_len.as<uint32_t>(), h->tile_list.as<uint32_t>(),
                         h->rows.as<float>(), h->row_ids.as<uint32_t>());
    } else
    hipLaunchKernelGGL(gather_rows_kernel, dim3(h->n_cu * 8), dim3(256), 0, st, X, ldx, h->d, h->ld, sorted.as<uint32_t>(), d_assign, starts,
                       h->list_off.as<uint32_t>(), h->world > 1 ? h->owner.as<uint8_t>() : (const uint8_t*)nullptr, h->rank, n,
                       h->rows.as<float>(), h->row_ids.as<uint32_t>());
    VERS_HIP_TRY(hipGetLastError());
  }
  return VERS_OK;
}
// index from (X in vec_id order -- ALL rows in this process --, centroids already in h->centroids, device assignments);
// with vers_ivf_set_shard only the owned lists are stored.
int32_t install_index(vers_ivf* h, const float* X, uint32_t ldx, uint64_t n, const uint32_t* d_assign, uint32_t k,
                      hipStream_t st) {
  DevBuf sorted;
  std::vector<uint32_t> lens;
  if (int32_t rc = group_for_install(h, n, d_assign, k, sorted, lens, st)) return rc;
  if (int32_t rc = plan_storage(h, lens.data(), k, st)) return rc;
  if (int32_t rc = place_rows(h, X, ldx, n, d_assign, k, sorted, st)) return rc;
  return finish_index(h, k, n, st);
}

// One destination segment of the row exchange: `count` consecutive rows of the receive buffer (one source rank's
// members of one owned list, ascending vec_id) go to storage rows dest, dest + 1, ...
struct RecvSeg {
  uint32_t src_row, count, dest, pad;
};

// send side: local rows in (destination rank, cluster, ascending index) order, row-major pitch ldp, + their vec ids
__global__ void pack_rows_kernel(const float* X, uint32_t ldx, uint32_t d, uint32_t ldp, const uint32_t* sorted_ids, const uint32_t* assign,
                                 const uint32_t* starts, const uint32_t* send_base, uint32_t row_begin, uint64_t n, float* out, uint32_t* out_ids) {
  const uint32_t ldp4 = ldp / 4, ldx4 = ldx / 4;
  const uint64_t total = n * ldp4;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p = i / ldp4;
    const uint32_t c4 = (uint32_t)(i % ldp4);
    const uint32_t id = sorted_ids[p];
    const uint32_t c = assign[id];
    const uint64_t dst = (uint64_t)send_base[c] + (p - starts[c]);
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (c4 < ldx4 && c4 * 4 < d) {
      v = reinterpret_cast<const f32x4*>(X + (uint64_t)id * ldx)[c4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (c4 * 4 + u >= d) v[u] = 0.0f;
    }
    reinterpret_cast<f32x4*>(out + dst * ldp)[c4] = v;
    if (c4 == 0) out_ids[dst] = row_begin + id;
  }
}

// receive side: block per segment, rows into the lane-transposed tiles of their list
__global__ __launch_bounds__(256) void unpack_rows_kernel(const float* in, uint32_t ldp, const uint32_t* in_ids, const RecvSeg* segs, uint32_t ld,
                                                          float* rows, uint32_t* row_ids) {
  const RecvSeg sg = segs[blockIdx.x];
  const uint32_t ld4 = ld / 4, ldp4 = ldp / 4;
  const uint64_t total = (uint64_t)sg.count * ld4;
  for (uint64_t i = threadIdx.x; i < total; i += blockDim.x) {
    const uint32_t r = (uint32_t)(i / ld4), c4 = (uint32_t)(i % ld4);
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (c4 < ldp4) v = reinterpret_cast<const f32x4*>(in + (uint64_t)(sg.src_row + r) * ldp)[c4];
    *reinterpret_cast<f32x4*>(rows + blocked_index((uint64_t)sg.dest + r, c4 * 4, ld)) = v;
    if (c4 == 0) row_ids[sg.dest + r] = in_ids[sg.src_row + r];
  }
}

// storage row -> row of the receive buffer, from the segments (a block per segment)
__global__ void fill_row_src_kernel(const RecvSeg* segs, uint32_t* row_src) {
  const RecvSeg sg = segs[blockIdx.x];
  for (uint32_t r = threadIdx.x; r < sg.count; r += blockDim.x) row_src[sg.dest + r] = sg.src_row + r;
}

__global__ void sum_counts_kernel(const uint32_t* counts_all, uint32_t world, uint32_t k, uint32_t* out) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= k) return;
  uint32_t s = 0;
  for (uint32_t r = 0; r < world; ++r) s += counts_all[(uint64_t)r * k + c];
  out[c] = s;
}

__global__ void scatter_centroid_rows_kernel(const float* tmp, uint32_t ld, const uint32_t* dst_c, uint32_t cnt, float* C) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)cnt * ld) return;
  C[(uint64_t)dst_c[i / ld] * ld + i % ld] = tmp[i];
}

// Row-sharded install (ivfflat.rs:123-127 across processes): the lists are dealt to the ranks by LPT over the GLOBAL
// lengths and every rank ships each of its rows to the owner of the row's list with ONE all_to_all_v (rows) + one for
// the vec ids.  A rank sends its rows ordered by (destination, cluster, ascending local index); ranks hold ascending
// ranges, so concatenating the sources in rank order inside a list IS the reference's ascending vec_id order.
int32_t install_index_sharded(vers_ivf* h, const float* X, uint32_t ldx, uint64_t n_loc, const BuildShard& sh, const uint32_t* d_assign,
                              uint32_t k, hipStream_t st) {
  const vers_comm_t* cm = sh.comm;
  const uint32_t W = sh.world, me = sh.rank;
  DevBuf sorted, counts_all_d;
  uint32_t* counts = nullptr;
  uint32_t* starts = nullptr;
  const int32_t rc_group = [&]() -> int32_t {  // (local work ahead of the first rendezvous of the install: agreed on before anyone enters it)
    if (int32_t rc = sorted.reserve((n_loc ? n_loc : 1) * sizeof(uint32_t))) return rc;
    if (int32_t rc = h->km.counts.reserve((2 * (size_t)k + 2) * sizeof(uint32_t))) return rc;
    counts = h->km.counts.as<uint32_t>();
    starts = counts + k;
    if (int32_t rc = km_group(d_assign, (uint32_t)n_loc, k, sorted.as<uint32_t>(), counts, starts, h->km, st)) return rc;
    if (int32_t rc = counts_all_d.reserve((size_t)W * (k ? k : 1) * 4)) return rc;
    VERS_HIP_TRY(hipStreamSynchronize(st));
    return VERS_OK;
  }();
  if (int32_t rc = sh.agree ? (*sh.agree)(rc_group, "grouping the local rows by list") : rc_group) return rc;
  if (k)
    if (int32_t rc = comm_rc(cm->all_gather(cm->ctx, counts, counts_all_d.p, (uint64_t)k * 4), "all_gather")) return rc;
  std::vector<uint32_t> ca((size_t)W * (k ? k : 1), 0), starts_h((size_t)k + 1, 0);
  if (k) {
    VERS_HIP_TRY(hipMemcpy(ca.data(), counts_all_d.p, (size_t)W * k * 4, hipMemcpyDeviceToHost));
    VERS_HIP_TRY(hipMemcpy(starts_h.data(), starts, ((size_t)k + 1) * 4, hipMemcpyDeviceToHost));
  }
  std::vector<uint32_t> lens(k ? k : 1, 0);
  for (uint32_t c = 0; c < k; ++c) {
    uint64_t s = 0;
    for (uint32_t r = 0; r < W; ++r) s += ca[(size_t)r * k + c];
    if (s > 0xFFFFFFFFull) return fail(VERS_ERR_INVALID, "a list longer than 2^32-1 rows");
    lens[c] = (uint32_t)s;
  }
  h->rank = me;
  h->world = W;
  const int32_t rc_plan = plan_storage(h, lens.data(), k, st);  // (a failure here -- the rows of the owned lists do not fit -- is agreed on below, with the exchange buffers)
  // send plan: rows for destination t = my members of the lists t owns, clusters ascending
  const uint32_t ldp = h->ldx;  // packed rows travel with the k-means pitch (d rounded up to 4 floats)
  std::vector<uint64_t> send_rows(W, 0), send_off_rows(W, 0), recv_rows(W, 0), recv_off_rows(W, 0);
  for (uint32_t c = 0; c < k; ++c) send_rows[h->h_owner[c]] += ca[(size_t)me * k + c];
  for (uint32_t t = 1; t < W; ++t) send_off_rows[t] = send_off_rows[t - 1] + send_rows[t - 1];
  std::vector<uint32_t> send_base(k ? k : 1, 0);
  {
    std::vector<uint64_t> cur(send_off_rows);
    for (uint32_t c = 0; c < k; ++c) {
      send_base[c] = (uint32_t)cur[h->h_owner[c]];
      cur[h->h_owner[c]] += ca[(size_t)me * k + c];
    }
  }
  // receive plan: from source s my owned lists' members, clusters ascending
  std::vector<RecvSeg> segs;
  for (uint32_t s = 0; s < W; ++s) {
    for (uint32_t c = 0; c < k; ++c)
      if (h->h_owner[c] == me) recv_rows[s] += ca[(size_t)s * k + c];
    if (s) recv_off_rows[s] = recv_off_rows[s - 1] + recv_rows[s - 1];
  }
  {
    std::vector<uint32_t> before(k ? k : 1, 0);  // members of list c that came from ranks before s
    for (uint32_t s = 0; s < W; ++s) {
      uint64_t r0 = recv_off_rows[s];
      for (uint32_t c = 0; c < k; ++c) {
        if (h->h_owner[c] != me) continue;
        const uint32_t cnt = ca[(size_t)s * k + c];
        if (cnt) segs.push_back(RecvSeg{(uint32_t)r0, cnt, h->h_off[c] + before[c], 0u});
        r0 += cnt;
        before[c] += cnt;
      }
    }
  }
  const uint64_t n_recv = recv_off_rows[W - 1] + recv_rows[W - 1];
  DevBuf sbuf, sids, rbuf, rids, dbase, dsegs;
  const int32_t rc_alloc = [&]() -> int32_t {
    if (rc_plan) return rc_plan;
    if (n_recv > 0xFFFFFFFFull) return fail(VERS_ERR_INVALID, "more than 2^32-1 rows received by one rank");
    if (int32_t rc = sbuf.reserve((n_loc ? n_loc : 1) * (size_t)ldp * 4)) return rc;
    if (int32_t rc = sids.reserve((n_loc ? n_loc : 1) * 4)) return rc;
    if (int32_t rc = rbuf.reserve((n_recv ? n_recv : 1) * (size_t)ldp * 4)) return rc;
    if (int32_t rc = rids.reserve((n_recv ? n_recv : 1) * 4)) return rc;
    if (int32_t rc = dbase.reserve((k ? k : 1) * 4)) return rc;
    if (int32_t rc = dsegs.reserve((segs.size() ? segs.size() : 1) * sizeof(RecvSeg))) return rc;
    return VERS_OK;
  }();
  if (int32_t rc = sh.agree ? (*sh.agree)(rc_alloc, "the exchange buffers of the rows-to-owners all_to_all_v") : rc_alloc) return rc;  // (storage + send + receive: the build's peak)
  if (k) VERS_HIP_TRY(hipMemcpyAsync(dbase.p, send_base.data(), (size_t)k * 4, hipMemcpyHostToDevice, st));
  if (!segs.empty()) VERS_HIP_TRY(hipMemcpyAsync(dsegs.p, segs.data(), segs.size() * sizeof(RecvSeg), hipMemcpyHostToDevice, st));
  if (n_loc) {
    hipLaunchKernelGGL(pack_rows_kernel, dim3(h->n_cu * 8), dim3(256), 0, st, X, ldx, h->d, ldp, sorted.as<uint32_t>(), d_assign, starts,
                       dbase.as<uint32_t>(), (uint32_t)sh.row_begin, n_loc, sbuf.as<float>(), sids.as<uint32_t>());
    VERS_HIP_TRY(hipGetLastError());
  }
  VERS_HIP_TRY(hipStreamSynchronize(st));
  std::vector<uint64_t> sb(W), so(W), rb(W), ro(W);
  for (uint32_t t = 0; t < W; ++t) {
    sb[t] = send_rows[t] * ldp * 4; so[t] = send_off_rows[t] * ldp * 4;
    rb[t] = recv_rows[t] * ldp * 4; ro[t] = recv_off_rows[t] * ldp * 4;
  }
  if (int32_t rc = comm_rc(cm->all_to_all_v(cm->ctx, sbuf.p, sb.data(), so.data(), rbuf.p, rb.data(), ro.data()), "all_to_all_v")) return rc;
  for (uint32_t t = 0; t < W; ++t) {
    sb[t] = send_rows[t] * 4; so[t] = send_off_rows[t] * 4;
    rb[t] = recv_rows[t] * 4; ro[t] = recv_off_rows[t] * 4;
  }
  if (int32_t rc = comm_rc(cm->all_to_all_v(cm->ctx, sids.p, sb.data(), so.data(), rids.p, rb.data(), ro.data()), "all_to_all_v")) return rc;
  sbuf.release();
  sids.release();
  // (capacity slack and tile padding of the storage are zero rows: (0 - q)^2 terms never enter a result, ids stay 0xFFFFFFFF)
  if (h->cap_rows >= 64 && !segs.empty()) {
    // whole destination tiles through LDS (gather_tiles_kernel), every tile written completely: no memset of the storage
    DevBuf row_src;
    if (int32_t rc = row_src.reserve(h->cap_rows * sizeof(uint32_t))) return rc;
    VERS_HIP_TRY(hipMemsetAsync(row_src.p, 0xFF, h->cap_rows * sizeof(uint32_t), st));
    hipLaunchKernelGGL(fill_row_src_kernel, dim3((unsigned)segs.size()), dim3(256), 0, st, dsegs.as<RecvSeg>(), row_src.as<uint32_t>());
    const size_t lds = 64 * (size_t)(kGatherCols4 + 1) * sizeof(f32x4);
    if (int32_t rc = scan_prepare_launch(gather_tiles_kernel, lds)) return rc;
    hipLaunchKernelGGL(gather_tiles_kernel, dim3((unsigned)(h->cap_rows / 64)), dim3(256), lds, st, rbuf.as<float>(), ldp, h->d, h->ld,
                       (const uint32_t*)nullptr, (const uint32_t*)nullptr, h->list_off.as<uint32_t>(), h->list_len.as<uint32_t>(),
                       h->tile_list.as<uint32_t>(), h->rows.as<float>(), h->row_ids.as<uint32_t>(), (const uint32_t*)row_src.as<uint32_t>(),
                       (const uint32_t*)rids.as<uint32_t>());
    VERS_HIP_TRY(hipGetLastError());
    VERS_HIP_TRY(hipStreamSynchronize(st));  // (row_src goes out of scope)
  } else {
    VERS_HIP_TRY(hipMemsetAsync(h->rows.p, 0, (h->cap_rows ? h->cap_rows : 1) * (size_t)h->ld * sizeof(float), st));
    if (!segs.empty()) {
      hipLaunchKernelGGL(unpack_rows_kernel, dim3((unsigned)segs.size()), dim3(256), 0, st, rbuf.as<float>(), ldp, rids.as<uint32_t>(),
                         dsegs.as<RecvSeg>(), h->ld, h->rows.as<float>(), h->row_ids.as<uint32_t>());
      VERS_HIP_TRY(hipGetLastError());
    }
  }
  VERS_HIP_TRY(hipStreamSynchronize(st));
  rbuf.release();
  rids.release();
  return finish_index(h, k, sh.n_total, st);
}

// build_kmeans + best-of-attempts (ivfflat.rs:73-121) on device-resident rows -- ALL of them (sh.comm == nullptr) or
// this process's contiguous range of a row-sharded corpus; leaves the winning centroids in h->centroids (or in
// *dst_centroids when one is given) and the assignments of the LOCAL rows in best_assign.  Same arithmetic order either way (see vers_hip.h).
int32_t run_build(vers_ivf* h, const float* X, uint32_t ldx, uint64_t n, const BuildShard& sh, uint32_t k, uint64_t num_attempts,
                  uint64_t max_iterations, const uint64_t* init_indices, DevBuf& best_assign, float* out_cost, int32_t* out_kept,
                  uint64_t* out_iterations, hipStream_t st, DevBuf* dst_centroids = nullptr) {
  const uint32_t ld = h->ldx;  // centroids live row-major with pitch ldx during k-means
  const vers_comm_t* cm = sh.comm;
  const uint32_t W = sh.world, me = sh.rank;
  const bool multi = cm != nullptr && W > 1;
  // the ranges of all ranks (contiguous, ascending, covering 0 .. n_total)
  std::vector<uint64_t> begins(W + 1, 0);
  begins[W] = sh.n_total;
  if (multi) {
    DevBuf mine, all;
    if (int32_t rc = mine.reserve(16)) return rc;
    if (int32_t rc = all.reserve(16 * (size_t)W)) return rc;
    const uint64_t my[2] = {sh.row_begin, n};
    VERS_HIP_TRY(hipMemcpy(mine.p, my, 16, hipMemcpyHostToDevice));
    if (int32_t rc = comm_rc(cm->all_gather(cm->ctx, mine.p, all.p, 16), "all_gather")) return rc;
    std::vector<uint64_t> rg(2 * (size_t)W);
    VERS_HIP_TRY(hipMemcpy(rg.data(), all.p, 16 * (size_t)W, hipMemcpyDeviceToHost));
    uint64_t expect = 0;
    for (uint32_t r = 0; r < W; ++r) {
      if (rg[2 * r] != expect) return fail(VERS_ERR_INVALID, "vers_ivf_build_sharded_dev: the ranks' row ranges are not contiguous and ascending in rank order");
      begins[r] = rg[2 * r];
      expect += rg[2 * r + 1];
    }
    if (expect != sh.n_total) return fail(VERS_ERR_INVALID, "vers_ivf_build_sharded_dev: the ranks' row counts do not add up to n_total");
  }
  DevBuf C, Cn, S, assign, mind, sorted, idx, idx2, bestC, counts_all, counts_g, tmp_rows, ctl, ctl_all;
  const size_t cbytes = ((size_t)k * ld ? (size_t)k * ld : 1) * sizeof(float);
  const int32_t rc_alloc = [&]() -> int32_t {
    PhaseClock alloc_clock(&BuildStats::alloc_ms);
    if (int32_t rc = C.reserve(cbytes)) return rc;
    if (int32_t rc = Cn.reserve(cbytes)) return rc;
    if (int32_t rc = bestC.reserve(cbytes)) return rc;
    if (int32_t rc = assign.reserve((n ? n : 1) * 4)) return rc;
    if (int32_t rc = best_assign.reserve((n ? n : 1) * 4)) return rc;
    if (int32_t rc = mind.reserve((n ? n : 1) * 4)) return rc;
    if (int32_t rc = sorted.reserve((n ? n : 1) * 4)) return rc;
    if (int32_t rc = idx.reserve((k ? k : 1) * 4)) return rc;
    if (int32_t rc = h->km.counts.reserve((2 * (size_t)k + 2) * 4)) return rc;
    if (int32_t rc = h->km.misc.reserve(64)) return rc;
    if (int32_t rc = h->km.status.reserve(16)) return rc;
    if (multi) {
      if (int32_t rc = S.reserve(cbytes)) return rc;
      if (int32_t rc = idx2.reserve((k ? k : 1) * 4)) return rc;
      if (int32_t rc = tmp_rows.reserve(cbytes)) return rc;
      if (int32_t rc = counts_all.reserve((size_t)W * (k ? k : 1) * 4)) return rc;
      if (int32_t rc = counts_g.reserve((k ? k : 1) * 4)) return rc;
      if (int32_t rc = ctl.reserve(16)) return rc;
      if (int32_t rc = ctl_all.reserve(16 * (size_t)W)) return rc;
    }
    return VERS_OK;
  }();
  auto agree = [&](int32_t rc, const char* where) -> int32_t { return multi && sh.agree ? (*sh.agree)(rc, where) : rc; };
  if (int32_t rc = agree(rc_alloc, "the build's allocations")) return rc;
  VERS_HIP_TRY(hipMemsetAsync(h->km.status.p, 0, 16, st));
  uint32_t* counts = h->km.counts.as<uint32_t>();
  uint32_t* starts = counts + k;
  float* cost_dev = h->km.misc.as<float>();
  float* cost_in = cost_dev + 1;
  uint32_t* flag_dev = h->km.misc.as<uint32_t>() + 4;
  float best = INFINITY;
  *out_kept = 0;
  const bool mfma = km_use_mfma(n, k, h->d);
  auto assign_pass = [&](const float* Cc, uint32_t* a_out, float* m_out) -> int32_t {
    if (n == 0) return VERS_OK;
    return (mfma ? km_assign_mfma : km_assign)(X, ldx, n, Cc, ld, k, h->d, a_out, m_out, h->km, h->n_cu, st, h->metric);
  };
  std::vector<uint32_t> src32(k ? k : 1), dst32(k ? k : 1);
  for (uint64_t a = 0; a < num_attempts; ++a) {
    if (sh.n_total > 0 && k == 0) return fail(VERS_ERR_EMPTY, "build_index with zero clusters: min_by over no centroids (reference panics)");
    for (uint32_t c = 0; c < k; ++c)
      if (init_indices[a * k + c] >= sh.n_total) return fail(VERS_ERR_INVALID, "vers_ivf_build: init index out of range");
    // initialize_centroids (ivfflat.rs:18-27, draws injected): C[c] = row init[c].  Sharded: the rows drawn from rank
    // r's range are gathered there and broadcast (bit copies), everyone scatters them to their centroid slots.
    for (uint32_t r = 0; r < W && k; ++r) {
      uint32_t cnt = 0;
      for (uint32_t c = 0; c < k; ++c) {
        const uint64_t ix = init_indices[a * k + c];
        if (ix >= begins[r] && ix < begins[r + 1]) { src32[cnt] = (uint32_t)(ix - begins[r]); dst32[cnt] = c; ++cnt; }
      }
      if (!multi) {  // one process: straight into C
        VERS_HIP_TRY(hipMemcpyAsync(idx.p, src32.data(), (size_t)k * 4, hipMemcpyHostToDevice, st));
        VERS_HIP_TRY(hipStreamSynchronize(st));  // src32 is reused by the next attempt
        hipLaunchKernelGGL(gather_init_kernel, dim3((unsigned)(((uint64_t)k * ld + 255) / 256)), dim3(256), 0, st, X, ldx, h->d, ld,
                           idx.as<uint32_t>(), k, C.as<float>());
        VERS_HIP_TRY(hipGetLastError());
        break;
      }
      if (cnt == 0) continue;
      if (r == me) {
        VERS_HIP_TRY(hipMemcpyAsync(idx.p, src32.data(), (size_t)cnt * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(gather_init_kernel, dim3((unsigned)(((uint64_t)cnt * ld + 255) / 256)), dim3(256), 0, st, X, ldx, h->d, ld,
                           idx.as<uint32_t>(), cnt, tmp_rows.as<float>());
        VERS_HIP_TRY(hipGetLastError());
      }
      VERS_HIP_TRY(hipMemcpyAsync(idx2.p, dst32.data(), (size_t)cnt * 4, hipMemcpyHostToDevice, st));
      VERS_HIP_TRY(hipStreamSynchronize(st));
      if (int32_t rc = comm_rc(cm->broadcast(cm->ctx, tmp_rows.p, (uint64_t)cnt * ld * 4, r), "broadcast")) return rc;
      hipLaunchKernelGGL(scatter_centroid_rows_kernel, dim3((unsigned)(((uint64_t)cnt * ld + 255) / 256)), dim3(256), 0, st,
                         tmp_rows.as<float>(), ld, idx2.as<uint32_t>(), cnt, C.as<float>());
      VERS_HIP_TRY(hipGetLastError());
      VERS_HIP_TRY(hipStreamSynchronize(st));  // dst32 / tmp_rows are reused by the next source rank
    }
    uint64_t iters = 0;
    for (uint64_t it = 0; it < max_iterations; ++it) {
      {  // assign + grouping are local: what a rank's own failure there was is agreed on before the ranks next meet
        int32_t rc_a = assign_pass(C.as<float>(), assign.as<uint32_t>(), nullptr);
        if (!rc_a) rc_a = km_group(assign.as<uint32_t>(), (uint32_t)n, k, sorted.as<uint32_t>(), counts, starts, h->km, st);
        if (int32_t rc = agree(rc_a, "assign_to_clusters")) return rc;
      }
      if (!multi) {
        KmTimer t(st, &BuildStats::update_ms);
        if (int32_t rc = km_update(X, ldx, h->d, sorted.as<uint32_t>(), starts, counts, k, Cn.as<float>(), ld, st)) return rc;
      } else if (k) {
        // update_centroids over the sharded rows (ivfflat.rs:47-71): global member counts by all-gather (integers),
        // running sums CHAINED through the ranks in ascending-range order, division on the last rank, broadcast.
        // A LOCAL failure (a HIP error, a failed launch) is remembered and the rank still walks through every rendezvous
        // of the pass -- its peers are waiting in them -- and all ranks leave together at the agreement behind the broadcast.
        int32_t rc_u = VERS_OK;
        auto local = [&](int32_t rc) { if (rc && !rc_u) rc_u = rc; };
        auto hip_local = [&](hipError_t e, const char* what) { if (e != hipSuccess) { (void)hipGetLastError(); local(fail(VERS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e))); } };
        hip_local(hipStreamSynchronize(st), "hipStreamSynchronize");
        if (int32_t rc = comm_rc(cm->all_gather(cm->ctx, counts, counts_all.p, (uint64_t)k * 4), "all_gather")) return rc;
        hipLaunchKernelGGL(sum_counts_kernel, dim3((k + 255) / 256), dim3(256), 0, st, counts_all.as<uint32_t>(), W, k, counts_g.as<uint32_t>());
        hip_local(hipGetLastError(), "sum_counts_kernel");
        if (me == 0) hip_local(hipMemsetAsync(S.p, 0, cbytes, st), "hipMemsetAsync");
        else {
          hip_local(hipStreamSynchronize(st), "hipStreamSynchronize");
          if (int32_t rc = comm_rc(cm->recv(cm->ctx, S.p, (uint64_t)k * ld * 4, me - 1), "recv")) return rc;
        }
        {
          KmTimer t(st, &BuildStats::update_ms);  // (this rank's share of the chained sums; the hops are the host's collectives)
          local(km_update_sums(X, ldx, h->d, sorted.as<uint32_t>(), starts, k, S.as<float>(), ld, st));
          if (me + 1 == W) local(km_finish_centroids(S.as<float>(), counts_g.as<uint32_t>(), k, ld, Cn.as<float>(), st));
        }
        hip_local(hipStreamSynchronize(st), "hipStreamSynchronize");
        if (me + 1 < W)
          if (int32_t rc = comm_rc(cm->send(cm->ctx, S.p, (uint64_t)k * ld * 4, me + 1), "send")) return rc;
        if (int32_t rc = comm_rc(cm->broadcast(cm->ctx, Cn.p, (uint64_t)k * ld * 4, W - 1), "broadcast")) return rc;
        if (int32_t rc = agree(rc_u, "update_centroids")) return rc;
      }
      if (int32_t rc = km_differs(C.as<float>(), Cn.as<float>(), (uint64_t)k * ld, flag_dev, st)) return rc;
      uint32_t differs = 0;
      VERS_HIP_TRY(hipMemcpyAsync(&differs, flag_dev, 4, hipMemcpyDeviceToHost, st));
      VERS_HIP_TRY(hipStreamSynchronize(st));
      ++iters;
      if (!differs) break;  // ivfflat.rs:91-93: bitwise equal -> keep the OLD centroids and stop
      std::swap(C.p, Cn.p);
      std::swap(C.cap, Cn.cap);
    }
    if (out_iterations) out_iterations[a] = iters;
    if (int32_t rc = agree(assign_pass(C.as<float>(), assign.as<uint32_t>(), mind.as<float>()), "the final assign_to_clusters")) return rc;
    // calculate_kmeans_cost (ivfflat.rs:138-149): one left-to-right f32 fold over ALL points -- chained like the sums
    const float* fold_init = nullptr;
    if (multi && me > 0) {
      VERS_HIP_TRY(hipStreamSynchronize(st));
      if (int32_t rc = comm_rc(cm->recv(cm->ctx, cost_in, 4, me - 1), "recv")) return rc;
      fold_init = cost_in;
    }
    int32_t rc_fold;
    {
      KmTimer t(st, &BuildStats::cost_ms);
      rc_fold = km_cost_fold(mind.as<float>(), n, fold_init, cost_dev, st);
    }
    if (!multi && rc_fold) return rc_fold;  // (sharded: the rank still hands a word on and is heard at the agreement below)
    uint32_t stw = 0;
    if (multi) {
      VERS_HIP_TRY(hipStreamSynchronize(st));
      if (me + 1 < W)
        if (int32_t rc = comm_rc(cm->send(cm->ctx, cost_dev, 4, me + 1), "send")) return rc;
      if (int32_t rc = comm_rc(cm->broadcast(cm->ctx, cost_dev, 4, W - 1), "broadcast")) return rc;
      // a NaN distance anywhere fails the build everywhere (the reference panics)
      VERS_HIP_TRY(hipMemcpyAsync(ctl.p, h->km.status.p, 16, hipMemcpyDeviceToDevice, st));
      VERS_HIP_TRY(hipStreamSynchronize(st));
      if (int32_t rc = comm_rc(cm->all_gather(cm->ctx, ctl.p, ctl_all.p, 16), "all_gather")) return rc;
      std::vector<uint32_t> sw(4 * (size_t)W);
      VERS_HIP_TRY(hipMemcpy(sw.data(), ctl_all.p, 16 * (size_t)W, hipMemcpyDeviceToHost));
      for (uint32_t r = 0; r < W; ++r) stw |= sw[4 * r];
      if (int32_t rc = agree(rc_fold, "calculate_kmeans_cost")) return rc;
    }
    float cost = 0.0f;
    VERS_HIP_TRY(hipMemcpyAsync(&cost, cost_dev, 4, hipMemcpyDeviceToHost, st));
    if (!multi) VERS_HIP_TRY(hipMemcpyAsync(&stw, h->km.status.p, 4, hipMemcpyDeviceToHost, st));
    VERS_HIP_TRY(hipStreamSynchronize(st));
    if ((stw & 1u) && k >= 2) {
      VERS_HIP_TRY(hipMemset(h->km.status.p, 0, 16));
      return fail(VERS_ERR_NAN, "NaN distance in assign_to_clusters (reference panics)");
    }
    if (cost < best) {  // strict: the first best attempt wins (ivfflat.rs:116)
      best = cost;
      *out_kept = 1;
      VERS_HIP_TRY(hipMemcpyAsync(bestC.p, C.p, cbytes, hipMemcpyDeviceToDevice, st));
      VERS_HIP_TRY(hipMemcpyAsync(best_assign.p, assign.p, (n ? n : 1) * 4, hipMemcpyDeviceToDevice, st));
    }
  }
  km_timers_collect();
  *out_cost = best;
  if (*out_kept) {
    DevBuf& dst = dst_centroids ? *dst_centroids : h->centroids;  // (vers_ivf_recluster: the handle's centroids stay until its commit point)
    if (int32_t rc = dst.reserve(cbytes)) return rc;
    VERS_HIP_TRY(hipMemcpyAsync(dst.p, bestC.p, cbytes, hipMemcpyDeviceToDevice, st));
  }
  VERS_HIP_TRY(hipStreamSynchronize(st));
  return VERS_OK;
}

// any other way of (re)making the index abandons a streamed upload in progress (vers_ivf_upload_begin .. _end)
static void upload_abandon(vers_ivf* h) {
  if (h->up.open) h->up.close();
}

int32_t build_common(vers_ivf* h, const float* X, uint32_t ldx, uint64_t n, const BuildShard& sh_in, uint64_t num_clusters, uint64_t num_attempts,
                     uint64_t max_iterations, const uint64_t* init_indices, float* out_centroids, uint64_t c_stride_bytes,
                     uint64_t* out_assignments, float* out_cost, int32_t* out_kept, uint64_t* out_iterations) {
  const uint32_t k = (uint32_t)num_clusters;
  upload_abandon(h);
  PhaseClock total_clock(&BuildStats::total_ms);
  DevBuf best_assign;
  float cost = INFINITY;
  int32_t kept = 0;
  // the agreement's words exist before the first collective of the build (see Agreement)
  Agreement ag;
  if (int32_t rc = ag.init(sh_in.comm, sh_in.world)) return rc;
  BuildShard sh = sh_in;
  sh.agree = &ag;
  if (int32_t rc = run_build(h, X, ldx, n, sh, k, num_attempts, max_iterations, init_indices, best_assign, &cost, &kept,
                             out_iterations, nullptr))
    return rc;
  if (out_cost) *out_cost = cost;
  if (out_kept) *out_kept = kept;
  if (!kept) {
    // nothing kept: centroids and assignments stay EMPTY, ids = num_clusters empty lists (ivfflat.rs:109-110,123)
    h->k = 0;
    h->n_total = 0;
    h->cap_rows = 0;
    h->max_len = 0;
    h->h_len.clear(); h->h_off.clear(); h->h_cap.clear();
    return VERS_OK;
  }
  {
    const auto t_in = std::chrono::steady_clock::now();
    const double derive0 = build_stats().derive_ms;
    if (sh.comm != nullptr && sh.world > 1) {
      if (int32_t rc = install_index_sharded(h, X, ldx, n, sh, best_assign.as<uint32_t>(), k, nullptr)) return rc;
    } else {
      if (int32_t rc = install_index(h, X, ldx, n, best_assign.as<uint32_t>(), k, nullptr)) return rc;
    }
    // (install = everything of this step but what finish_index accounted as derive)
    build_stats_add(&BuildStats::install_ms, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_in).count() - (build_stats().derive_ms - derive0));
  }
  if (out_centroids && k)
    VERS_HIP_TRY(hipMemcpy2D(out_centroids, (size_t)c_stride_bytes, h->centroids.p, (size_t)h->ldx * 4, (size_t)h->d * 4, k,
                             hipMemcpyDeviceToHost));
  if (out_assignments && n) {
    DevBuf a64;
    if (int32_t rc = a64.reserve(n * 8)) return rc;
    hipLaunchKernelGGL(u32_to_u64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, best_assign.as<uint32_t>(), n,
                       a64.as<uint64_t>());
    VERS_HIP_TRY(hipGetLastError());
    VERS_HIP_TRY(hipMemcpy(out_assignments, a64.p, n * 8, hipMemcpyDeviceToHost));
  }
  return VERS_OK;
}

// Every owned list moves to a new storage plan with room for lens[c] rows plus head-room (the rows it holds now, h_len[c], are copied):
// relayout() plans for the current lengths, add_batch for the lengths after the chunk -- one re-layout per chunk however many lists overflow.
static int32_t relayout_for(vers_ivf* h, const uint32_t* lens) {
  h->flt_moved += 1;  // (prepared filters: every storage row moves)
  const uint32_t k = h->k;
  std::vector<uint32_t> noff(k), ncap(k);
  uint64_t off = 0;
  for (uint32_t c = 0; c < k; ++c) {
    const uint32_t len = lens[c];
    ncap[c] = h->h_owner[c] == h->rank ? round_up(len + std::max<uint32_t>(64u, len / 8u), 64u) : 0u;
    noff[c] = (uint32_t)off;
    off += ncap[c];
    if (off > 0xFFFFFFFFull) return fail(VERS_ERR_INVALID, "more than 2^32-1 storage rows on one GPU");
  }
  DevBuf nrows, nids;
  if (int32_t rc = nrows.reserve((off ? off : 1) * (size_t)h->ld * sizeof(float))) return rc;
  if (int32_t rc = nids.reserve((off ? off : 1) * sizeof(uint32_t))) return rc;
  VERS_HIP_TRY(hipMemset(nids.p, 0xFF, (off ? off : 1) * sizeof(uint32_t)));
  for (uint32_t c = 0; c < k; ++c) {
    if (!h->h_len[c] || h->h_owner[c] != h->rank) continue;
    // lists start on tile boundaries, so whole 64-row tiles move as they are
    VERS_HIP_TRY(hipMemcpyAsync(nrows.as<float>() + (size_t)noff[c] * h->ld, h->rows.as<float>() + (size_t)h->h_off[c] * h->ld,
                                (size_t)round_up(h->h_len[c], 64) * h->ld * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
    VERS_HIP_TRY(hipMemcpyAsync(nids.as<uint32_t>() + noff[c], h->row_ids.as<uint32_t>() + h->h_off[c],
                                (size_t)h->h_len[c] * sizeof(uint32_t), hipMemcpyDeviceToDevice, nullptr));
  }
  VERS_HIP_TRY(hipDeviceSynchronize());
  std::swap(h->rows.p, nrows.p); std::swap(h->rows.cap, nrows.cap);
  std::swap(h->row_ids.p, nids.p); std::swap(h->row_ids.cap, nids.cap);
  nrows.release(); nids.release();  // (the old storage goes before refresh_norms re-allocates the shadow and the row-major copy)
  h->h_off = noff; h->h_cap = ncap; h->cap_rows = off;
  VERS_HIP_TRY(hipMemcpy(h->list_off.p, h->h_off.data(), (size_t)k * 4, hipMemcpyHostToDevice));
  {
    std::vector<uint32_t> so(k ? k : 1);
    for (uint32_t c = 0; c < k; ++c) so[h->h_slot[c]] = h->h_off[c];
    if (k) VERS_HIP_TRY(hipMemcpy(h->slot_off.p, so.data(), (size_t)k * 4, hipMemcpyHostToDevice));
  }
  if (int32_t rc = refresh_norms(h, 0, h->cap_rows, nullptr)) return rc;
  VERS_HIP_TRY(hipDeviceSynchronize());
  return VERS_OK;
}

int32_t relayout(vers_ivf* h) { return relayout_for(h, h->h_len.data()); }


// ---- streamed upload: begin / chunk / end (see vers_hip.h) -----------------------------------------------------------------

static int32_t upload_begin_inner(vers_ivf* h, const float* centroids, uint64_t k64, uint64_t c_stride_bytes, const uint64_t* list_lengths, uint64_t n_total);
int32_t upload_begin_locked(vers_ivf* h, const float* centroids, uint64_t k64, uint64_t c_stride_bytes, const uint64_t* list_lengths,
                            uint64_t n_total) {
  const int32_t rc = upload_begin_inner(h, centroids, k64, c_stride_bytes, list_lengths, n_total);
  if (rc) {  // (a failed begin leaves an EMPTY handle: no index, no stored rows for the exhaustive scan, no upload in progress)
    h->k = 0; h->n_total = 0; h->cap_rows = 0;
    upload_abandon(h);
  }
  return rc;
}
static int32_t upload_begin_inner(vers_ivf* h, const float* centroids, uint64_t k64, uint64_t c_stride_bytes, const uint64_t* list_lengths,
                                  uint64_t n_total) {
  const uint32_t k = (uint32_t)k64;
  VERS_HIP_TRY(hipDeviceSynchronize());  // searches still in flight read the storage this call re-plans
  upload_abandon(h);
  h->k = 0;  // no index until _end
  h->n_total = 0;
  std::vector<uint32_t> lens(k ? k : 1, 0);
  uint64_t sum = 0;
  for (uint32_t c = 0; c < k; ++c) {
    if (list_lengths[c] > 0xFFFFFFFFull) return fail(VERS_ERR_INVALID, "vers_ivf_upload_begin: a list longer than 2^32-1 rows");
    lens[c] = (uint32_t)list_lengths[c];
    sum += list_lengths[c];
  }
  if (sum != n_total) return fail(VERS_ERR_INVALID, "vers_ivf_upload_begin: the list lengths do not add up to n_total");
  const size_t cbytes = ((size_t)k * h->ldx ? (size_t)k * h->ldx : 1) * sizeof(float);
  if (int32_t rc = h->centroids.reserve(cbytes)) return rc;
  if (k) {
    VERS_HIP_TRY(hipMemset(h->centroids.p, 0, cbytes));
    VERS_HIP_TRY(hipMemcpy2D(h->centroids.p, (size_t)h->ldx * 4, centroids, c_stride_bytes, (size_t)h->d * 4, k, hipMemcpyHostToDevice));
  }
  if (int32_t rc = plan_storage(h, lens.data(), k, nullptr)) return rc;
  // slack behind the lists and tile padding are zero rows, as after build_index (gather_tiles_kernel writes whole tiles)
  VERS_HIP_TRY(hipMemsetAsync(h->rows.p, 0, (h->cap_rows ? h->cap_rows : 1) * (size_t)h->ld * sizeof(float), nullptr));
  auto& up = h->up;
  if (int32_t rc = up.fill.reserve(2 * (size_t)(k ? k : 1) * sizeof(uint32_t))) return rc;
  VERS_HIP_TRY(hipMemsetAsync(up.fill.p, 0, 2 * (size_t)(k ? k : 1) * sizeof(uint32_t), nullptr));
  if (int32_t rc = up.bad.reserve(16)) return rc;
  VERS_HIP_TRY(hipMemsetAsync(up.bad.p, 0, 16, nullptr));
  if (int32_t rc = h->km.counts.reserve((2 * (size_t)k + 2) * sizeof(uint32_t))) return rc;
  VERS_HIP_TRY(hipStreamSynchronize(nullptr));
  up.h_seen.assign(k ? k : 1, 0u);
  up.cap_rows = h->cap_rows;  // (utils::search_exhaustive over the stored rows sees none until _end)
  h->cap_rows = 0;
  up.k = k;
  up.n_total = n_total;
  up.seen = 0;
  up.open = true;
  return VERS_OK;
}

// one chunk whose rows are device-resident: a32 = assignments as u32 (range-checked by the caller's kernel: up.bad bit 0),
// ids32 = the rows' vec ids (nullptr: first + row), count_seen = the chunk holds ALL rows of its vec id range
static int32_t upload_place(vers_ivf* h, const float* X, uint32_t ldx, const uint32_t* a32, const uint32_t* ids32, uint32_t first, uint32_t n,
                            bool count_seen, hipStream_t st) {
  auto& up = h->up;
  const uint32_t k = up.k;
  if (n == 0 || k == 0) return VERS_OK;
  if (int32_t rc = up.sorted.reserve((size_t)n * sizeof(uint32_t))) return rc;
  uint32_t* counts = h->km.counts.as<uint32_t>();
  uint32_t* starts = counts + k;
  if (int32_t rc = km_group(a32, n, k, up.sorted.as<uint32_t>(), counts, starts, h->km, st)) return rc;
  const uint8_t* owner = h->world > 1 ? h->owner.as<uint8_t>() : (const uint8_t*)nullptr;
  uint32_t* fill = up.fill.as<uint32_t>();
  const size_t lds = 64 * (size_t)(kGatherCols4 + 1) * sizeof(f32x4);
  if (int32_t rc = scan_prepare_launch(place_chunk_kernel, lds)) return rc;
  hipLaunchKernelGGL(place_chunk_kernel, dim3((n + 63u) / 64u), dim3(256), lds, st, X, ldx, h->d, h->ld, (const uint32_t*)up.sorted.as<uint32_t>(), a32,
                     (const uint32_t*)starts, (const uint32_t*)h->list_off.as<uint32_t>(), (const uint32_t*)h->list_len.as<uint32_t>(),
                     (const uint32_t*)fill, owner, h->rank, ids32, first, n, h->rows.as<float>(), h->row_ids.as<uint32_t>());
  hipLaunchKernelGGL(advance_fill_kernel, dim3((k + 255u) / 256u), dim3(256), 0, st, (const uint32_t*)counts, k, owner, h->rank,
                     (const uint32_t*)h->list_len.as<uint32_t>(), fill, count_seen ? fill + k : (uint32_t*)nullptr, up.bad.as<uint32_t>());
  VERS_HIP_TRY(hipGetLastError());
  return VERS_OK;
}

static int32_t upload_check_bad(vers_ivf* h, const char* who) {
  uint32_t bad = 0;
  VERS_HIP_TRY(hipMemcpy(&bad, h->up.bad.p, 4, hipMemcpyDeviceToHost));  // (synchronises the null stream: the chunk is placed)
  if (bad) {
    upload_abandon(h);
    return fail(VERS_ERR_INVALID, std::string(who) + (bad & 1u ? ": assignment out of range" : ": a list received more rows than vers_ivf_upload_begin announced") +
                                      " (the streamed upload is abandoned)");
  }
  return VERS_OK;
}

static int32_t upload_chunk_args(vers_ivf* h, const char* who, uint64_t first_vec_id, uint64_t n) {
  if (!h->up.open) return fail(VERS_ERR_INVALID, std::string(who) + ": no streamed upload in progress (vers_ivf_upload_begin first)");
  if (first_vec_id != h->up.seen) return fail(VERS_ERR_INVALID, std::string(who) + ": chunks must arrive in ascending contiguous order (first_vec_id != rows received so far)");
  if (n > h->up.n_total - h->up.seen) return fail(VERS_ERR_INVALID, std::string(who) + ": more rows than vers_ivf_upload_begin announced");
  return VERS_OK;
}

int32_t upload_chunk_dev_locked(vers_ivf* h, const float* rows_dev, uint64_t ld_floats, const uint64_t* assignments_dev, uint64_t first_vec_id,
                                uint64_t n) {
  if (int32_t rc = upload_chunk_args(h, "vers_ivf_upload_chunk_dev", first_vec_id, n)) return rc;
  auto& up = h->up;
  if (n) {
    if (int32_t rc = up.a32.reserve(n * sizeof(uint32_t))) return rc;
    hipLaunchKernelGGL(u64_to_u32_checked_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, assignments_dev, n, (uint64_t)up.k,
                       up.a32.as<uint32_t>(), up.bad.as<uint32_t>());
    VERS_HIP_TRY(hipGetLastError());
    if (int32_t rc = upload_place(h, rows_dev, (uint32_t)ld_floats, up.a32.as<uint32_t>(), nullptr, (uint32_t)first_vec_id, (uint32_t)n, true, nullptr)) return rc;
    if (int32_t rc = upload_check_bad(h, "vers_ivf_upload_chunk_dev")) return rc;
  }
  up.seen += n;
  return VERS_OK;
}

// Host rows: sub-chunks through a bounded pinned buffer of TWO halves.  Only the rows of the lists this rank owns are packed and cross
// PCIe (1/W of them on a rank of W), with their vec ids; every row is counted on the host for the final check.  While the copy engine
// and the placement kernel work on one half (an event per half says when they are done with it) the host packs the next sub-chunk
// into the other -- with several threads when it is large -- and the device-side `bad` word is read ONCE per chunk, at its end.
// (Round 5 packed row by row on one thread into ONE buffer and read `bad` back after every sub-chunk: pack, H2D and placement never
// overlapped.)
int32_t upload_chunk_host_locked(vers_ivf* h, const float* rows, uint64_t row_stride_bytes, const uint64_t* assignments, uint64_t first_vec_id,
                                 uint64_t n) {
  if (int32_t rc = upload_chunk_args(h, "vers_ivf_upload_chunk", first_vec_id, n)) return rc;
  auto& up = h->up;
  const uint32_t ldx = h->ldx, d = h->d;
  const size_t row_b = (size_t)ldx * 4;
  const size_t stage_bytes = (size_t)opt_get("upload_stage_mb", 256) << 20;
  const uint64_t sub = std::max<uint64_t>(64, std::min<uint64_t>(n ? n : 1, (stage_bytes / 2) / (row_b + 8)));
  const size_t half_b = (sub * (row_b + 8) + 255) & ~(size_t)255;
  if (up.pin_cap < 2 * half_b) {
    if (up.pin) { (void)hipHostFree(up.pin); up.pin = nullptr; up.pin_cap = 0; }
    VERS_HIP_TRY(hipHostMalloc(&up.pin, 2 * half_b, hipHostMallocDefault));
    up.pin_cap = 2 * half_b;
  }
  if (int32_t rc = up.stage.reserve(2 * sub * row_b)) return rc;
  if (int32_t rc = up.ids.reserve(2 * sub * 4)) return rc;
  if (int32_t rc = up.a32.reserve(2 * sub * 4)) return rc;
  for (auto& e : up.half_free)
    if (!e) VERS_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  const bool sharded = h->world > 1;
  std::vector<uint32_t> pos(sub);
  bool used[2] = {false, false};
  uint32_t turn = 0;
  for (uint64_t s0 = 0; s0 < n; s0 += sub) {
    const uint64_t m = std::min<uint64_t>(sub, n - s0);
    const uint32_t hf = turn & 1u;
    float* p_rows = (float*)((char*)up.pin + hf * half_b);
    uint32_t* p_ids = (uint32_t*)((char*)p_rows + sub * row_b);
    uint32_t* p_a = p_ids + sub;
    // (the half is free once the copies and the placement queued from it two sub-chunks ago are done)
    if (used[hf]) VERS_HIP_TRY(hipEventSynchronize(up.half_free[hf]));
    uint32_t packed = 0;
    for (uint64_t i = 0; i < m; ++i) {  // which rows go, where, with which id (serial: the owned rows keep their ascending order)
      const uint64_t a = assignments[s0 + i];
      if (a >= up.k) { (void)hipDeviceSynchronize(); upload_abandon(h); return fail(VERS_ERR_INVALID, "vers_ivf_upload_chunk: assignment out of range (the streamed upload is abandoned)"); }
      up.h_seen[a] += 1;
      if (sharded && h->h_owner[a] != h->rank) { pos[i] = 0xFFFFFFFFu; continue; }
      pos[i] = packed;
      p_ids[packed] = (uint32_t)(first_vec_id + s0 + i);
      p_a[packed] = (uint32_t)a;
      ++packed;
    }
    auto pack = [&](uint64_t i0, uint64_t i1) {
      for (uint64_t i = i0; i < i1; ++i) {
        if (pos[i] == 0xFFFFFFFFu) continue;
        float* dst = p_rows + (size_t)pos[i] * ldx;
        std::memcpy(dst, (const char*)rows + (s0 + i) * row_stride_bytes, (size_t)d * 4);
        for (uint32_t j = d; j < ldx; ++j) dst[j] = 0.0f;
      }
    };
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const unsigned nt = (size_t)packed * row_b >= (size_t(8) << 20) ? std::min(8u, hw) : 1u;
    if (nt > 1) {
      std::vector<std::thread> th;
      const uint64_t per = (m + nt - 1) / nt;
      for (unsigned t = 1; t < nt; ++t) th.emplace_back(pack, std::min<uint64_t>(m, t * per), std::min<uint64_t>(m, (t + 1) * per));
      pack(0, std::min<uint64_t>(m, per));
      for (auto& t : th) t.join();
    } else {
      pack(0, m);
    }
    if (packed) {
      float* d_rows = up.stage.as<float>() + (size_t)hf * sub * ldx;
      uint32_t* d_ids = up.ids.as<uint32_t>() + (size_t)hf * sub;
      uint32_t* d_a = up.a32.as<uint32_t>() + (size_t)hf * sub;
      VERS_HIP_TRY(hipMemcpyAsync(d_rows, p_rows, (size_t)packed * row_b, hipMemcpyHostToDevice, nullptr));
      VERS_HIP_TRY(hipMemcpyAsync(d_ids, p_ids, (size_t)packed * 4, hipMemcpyHostToDevice, nullptr));
      VERS_HIP_TRY(hipMemcpyAsync(d_a, p_a, (size_t)packed * 4, hipMemcpyHostToDevice, nullptr));
      if (int32_t rc = upload_place(h, d_rows, ldx, d_a, d_ids, 0u, packed, false, nullptr)) return rc;
      VERS_HIP_TRY(hipEventRecord(up.half_free[hf], nullptr));
      used[hf] = true;
    }
    ++turn;
  }
  // once per chunk (synchronises the null stream: everything is placed, both halves are free); a list that received too many rows
  // would also be caught by the per-list counts checked in _end
  if (n)
    if (int32_t rc = upload_check_bad(h, "vers_ivf_upload_chunk")) return rc;
  up.seen += n;
  return VERS_OK;
}

int32_t upload_end_locked(vers_ivf* h) {
  auto& up = h->up;
  if (!up.open) return fail(VERS_ERR_INVALID, "vers_ivf_upload_end: no streamed upload in progress");
  const uint32_t k = up.k;
  const uint64_t n_total = up.n_total;
  auto bail = [&](const std::string& m) { upload_abandon(h); return fail(VERS_ERR_INVALID, "vers_ivf_upload_end: " + m + " (the handle stays empty)"); };
  if (up.seen != n_total) return bail("fewer rows arrived than vers_ivf_upload_begin announced");
  std::vector<uint32_t> f(2 * (size_t)(k ? k : 1), 0u);
  VERS_HIP_TRY(hipMemcpy(f.data(), up.fill.p, f.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (uint32_t c = 0; c < k; ++c) {
    if ((uint64_t)f[k + c] + up.h_seen[c] != h->h_len[c]) return bail("list " + std::to_string(c) + " received a different number of rows than announced");
    if (h->h_owner[c] == h->rank && f[c] != h->h_len[c]) return bail("owned list " + std::to_string(c) + " is not complete");
  }
  h->cap_rows = up.cap_rows;
  up.close();
  return finish_index(h, k, n_total, nullptr);
}


// ---- add_batch: Index::add for many rows (see vers_hip.h) -----------------------------------------------------------------------
// Where the time of the add_batch calls of this process went (vers_add_batch_phases): host wall clock per phase, the stream
// synchronised at each phase's end.
constexpr int kAddBatchPhases = 9;
static std::mutex g_ab_mu;
static double g_ab[kAddBatchPhases] = {};  // calls, rows, re-layouts, stage, assign, group, relayout, place, derive (ms)
constexpr int kRemovePhases = 8;
static double g_rm[kRemovePhases] = {};  // vers_remove_phases: calls, ids, rows removed, stage, mark, compact, tables, derive (ms)
struct AbClock {
  int slot;
  double* acc;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit AbClock(int s, double* a = g_ab) : slot(s), acc(a) {}
  int32_t done() {  // the phase's work is finished when its clock stops
    VERS_HIP_TRY(hipStreamSynchronize(nullptr));
    std::lock_guard<std::mutex> lk(g_ab_mu);
    acc[slot] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return VERS_OK;
  }
};
static void ab_count(int slot, double v, double* acc = g_ab) {
  std::lock_guard<std::mutex> lk(g_ab_mu);
  acc[slot] += v;
}

// |x|^2 (+ maximum), fp16 shadow (+ residual maximum) and row-major copy of the listed tiles: refresh_norms for a tile list, one launch per array
static int32_t refresh_tiles(vers_ivf* h, const uint32_t* tiles, uint32_t nt, hipStream_t st) {
  if (nt == 0) return VERS_OK;
  h->head_valid = false;  // the int8 head does not follow tile lists: the list scan is one launch again until a compact or a full refresh
  h->balls_valid = false;
  const uint64_t n_rows = (uint64_t)nt * 64;
  if (shadow_mode() != 0) {
    if (h->shadow_valid) {
      const uint64_t work = n_rows * (h->ld / 8);
      hipLaunchKernelGGL(rows_to_f16_tiles_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, h->rows.as<float>(), h->ld, tiles, n_rows,
                         h->rows_bf.as<uint16_t>());
      hipLaunchKernelGGL(shadow_residual_tiles_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, h->rows.as<float>(), h->ld,
                         (const uint32_t*)h->row_ids.as<uint32_t>(), tiles, n_rows, h->pre_misc.as<uint32_t>() + 2);
      VERS_HIP_TRY(hipGetLastError());
    }
  } else {
    h->shadow_valid = false;  // rows changed without their shadow following (as refresh_norms)
  }
  if (h->rows_rm.p) {
    const size_t lds = 64 * (size_t)(kGatherCols4 + 1) * sizeof(f32x4);
    if (int32_t rc = scan_prepare_launch(tiles_to_rowmajor_kernel, lds)) return rc;
    hipLaunchKernelGGL(tiles_to_rowmajor_kernel, dim3(nt), dim3(256), lds, st, (const float*)h->rows.as<float>(), h->ld, tiles, h->rows_rm.as<float>());
    VERS_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(row_norms_tiles_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, h->rows.as<float>(), h->ld,
                     (const uint32_t*)h->row_ids.as<uint32_t>(), tiles, n_rows, h->xnorm.as<float>(), h->pre_misc.as<uint32_t>());
  VERS_HIP_TRY(hipGetLastError());
  return VERS_OK;
}

// One staged chunk X [m][ldx] (zero-padded) of rows with vec ids n_total, n_total + 1, ...: assignment, grouping, at most one re-layout,
// placement, tables, derived arrays.  A NaN distance at row i (k >= 2) keeps rows 0 .. i-1 only (*out_nan).  *out_m = rows added;
// out_a32_host (nullable) receives their clusters.
static int32_t add_batch_chunk(vers_ivf* h, const float* X, uint32_t m, uint32_t* out_m, bool* out_nan, uint32_t* out_a32_host) {
  const uint32_t k = h->k;
  const hipStream_t st = nullptr;
  auto& ab = h->ab;
  uint32_t* a32 = ab.a32.as<uint32_t>();
  *out_m = 0;
  *out_nan = false;
  // 1. first-minimum centroid of every row (ivfflat.rs:201-207) -- the build's assign pass on the handle's centroids
  {
    AbClock clk(4);
    if (k == 1) {  // one centroid: every row goes there, a NaN one included (nothing is compared)
      VERS_HIP_TRY(hipMemsetAsync(a32, 0, (size_t)m * sizeof(uint32_t), st));
    } else {
      if (int32_t rc = h->km.status.reserve(16)) return rc;
      VERS_HIP_TRY(hipMemsetAsync(h->km.status.p, 0, 16, st));
      if (int32_t rc = (km_use_mfma(m, k, h->d) ? km_assign_mfma : km_assign)(X, h->ldx, m, h->centroids.as<float>(), h->ldx, k, h->d, a32, nullptr,
                                                                              h->km, h->n_cu, st, h->metric))
        return rc;
      uint32_t stw = 0;
      VERS_HIP_TRY(hipMemcpy(&stw, h->km.status.p, 4, hipMemcpyDeviceToHost));
      if (stw & 1u) {
        // The pass reports a NaN distance by one status word, not per row: the first row that has one is found by bisection with the
        // exact scan over the rows not yet cleared ([0, lo) holds none, [lo, hi) holds one) -- about one more pass over the chunk, on the
        // error path only.  The rows before it keep the assignments of the pass above.
        DevBuf tmp;
        if (int32_t rc = tmp.reserve((size_t)m * sizeof(uint32_t))) return rc;
        uint32_t lo = 0, hi = m;
        while (hi - lo > 1) {
          const uint32_t mid = lo + (hi - lo) / 2;
          VERS_HIP_TRY(hipMemsetAsync(h->km.status.p, 0, 16, st));
          if (int32_t rc = km_assign(X + (uint64_t)lo * h->ldx, h->ldx, mid - lo, h->centroids.as<float>(), h->ldx, k, h->d, tmp.as<uint32_t>(), nullptr,
                                     h->km, h->n_cu, st, h->metric))
            return rc;
          VERS_HIP_TRY(hipMemcpy(&stw, h->km.status.p, 4, hipMemcpyDeviceToHost));
          if (stw & 1u) hi = mid;
          else lo = mid;
        }
        VERS_HIP_TRY(hipMemsetAsync(h->km.status.p, 0, 16, st));
        m = lo;
        *out_nan = true;
      }
    }
    if (int32_t rc = clk.done()) return rc;
  }
  if (m == 0) return VERS_OK;
  // 2. stable grouping by list, rows per list
  uint32_t* counts = h->km.counts.as<uint32_t>();
  uint32_t* starts = counts + k;
  std::vector<uint32_t> cnt(k);
  {
    AbClock clk(5);
    if (int32_t rc = ab.jobs.reserve(16)) return rc;  // (its first word: the range check's flag until the jobs are written)
    VERS_HIP_TRY(hipMemsetAsync(ab.jobs.p, 0, 4, st));
    hipLaunchKernelGGL(add_check_assign_kernel, dim3((m + 255) / 256), dim3(256), 0, st, a32, m, k, ab.jobs.as<uint32_t>());
    VERS_HIP_TRY(hipGetLastError());
    if (int32_t rc = km_group(a32, m, k, ab.sorted.as<uint32_t>(), counts, starts, h->km, st)) return rc;
    uint32_t bad = 0;
    VERS_HIP_TRY(hipMemcpy(cnt.data(), counts, (size_t)k * 4, hipMemcpyDeviceToHost));
    VERS_HIP_TRY(hipMemcpy(&bad, ab.jobs.p, 4, hipMemcpyDeviceToHost));
    if (bad) return fail(VERS_ERR_HIP, "vers_ivf_add_batch: the assign pass returned a cluster index out of range");
    if (int32_t rc = clk.done()) return rc;
  }
  // 3. new lengths; one re-layout for the whole chunk when an owned list outgrows its capacity
  std::vector<uint32_t> nl(k), first(k);
  bool grow = false;
  {
    uint32_t run = 0;
    for (uint32_t c = 0; c < k; ++c) {
      first[c] = run;
      run += cnt[c];
      nl[c] = h->h_len[c] + cnt[c];  // (no overflow: n_total + n <= 0xFFFFFFFE was checked)
      if (h->h_owner[c] == h->rank && nl[c] > h->h_cap[c]) grow = true;
    }
  }
  if (grow) {
    AbClock clk(6);
    if (int32_t rc = relayout_for(h, nl.data())) return rc;
    ab_count(2, 1.0);
    if (int32_t rc = clk.done()) return rc;
  }
  // 4. placement: one job per touched tile of an owned list; row p of list c's new rows -> storage row list_off[c] + old_len[c] + p
  std::vector<AddTileJob> jobs;
  for (uint32_t c = 0; c < k; ++c) {
    if (!cnt[c] || h->h_owner[c] != h->rank) continue;
    const uint64_t b = (uint64_t)h->h_off[c] + h->h_len[c], e = b + cnt[c];
    for (uint64_t t = b / 64; t * 64 < e; ++t) {
      const uint64_t r0 = std::max<uint64_t>(b, t * 64), r1 = std::min<uint64_t>(e, t * 64 + 64);
      jobs.push_back(AddTileJob{(uint32_t)t, (uint32_t)(r0 - t * 64), (uint32_t)(r1 - t * 64), first[c] + (uint32_t)(r0 - b)});
    }
  }
  const uint32_t nt = (uint32_t)jobs.size();
  const size_t jobs_b = (size_t)nt * sizeof(AddTileJob);
  {
    AbClock clk(7);
    if (nt) {
      std::vector<uint32_t> tiles(nt);
      for (uint32_t i = 0; i < nt; ++i) tiles[i] = jobs[i].tile;
      if (int32_t rc = ab.jobs.reserve(jobs_b + (size_t)nt * 4)) return rc;
      VERS_HIP_TRY(hipMemcpy(ab.jobs.p, jobs.data(), jobs_b, hipMemcpyHostToDevice));
      VERS_HIP_TRY(hipMemcpy(ab.jobs.as<char>() + jobs_b, tiles.data(), (size_t)nt * 4, hipMemcpyHostToDevice));
      const size_t lds = 64 * (size_t)(kGatherCols4 + 1) * sizeof(f32x4);
      if (int32_t rc = scan_prepare_launch(add_tiles_kernel, lds)) return rc;
      hipLaunchKernelGGL(add_tiles_kernel, dim3(nt), dim3(256), lds, st, X, h->ldx, h->d, h->ld, (const AddTileJob*)ab.jobs.p,
                         (const uint32_t*)ab.sorted.as<uint32_t>(), (uint32_t)h->n_total, h->rows.as<float>(), h->row_ids.as<uint32_t>());
      VERS_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(add_counts_kernel, dim3((k + 255) / 256), dim3(256), 0, st, (const uint32_t*)counts, k, (const uint32_t*)h->list_slot.as<uint32_t>(),
                       h->list_len.as<uint32_t>(), h->slot_len.as<uint32_t>());
    VERS_HIP_TRY(hipGetLastError());
    if (int32_t rc = clk.done()) return rc;
  }
  // 5. derived arrays of the touched tiles; the index is consistent once the stream is idle (the caller returns after that)
  {
    AbClock clk(8);
    if (int32_t rc = refresh_tiles(h, (const uint32_t*)(ab.jobs.as<char>() + jobs_b), nt, st)) return rc;
    if (int32_t rc = clk.done()) return rc;
  }
  if (out_a32_host) VERS_HIP_TRY(hipMemcpy(out_a32_host, a32, (size_t)m * 4, hipMemcpyDeviceToHost));
  for (uint32_t c = 0; c < k; ++c) h->max_len = std::max(h->max_len, nl[c]);
  h->h_len = nl;
  h->n_total += m;
  *out_m = m;
  return VERS_OK;
}

// The batch in chunks of option "add_batch_rows" rows (default: the matrix-core assign pass's batch), each staged zero-padded with pitch ldx:
// rows_host != nullptr copies through the pinned buffer (rows at row_stride_bytes), otherwise from rows_dev (pitch ld_floats) on the device.
// Clusters go to out_host (u64, host) or out_dev (u64, device), either may be null.
int32_t add_batch_locked(vers_ivf* h, const float* rows_host, uint64_t row_stride_bytes, const float* rows_dev, uint64_t ld_floats, uint64_t n,
                         uint64_t* out_host, uint64_t* out_dev, uint64_t* out_first_vec_id, uint64_t* out_added) {
  VERS_HIP_TRY(hipDeviceSynchronize());  // searches still in flight on any stream read the rows and tables this call changes
  if (out_first_vec_id) *out_first_vec_id = h->n_total;
  if (out_added) *out_added = 0;
  if (h->k == 0) return fail(VERS_ERR_EMPTY, "add_batch on an index without centroids (reference: unwrap on None, ivfflat.rs:207)");
  if (n == 0) return VERS_OK;
  if (h->n_total + n > 0xFFFFFFFEull) return fail(VERS_ERR_INVALID, "vers_ivf_add_batch: vec_id space exhausted");
  const uint32_t ldx = h->ldx, d = h->d;
  const uint64_t chunk = std::min<uint64_t>(n, (uint64_t)std::max<int64_t>(1, opt_get("add_batch_rows", 131072)));
  auto& ab = h->ab;
  if (int32_t rc = ab.stage.reserve(chunk * ldx * sizeof(float))) return rc;
  if (int32_t rc = ab.a32.reserve(chunk * sizeof(uint32_t))) return rc;
  if (int32_t rc = ab.sorted.reserve(chunk * sizeof(uint32_t))) return rc;
  if (int32_t rc = h->km.counts.reserve((2 * (size_t)h->k + 2) * sizeof(uint32_t))) return rc;
  if (int32_t rc = h->pre_misc.reserve(64)) return rc;
  if (rows_host && ab.pin_cap < chunk * ldx * sizeof(float)) {
    ab.free_pin();
    VERS_HIP_TRY(hipHostMalloc(&ab.pin, chunk * ldx * sizeof(float), hipHostMallocDefault));
    ab.pin_cap = chunk * ldx * sizeof(float);
  }
  std::vector<uint32_t> a_host(out_host ? chunk : 0);
  uint64_t added = 0;
  ab_count(0, 1.0);
  for (uint64_t s0 = 0; s0 < n; s0 += chunk) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - s0);
    {
      AbClock clk(3);
      if (rows_host) {
        float* pin = (float*)ab.pin;
        auto pack = [&](uint64_t i0, uint64_t i1) {
          for (uint64_t i = i0; i < i1; ++i) {
            float* dst = pin + i * ldx;
            std::memcpy(dst, (const char*)rows_host + (s0 + i) * row_stride_bytes, (size_t)d * 4);
            for (uint32_t j = d; j < ldx; ++j) dst[j] = 0.0f;
          }
        };
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        const unsigned nth = (size_t)m * ldx * 4 >= (size_t(8) << 20) ? std::min(8u, hw) : 1u;
        if (nth > 1) {
          std::vector<std::thread> th;
          const uint64_t per = (m + nth - 1) / nth;
          for (unsigned t = 1; t < nth; ++t) th.emplace_back(pack, std::min<uint64_t>(m, t * per), std::min<uint64_t>(m, (t + 1) * per));
          pack(0, std::min<uint64_t>(m, per));
          for (auto& t : th) t.join();
        } else {
          pack(0, m);
        }
        VERS_HIP_TRY(hipMemcpyAsync(ab.stage.p, pin, (size_t)m * ldx * 4, hipMemcpyHostToDevice, nullptr));
      } else {
        const uint64_t blocks = std::min<uint64_t>((uint64_t)h->n_cu * 8, ((uint64_t)m * (ldx / 4) + 255) / 256);
        hipLaunchKernelGGL(add_stage_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, nullptr, rows_dev + s0 * ld_floats, ld_floats, d, ldx, (uint64_t)m,
                           ab.stage.as<float>());
        VERS_HIP_TRY(hipGetLastError());
      }
      if (int32_t rc = clk.done()) return rc;
    }
    uint32_t got = 0;
    bool nan = false;
    const int32_t rc = add_batch_chunk(h, ab.stage.as<float>(), m, &got, &nan, out_host ? a_host.data() : nullptr);
    if (got) {
      if (out_host)
        for (uint32_t i = 0; i < got; ++i) out_host[s0 + i] = a_host[i];
      if (out_dev) {
        hipLaunchKernelGGL(u32_to_u64_kernel, dim3((got + 255) / 256), dim3(256), 0, nullptr, (const uint32_t*)ab.a32.as<uint32_t>(), (uint64_t)got,
                           out_dev + s0);
        VERS_HIP_TRY(hipGetLastError());
        VERS_HIP_TRY(hipStreamSynchronize(nullptr));
      }
      added += got;
      if (out_added) *out_added = added;
      ab_count(1, (double)got);
    }
    if (rc) return rc;
    if (nan) return fail(VERS_ERR_NAN, "NaN distance in add_batch at row " + std::to_string(s0 + got) + " (reference panics)");
  }
  return VERS_OK;
}

// ---- remove_batch: ids[assignments[v]].retain(|&x| x != v) for many v (see vers_hip.h) -----------------------------------------------
// ids_host != nullptr: the ids go through the pinned buffer in chunks of option "remove_batch_ids" (default 1M ids = 8 MB), otherwise
// ids_dev is read where it lies.  Nothing of the index is written before every id has passed the range check.
int32_t remove_batch_locked(vers_ivf* h, const uint64_t* ids_host, const uint64_t* ids_dev, uint64_t n_ids, const vers_comm_t* comm,
                            uint64_t* out_removed) {
  VERS_HIP_TRY(hipDeviceSynchronize());  // searches still in flight on any stream read the rows and tables this call changes
  if (out_removed) *out_removed = 0;
  if (h->world > 1 && (comm == nullptr || comm->world != h->world || comm->rank != h->rank || !comm->all_gather))
    return fail(VERS_ERR_INVALID, "vers_ivf_remove_batch: a sharded handle needs vers_ivf_remove_batch_dev with the build's vers_comm_t (every rank calls)");
  if (n_ids == 0) return VERS_OK;
  if (h->k == 0) {
    if (h->up.open) return fail(VERS_ERR_EMPTY, "remove_batch while a streamed upload is in progress: the handle holds no index until vers_ivf_upload_end");
    return fail(VERS_ERR_INVALID, "vers_ivf_remove_batch: vec id out of range (the index holds no vectors)");
  }
  const uint32_t k = h->k;
  const uint64_t n = h->n_total;
  const hipStream_t st = nullptr;
  auto& rm = h->rm;
  const size_t words = (size_t)((n + 31) / 32);
  const uint64_t chunk = std::min<uint64_t>(n_ids, (uint64_t)std::max<int64_t>(1, opt_get("remove_batch_ids", 1 << 20)));
  if (int32_t rc = rm.bitmap.reserve((words ? words : 1) * sizeof(uint32_t))) return rc;
  if (int32_t rc = rm.cnt.reserve((2 * (size_t)k + 1) * sizeof(uint32_t))) return rc;
  if (h->world > 1)
    if (int32_t rc = rm.gath.reserve((size_t)h->world * k * sizeof(uint32_t))) return rc;
  if (ids_host) {
    if (int32_t rc = rm.ids.reserve(chunk * sizeof(uint64_t))) return rc;
    if (rm.pin_cap < chunk * sizeof(uint64_t)) {
      rm.free_pin();
      VERS_HIP_TRY(hipHostMalloc(&rm.pin, chunk * sizeof(uint64_t), hipHostMallocDefault));
      rm.pin_cap = chunk * sizeof(uint64_t);
    }
  }
  uint32_t* const rm_cnt = rm.cnt.as<uint32_t>();
  uint32_t* const first_tile = rm_cnt + k;
  uint32_t* const bad = rm_cnt + 2 * (size_t)k;
  ab_count(0, 1.0, g_rm);
  ab_count(1, (double)n_ids, g_rm);
  // 1. the ids as one bit per vec id, range-checked
  VERS_HIP_TRY(hipMemsetAsync(rm.bitmap.p, 0, (words ? words : 1) * sizeof(uint32_t), st));
  VERS_HIP_TRY(hipMemsetAsync(rm_cnt, 0, (size_t)k * sizeof(uint32_t), st));
  VERS_HIP_TRY(hipMemsetAsync(first_tile, 0xFF, (size_t)k * sizeof(uint32_t), st));
  VERS_HIP_TRY(hipMemsetAsync(bad, 0, sizeof(uint32_t), st));
  for (uint64_t s0 = 0; s0 < n_ids; s0 += chunk) {
    const uint64_t m = std::min<uint64_t>(chunk, n_ids - s0);
    const uint64_t* src = ids_dev ? ids_dev + s0 : rm.ids.as<uint64_t>();
    if (ids_host) {
      AbClock clk(3, g_rm);
      std::memcpy(rm.pin, ids_host + s0, (size_t)m * sizeof(uint64_t));
      VERS_HIP_TRY(hipMemcpyAsync(rm.ids.p, rm.pin, (size_t)m * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      if (int32_t rc = clk.done()) return rc;
    }
    AbClock clk(4, g_rm);
    hipLaunchKernelGGL(remove_mark_ids_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, src, m, n, rm.bitmap.as<uint32_t>(), bad);
    VERS_HIP_TRY(hipGetLastError());
    if (int32_t rc = clk.done()) return rc;  // (the pinned chunk and rm.ids are free again)
  }
  std::vector<uint32_t> cnt_own(2 * (size_t)k), tot(k);
  {
    // 2. one pass over row_ids: rows removed per list, first tile of each list that loses one
    AbClock clk(4, g_rm);
    uint32_t any_bad = 0;
    VERS_HIP_TRY(hipMemcpy(&any_bad, bad, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (any_bad) return fail(VERS_ERR_INVALID, "vers_ivf_remove_batch: vec id >= n (assignments.len() = " + std::to_string(n) + "): nothing removed");
    if (h->cap_rows) {
      const uint64_t blocks = std::min<uint64_t>((uint64_t)h->n_cu * 8, (h->cap_rows + 255) / 256);
      hipLaunchKernelGGL(remove_scan_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const uint32_t*)h->row_ids.as<uint32_t>(), h->cap_rows,
                         (const uint32_t*)rm.bitmap.as<uint32_t>(), n, (const uint32_t*)h->list_off.as<uint32_t>(), k, rm_cnt, first_tile);
      VERS_HIP_TRY(hipGetLastError());
    }
    VERS_HIP_TRY(hipMemcpy(cnt_own.data(), rm_cnt, 2 * (size_t)k * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (h->world > 1) {  // the one exchange of the call: every rank's counts (zero for lists it does not own), summed
      if (int32_t rc = comm_rc(comm->all_gather(comm->ctx, rm_cnt, rm.gath.p, (uint64_t)k * sizeof(uint32_t)), "all_gather")) return rc;
      std::vector<uint32_t> all((size_t)h->world * k);
      VERS_HIP_TRY(hipMemcpy(all.data(), rm.gath.p, all.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
      for (uint32_t c = 0; c < k; ++c) {
        uint64_t s = 0;
        for (uint32_t r = 0; r < h->world; ++r) s += all[(size_t)r * k + c];
        tot[c] = (uint32_t)std::min<uint64_t>(s, 0xFFFFFFFFull);
      }
    } else {
      std::copy(cnt_own.begin(), cnt_own.begin() + k, tot.begin());
    }
    if (int32_t rc = clk.done()) return rc;
  }
  // 3. jobs of the owned lists that lose rows, the tiles they touch, the new global lengths -- all checked before anything is written
  std::vector<uint32_t> nl(h->h_len);
  std::vector<RemoveJob> jobs;
  std::vector<uint32_t> tiles;
  uint64_t removed = 0;
  for (uint32_t c = 0; c < k; ++c) {
    if (tot[c] > h->h_len[c]) return fail(VERS_ERR_HIP, "vers_ivf_remove_batch: more rows of a list marked than it holds (inconsistent index)");
    nl[c] -= tot[c];
    removed += tot[c];
    if (!cnt_own[c]) continue;
    const uint32_t t0 = h->h_off[c] / 64u, t_end = (uint32_t)(((uint64_t)h->h_off[c] + h->h_len[c] + 63) / 64), ft = cnt_own[k + c];
    if (h->h_owner[c] != h->rank || ft < t0 || ft >= t_end || (uint64_t)t_end * 64 > (uint64_t)h->h_off[c] + h->h_cap[c] || (uint64_t)t_end * 64 > h->cap_rows)
      return fail(VERS_ERR_HIP, "vers_ivf_remove_batch: a marked row lies outside its list (inconsistent index)");
    jobs.push_back(RemoveJob{h->h_off[c], h->h_len[c], ft - t0});
    for (uint32_t t = ft; t < t_end; ++t) tiles.push_back(t);
  }
  if (removed == 0) return VERS_OK;
  const uint32_t nj = (uint32_t)jobs.size(), nt = (uint32_t)tiles.size();
  const size_t jobs_b = (size_t)nj * sizeof(RemoveJob);
  {
    AbClock clk(5, g_rm);
    if (nj) {
      if (int32_t rc = rm.jobs.reserve(jobs_b + (size_t)nt * sizeof(uint32_t))) return rc;
      VERS_HIP_TRY(hipMemcpy(rm.jobs.p, jobs.data(), jobs_b, hipMemcpyHostToDevice));
      VERS_HIP_TRY(hipMemcpy(rm.jobs.as<char>() + jobs_b, tiles.data(), (size_t)nt * sizeof(uint32_t), hipMemcpyHostToDevice));
      hipLaunchKernelGGL(remove_compact_kernel, dim3(nj), dim3(kRmWaves * 64), 0, st, (const RemoveJob*)rm.jobs.p, (const uint32_t*)rm.bitmap.as<uint32_t>(), n,
                         h->ld, h->rows.as<float>(), h->row_ids.as<uint32_t>());
      VERS_HIP_TRY(hipGetLastError());
    }
    if (int32_t rc = clk.done()) return rc;
  }
  {
    // 4. tables: lengths by list and by slot (the slot ORDER is a scheduling heuristic and stays), the host's copies, and what the
    // host derives from the lengths: the longest list and len_asc_prefix (reference-mode depth, reference-mode batches as nprobe = 1)
    AbClock clk(6, g_rm);
    std::vector<uint32_t> sl(k);
    for (uint32_t c = 0; c < k; ++c) sl[h->h_slot[c]] = nl[c];
    VERS_HIP_TRY(hipMemcpy(h->list_len.p, nl.data(), (size_t)k * sizeof(uint32_t), hipMemcpyHostToDevice));
    VERS_HIP_TRY(hipMemcpy(h->slot_len.p, sl.data(), (size_t)k * sizeof(uint32_t), hipMemcpyHostToDevice));
    h->h_len = nl;
    h->max_len = 0;
    for (uint32_t c = 0; c < k; ++c) h->max_len = std::max(h->max_len, nl[c]);
    h->set_len_asc_prefix();
    if (int32_t rc = clk.done()) return rc;
  }
  {
    // 5. derived arrays of the touched tiles.  The running maxima in pre_misc (max |x|^2, max fp16 residual) only grow: after a removal
    // they are still upper bounds of what the certificates charge, merely not tight.
    AbClock clk(7, g_rm);
    if (int32_t rc = refresh_tiles(h, (const uint32_t*)(rm.jobs.as<char>() + jobs_b), nt, st)) return rc;
    if (int32_t rc = clk.done()) return rc;
  }
  ab_count(2, (double)removed, g_rm);
  if (out_removed) *out_removed = removed;
  return VERS_OK;
}

// ---- update_batch: values[v] = x for many v, each row to the list of its first-minimum centroid (see vers_hip.h) -------------------------
constexpr int kUpdatePhases = 10;
static double g_up[kUpdatePhases] = {};  // vers_update_phases: calls, rows, stayed, moved, stage, assign, mark + locate, overwrite, compact + merge, tables + derive (ms)

// rows [s0, s0 + m) of the call -> ab.stage [m][ldx], zero-padded (add_batch_locked's staging: through the pinned buffer, or from rows_dev)
static int32_t update_stage_chunk(vers_ivf* h, const float* rows_host, uint64_t row_stride_bytes, const float* rows_dev, uint64_t ld_floats, uint64_t s0,
                                  uint32_t m) {
  const uint32_t ldx = h->ldx, d = h->d;
  auto& ab = h->ab;
  if (rows_host) {
    float* pin = (float*)ab.pin;
    for (uint64_t i = 0; i < m; ++i) {
      float* dst = pin + i * ldx;
      std::memcpy(dst, (const char*)rows_host + (s0 + i) * row_stride_bytes, (size_t)d * 4);
      for (uint32_t j = d; j < ldx; ++j) dst[j] = 0.0f;
    }
    VERS_HIP_TRY(hipMemcpyAsync(ab.stage.p, pin, (size_t)m * ldx * 4, hipMemcpyHostToDevice, nullptr));
  } else {
    const uint64_t blocks = std::min<uint64_t>((uint64_t)h->n_cu * 8, ((uint64_t)m * (ldx / 4) + 255) / 256);
    hipLaunchKernelGGL(add_stage_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, nullptr, rows_dev + s0 * ld_floats, ld_floats, d, ldx, (uint64_t)m,
                       ab.stage.as<float>());
    VERS_HIP_TRY(hipGetLastError());
  }
  return VERS_OK;
}

// ALL OR NOTHING: the range and duplicate checks (mark), the assignment of every row (NaN) and the plan (locate, lengths, at most one
// re-layout, which moves rows but changes nothing observable) come before the first stored row is written.  A call of more than one staging
// chunk (option "add_batch_rows") therefore stages its rows TWICE: once to assign and check, once to place -- the second pass over the
// caller's rows is the price of refusing a NaN in the last chunk with the index untouched.  dev: the outputs but out_counts are device memory.
int32_t update_batch_locked(vers_ivf* h, const uint64_t* ids_host, const uint64_t* ids_dev, const float* rows_host, uint64_t row_stride_bytes,
                            const float* rows_dev, uint64_t ld_floats, uint64_t n, bool dev, uint64_t* out_clusters, uint8_t* out_status, uint64_t* out_counts,
                            const vers_comm_t* comm = nullptr) {
  // comm != nullptr: vers_ivf_update_batch_sharded_dev -- the handle is sharded by cluster (or a one-rank communicator stands in for that):
  // every rank runs the same call; what differs is marked `sh` below.  The where round (shard_where.hpp) sits between locate and the plan.
  const bool sh = comm != nullptr;
  VERS_HIP_TRY(hipDeviceSynchronize());  // searches still in flight on any stream read the rows and tables this call changes
  if (h->world > 1 && !sh)
    return fail(VERS_ERR_INVALID, "vers_ivf_update_batch: a handle sharded by cluster is not supported (the old and the new owner of a row differ)");
  if (n == 0) {
    if (out_counts) std::fill(out_counts, out_counts + 4, 0ull);
    return VERS_OK;
  }
  if (h->k == 0) {
    if (h->up.open) return fail(VERS_ERR_EMPTY, "update_batch while a streamed upload is in progress: the handle holds no index until vers_ivf_upload_end");
    return fail(VERS_ERR_EMPTY, "update_batch on an index without centroids");
  }
  const uint32_t k = h->k, ldx = h->ldx;
  const uint64_t nt_ids = h->n_total;
  if (n > nt_ids) return fail(VERS_ERR_INVALID, "vers_ivf_update_batch: more ids than the index ever held (one is out of range or repeated): nothing updated");
  const hipStream_t st = nullptr;
  auto& ud = h->ud;
  auto& ab = h->ab;
  const size_t words = (size_t)((nt_ids + 31) / 32);
  const uint64_t chunk = std::min<uint64_t>(n, (uint64_t)std::max<int64_t>(1, opt_get("add_batch_rows", 131072)));
  if (int32_t rc = ud.slot.reserve(nt_ids * sizeof(uint32_t))) return rc;
  if (int32_t rc = ud.a32.reserve(n * sizeof(uint32_t))) return rc;
  if (int32_t rc = ud.status.reserve(n)) return rc;
  if (int32_t rc = ud.rel.reserve(n * sizeof(uint32_t))) return rc;
  if (int32_t rc = ud.mv_row.reserve(n * sizeof(uint32_t))) return rc;
  if (int32_t rc = ud.cnt.reserve((4 * (size_t)k + 2) * sizeof(uint32_t))) return rc;
  if (int32_t rc = ud.keys.reserve(2 * n * sizeof(uint64_t))) return rc;
  if (int32_t rc = ud.vals.reserve(2 * n * sizeof(uint64_t) + 2 * sizeof(uint64_t))) return rc;
  if (int32_t rc = h->rm.bitmap.reserve((words ? words : 1) * sizeof(uint32_t))) return rc;
  if (int32_t rc = ab.stage.reserve(chunk * ldx * sizeof(float))) return rc;
  if (int32_t rc = h->km.counts.reserve((2 * (size_t)k + 2) * sizeof(uint32_t))) return rc;
  if (int32_t rc = h->pre_misc.reserve(64)) return rc;
  if (sh) {  // (before any exchange: a rank without these cannot join the where round at all -- the host aborts the group)
    if (int32_t rc = ud.where.reserve((n + 1) * sizeof(uint32_t))) return rc;
    if (int32_t rc = ud.gstat.reserve(n)) return rc;
    if (int32_t rc = h->rm.gath.reserve((size_t)h->world * (n + 1) * sizeof(uint32_t))) return rc;
  }
  if (rows_host && ab.pin_cap < chunk * ldx * sizeof(float)) {
    ab.free_pin();
    VERS_HIP_TRY(hipHostMalloc(&ab.pin, chunk * ldx * sizeof(float), hipHostMallocDefault));
    ab.pin_cap = chunk * ldx * sizeof(float);
  }
  uint32_t* const a32 = ud.a32.as<uint32_t>();
  uint32_t* const out_cnt = ud.cnt.as<uint32_t>();
  uint32_t* const first_tile = out_cnt + k;
  uint32_t* const in_cnt = out_cnt + 2 * (size_t)k;
  uint32_t* const mid_len = out_cnt + 3 * (size_t)k;
  uint32_t* const n_mv_dev = out_cnt + 4 * (size_t)k;
  uint32_t* const bad = n_mv_dev + 1;
  const uint64_t* ids = ids_dev;
  ab_count(0, 1.0, g_up);
  ab_count(1, (double)n, g_up);
  // 1. the ids: one table entry per vec id, range- and duplicate-checked
  {
    AbClock clk(6, g_up);
    if (ids_host) {
      if (int32_t rc = ud.ids.reserve(n * sizeof(uint64_t))) return rc;
      VERS_HIP_TRY(hipMemcpy(ud.ids.p, ids_host, n * sizeof(uint64_t), hipMemcpyHostToDevice));
      ids = ud.ids.as<uint64_t>();
    }
    VERS_HIP_TRY(hipMemsetAsync(ud.slot.p, 0xFF, nt_ids * sizeof(uint32_t), st));
    VERS_HIP_TRY(hipMemsetAsync(bad, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(update_mark_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ids, n, nt_ids, ud.slot.as<uint32_t>(), bad);
    VERS_HIP_TRY(hipGetLastError());
    uint32_t any_bad = 0;
    VERS_HIP_TRY(hipMemcpy(&any_bad, bad, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (int32_t rc = clk.done()) return rc;
    if (any_bad & 1u) return fail(VERS_ERR_INVALID, "vers_ivf_update_batch: vec id >= n (assignments.len() = " + std::to_string(nt_ids) + "): nothing updated");
    if (any_bad & 2u) return fail(VERS_ERR_INVALID, "vers_ivf_update_batch: the same vec id twice in one call: nothing updated");
  }
  // 2. first-minimum centroid of every row of the call (ivfflat.rs:201-207), chunk by chunk
  const bool one_chunk = chunk >= n;
  for (uint64_t s0 = 0; s0 < n; s0 += chunk) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - s0);
    {
      AbClock clk(4, g_up);
      if (int32_t rc = update_stage_chunk(h, rows_host, row_stride_bytes, rows_dev, ld_floats, s0, m)) return rc;
      if (int32_t rc = clk.done()) return rc;
    }
    AbClock clk(5, g_up);
    if (k == 1) {  // one centroid: every row stays there, a NaN one included (nothing is compared)
      VERS_HIP_TRY(hipMemsetAsync(a32 + s0, 0, (size_t)m * sizeof(uint32_t), st));
    } else {
      if (int32_t rc = h->km.status.reserve(16)) return rc;
      VERS_HIP_TRY(hipMemsetAsync(h->km.status.p, 0, 16, st));
      if (int32_t rc = (km_use_mfma(m, k, h->d) ? km_assign_mfma : km_assign)(ab.stage.as<float>(), ldx, m, h->centroids.as<float>(), ldx, k, h->d, a32 + s0,
                                                                              nullptr, h->km, h->n_cu, st, h->metric))
        return rc;
      uint32_t stw = 0;
      VERS_HIP_TRY(hipMemcpy(&stw, h->km.status.p, 4, hipMemcpyDeviceToHost));
      if (stw & 1u) {
        VERS_HIP_TRY(hipMemsetAsync(h->km.status.p, 0, 16, st));
        VERS_HIP_TRY(hipStreamSynchronize(st));
        return fail(VERS_ERR_NAN, "NaN distance in update_batch (rows " + std::to_string(s0) + " .. " + std::to_string(s0 + m) + "): nothing updated");
      }
    }
    if (int32_t rc = clk.done()) return rc;
  }
  // 3. locate: who stays where, who leaves which list for which
  std::vector<uint32_t> cnt(3 * (size_t)k);
  std::vector<uint8_t> status(n);
  std::vector<uint32_t> a_host(n), rel;
  uint32_t n_mv = 0;
  uint64_t* const keys_in = ud.keys.as<uint64_t>();
  uint64_t* const keys_out = keys_in + n;
  uint64_t* const vals_in = ud.vals.as<uint64_t>();
  uint64_t* const vals_out = vals_in + n;
  uint64_t* const lims = vals_out + n;
  {
    AbClock clk(6, g_up);
    VERS_HIP_TRY(hipMemsetAsync(bad, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(add_check_assign_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a32, (uint32_t)n, k, bad);
    VERS_HIP_TRY(hipMemsetAsync(ud.status.p, upd::kSkipped, n, st));
    VERS_HIP_TRY(hipMemsetAsync(h->rm.bitmap.p, 0, (words ? words : 1) * sizeof(uint32_t), st));
    VERS_HIP_TRY(hipMemsetAsync(out_cnt, 0, (size_t)k * sizeof(uint32_t), st));
    VERS_HIP_TRY(hipMemsetAsync(first_tile, 0xFF, (size_t)k * sizeof(uint32_t), st));
    VERS_HIP_TRY(hipMemsetAsync(in_cnt, 0, (size_t)k * sizeof(uint32_t), st));
    VERS_HIP_TRY(hipMemsetAsync(n_mv_dev, 0, sizeof(uint32_t), st));
    if (sh) VERS_HIP_TRY(hipMemsetAsync(ud.where.p, 0xFF, n * sizeof(uint32_t), st));  // (an id this rank stores in no list)
    if (h->cap_rows) {
      const uint64_t blocks = std::min<uint64_t>((uint64_t)h->n_cu * 8, (h->cap_rows + 255) / 256);
      hipLaunchKernelGGL(update_locate_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const uint32_t*)h->row_ids.as<uint32_t>(), h->cap_rows,
                         (const uint32_t*)ud.slot.as<uint32_t>(), nt_ids, (const uint32_t*)h->list_off.as<uint32_t>(), k, (const uint32_t*)a32,
                         ud.status.as<uint8_t>(), ud.rel.as<uint32_t>(), h->rm.bitmap.as<uint32_t>(), out_cnt, first_tile, in_cnt, n_mv_dev, (uint32_t)n, keys_in, vals_in,
                         sh ? ud.where.as<uint32_t>() : (uint32_t*)nullptr);
    }
    VERS_HIP_TRY(hipGetLastError());
    uint32_t tail[2] = {0, 0};
    VERS_HIP_TRY(hipMemcpy(cnt.data(), out_cnt, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    VERS_HIP_TRY(hipMemcpy(tail, n_mv_dev, sizeof(tail), hipMemcpyDeviceToHost));
    VERS_HIP_TRY(hipMemcpy(status.data(), ud.status.p, n, hipMemcpyDeviceToHost));
    VERS_HIP_TRY(hipMemcpy(a_host.data(), a32, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (tail[1]) return fail(VERS_ERR_HIP, "vers_ivf_update_batch: the assign pass returned a cluster index out of range");  // (centroids are replicated: every rank alike)
    n_mv = tail[0];
    if (int32_t rc = clk.done()) return rc;
  }
  uint64_t stayed = 0, moved = 0, skipped = 0;
  for (uint64_t i = 0; i < n; ++i) (status[i] == upd::kStayed ? stayed : status[i] == upd::kMoved ? moved : skipped) += 1;
  // On a sharded handle what this rank's own rows show wrong is a LOCAL failure: it travels in the status word of the where round.
  int32_t local_rc = VERS_OK;
  std::string local_why;
  auto refuse = [&](const char* msg) -> int32_t {
    const int32_t e = fail(VERS_ERR_HIP, msg);
    if (sh && !local_rc) { local_rc = e; local_why = msg; }
    return e;
  };
  if (moved != n_mv)
    if (int32_t e = refuse("vers_ivf_update_batch: a vec id is stored twice (inconsistent index)"); !sh) return e;
  // 4. the plan: lengths in between and afterwards, the jobs of both kernels (list-relative: a re-layout may follow)
  const uint32_t* const c_out = cnt.data();
  const uint32_t* const c_ft = cnt.data() + k;
  const uint32_t* c_in = cnt.data() + 2 * (size_t)k;
  for (uint32_t c = 0; c < k; ++c)
    if (c_out[c] > h->h_len[c] || (c_out[c] && (uint64_t)c_ft[c] * 64 >= h->h_len[c]) || (sh && c_out[c] && h->h_owner.size() == k && h->h_owner[c] != h->rank)) {
      if (int32_t e = refuse("vers_ivf_update_batch: a located row lies outside its list (inconsistent index)"); !sh) return e;
      break;
    }
  std::vector<uint32_t> mid(k), nl(k), g_in;
  bool own_io = moved != 0;  // this rank compacts or merges something
  uint64_t moved_any = moved;  // rows that moved anywhere (prepared filters, fetch maps, tables)
  bool grow = false;
  if (sh) {
    // 4a. the where round -- ONE all_gather of n + 1 words per rank -- and the resolve pass over the gathered table
    AbClock clk(6, g_up);
    const uint32_t world = h->world, me = h->rank;
    const size_t nw = (size_t)n + 1;
    if (!local_rc && test_fail_sharded_ref().load() > 0 && test_fail_sharded_ref().fetch_sub(1) > 0) (void)refuse("vers_ivf_update_batch_sharded_dev: injected local failure (test hook)");
    uint32_t* const send = ud.where.as<uint32_t>();
    if (local_rc) VERS_HIP_TRY(hipMemsetAsync(send, 0xFF, n * sizeof(uint32_t), st));
    const uint32_t stw = (uint32_t)local_rc;
    VERS_HIP_TRY(hipMemcpy(send + n, &stw, sizeof(stw), hipMemcpyHostToDevice));
    VERS_HIP_TRY(hipDeviceSynchronize());
    uint32_t* const table = h->rm.gath.as<uint32_t>();
    if (int32_t crc = comm->all_gather(comm->ctx, send, table, (uint64_t)nw * sizeof(uint32_t)))
      return local_rc ? fail(local_rc, local_why) : comm_rc(crc, "all_gather");
    for (uint32_t r = 0; r < world; ++r) {  // the agreement: the first failing rank's status, in rank order
      uint32_t s = 0;
      VERS_HIP_TRY(hipMemcpy(&s, table + (size_t)r * nw + n, sizeof(s), hipMemcpyDeviceToHost));
      if (s == 0) continue;
      if (r == me && local_rc) return fail((int32_t)s, local_why);
      return fail((int32_t)s, "vers_ivf_update_batch_sharded_dev: rank " + std::to_string(r) + " reported status " + std::to_string(s) + "; nothing updated");
    }
    // (mid_len's place holds the rows leaving every list until the host has read them)
    VERS_HIP_TRY(hipMemsetAsync(in_cnt, 0, (size_t)k * sizeof(uint32_t), st));
    VERS_HIP_TRY(hipMemsetAsync(mid_len, 0, (size_t)k * sizeof(uint32_t), st));
    VERS_HIP_TRY(hipMemsetAsync(n_mv_dev, 0, 2 * sizeof(uint32_t), st));
    DevBuf own_tmp;  // (a one-rank communicator on an unsharded handle: every list is this rank's)
    const uint8_t* owner_dev = h->owner.as<uint8_t>();
    if (h->h_owner.size() != k || owner_dev == nullptr) {
      if (int32_t rc = own_tmp.reserve(k)) return rc;
      VERS_HIP_TRY(hipMemsetAsync(own_tmp.p, 0, k, st));
      owner_dev = own_tmp.as<uint8_t>();
    }
    hipLaunchKernelGGL(update_resolve_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const uint32_t*)table, world, me, ids, (uint32_t)n,
                       owner_dev, k, (const uint32_t*)a32, ud.gstat.as<uint8_t>(), ud.status.as<uint8_t>(), mid_len, in_cnt, n_mv_dev, keys_in,
                       vals_in, bad);
    VERS_HIP_TRY(hipGetLastError());
    std::vector<uint8_t> gstat(n);
    std::vector<uint32_t> g_out(k);
    g_in.resize(k);
    uint32_t tail[2] = {0, 0};
    VERS_HIP_TRY(hipMemcpy(tail, n_mv_dev, sizeof(tail), hipMemcpyDeviceToHost));
    VERS_HIP_TRY(hipMemcpy(gstat.data(), ud.gstat.p, n, hipMemcpyDeviceToHost));
    VERS_HIP_TRY(hipMemcpy(status.data(), ud.status.p, n, hipMemcpyDeviceToHost));  // from here on: this rank's part
    VERS_HIP_TRY(hipMemcpy(g_out.data(), mid_len, (size_t)k * sizeof(uint32_t), hipMemcpyDeviceToHost));
    VERS_HIP_TRY(hipMemcpy(g_in.data(), in_cnt, (size_t)k * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (int32_t rc = clk.done()) return rc;
    if (tail[1]) return fail(VERS_ERR_HIP, "vers_ivf_update_batch_sharded_dev: a vec id is claimed by two ranks, or by a rank that does not own its list (inconsistent index); nothing updated");
    n_mv = tail[0];
    stayed = moved = skipped = 0;
    for (uint64_t i = 0; i < n; ++i) (gstat[i] == upd::kStayed ? stayed : gstat[i] == upd::kMoved ? moved : skipped) += 1;
    moved_any = moved;
    bool any_out = false;
    for (uint32_t c = 0; c < k; ++c) {
      const bool mine_c = h->h_owner.size() != k || h->h_owner[c] == me;
      if (g_out[c] > h->h_len[c] || (mine_c && g_out[c] != c_out[c]))
        return fail(VERS_ERR_HIP, "vers_ivf_update_batch_sharded_dev: the gathered table and this rank's lists disagree (inconsistent index); nothing updated");
      mid[c] = h->h_len[c] - g_out[c];
      nl[c] = mid[c] + g_in[c];
      if (!mine_c) g_in[c] = 0;  // (the merge jobs: owned lists only)
      else if (nl[c] > h->h_cap[c]) grow = true;
      any_out = any_out || c_out[c] != 0;
    }
    c_in = g_in.data();
    own_io = any_out || n_mv != 0;
  } else {
    grow = moved != 0 && upd::plan_lengths(h->h_len.data(), c_out, c_in, h->h_cap.data(), k, mid.data(), nl.data());
    if (moved == 0) { mid = h->h_len; nl = h->h_len; }
  }
  uint64_t relayouts = 0;
  if (grow) {
    AbClock clk(8, g_up);
    // relayout_for copies the rows a list holds NOW (h_len) into the room planned for the length it is given: a list that shrinks in this
    // call (its movers leave after the re-layout, below) keeps room for its old length -- planned for the new one, its tiles would be
    // copied, and then compacted, over the storage of the lists behind it
    std::vector<uint32_t> room(k);
    for (uint32_t c = 0; c < k; ++c) room[c] = std::max(h->h_len[c], nl[c]);
    if (int32_t rc = relayout_for(h, room.data())) return rc;
    relayouts = 1;
    if (int32_t rc = clk.done()) return rc;
  }
  // 5. the movers in (new list, vec id) order; every update's place among them
  if (n_mv) {
    AbClock clk(8, g_up);
    const uint64_t lim_host[2] = {0, n_mv};
    const size_t tmp_b = range_sort_temp_bytes(n_mv, 1);
    if (int32_t rc = ud.tmp.reserve(tmp_b)) return rc;
    if (int32_t rc = ud.pos.reserve((size_t)n_mv * sizeof(uint32_t))) return rc;
    if (int32_t rc = ud.mstage.reserve((size_t)n_mv * ldx * sizeof(float))) return rc;
    VERS_HIP_TRY(hipMemcpy(lims, lim_host, sizeof(lim_host), hipMemcpyHostToDevice));
    if (int32_t rc = range_sort_segments(keys_in, keys_out, vals_in, vals_out, n_mv, 1, lims, ud.tmp.p, tmp_b, st)) return rc;
    hipLaunchKernelGGL(update_mover_rows_kernel, dim3((n_mv + 255) / 256), dim3(256), 0, st, (const uint64_t*)vals_out, n_mv, ud.mv_row.as<uint32_t>());
    VERS_HIP_TRY(hipGetLastError());
    if (int32_t rc = clk.done()) return rc;
  }
  // 6. placement of the staged rows: stays over their storage rows, movers into their stage.  THE FIRST WRITE to a stored row.
  if (moved_any) h->flt_moved += 1;  // (prepared filters, fetch maps: storage rows change their vec ids from here on -- on a sharded handle on EVERY rank when anything moved anywhere)
  for (uint64_t s0 = 0; s0 < n; s0 += chunk) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - s0);
    if (!one_chunk) {
      AbClock clk(4, g_up);
      if (int32_t rc = update_stage_chunk(h, rows_host, row_stride_bytes, rows_dev, ld_floats, s0, m)) return rc;
      if (int32_t rc = clk.done()) return rc;
    }
    AbClock clk(7, g_up);
    const uint64_t blocks = std::min<uint64_t>((uint64_t)h->n_cu * 8, ((uint64_t)m * (h->ld / 4) + 255) / 256);
    hipLaunchKernelGGL(update_place_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)ab.stage.as<float>(), ldx, h->ld, s0, m,
                       (const uint8_t*)ud.status.as<uint8_t>(), (const uint32_t*)a32, (const uint32_t*)ud.rel.as<uint32_t>(),
                       (const uint32_t*)ud.mv_row.as<uint32_t>(), (const uint32_t*)h->list_off.as<uint32_t>(), h->rows.as<float>(), ud.mstage.as<float>());
    VERS_HIP_TRY(hipGetLastError());
    if (int32_t rc = clk.done()) return rc;
  }
  // 7. the touched tiles: of the stays, of the lists that lose rows (from their first loss on), of the lists that gain rows (from their
  // first insertion point on -- known once the positions are computed, below)
  std::vector<uint32_t> tiles;
  if (stayed) {
    rel.resize(n);
    VERS_HIP_TRY(hipMemcpy(rel.data(), ud.rel.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n; ++i)
      if (status[i] == upd::kStayed) tiles.push_back((uint32_t)(((uint64_t)h->h_off[a_host[i]] + rel[i]) / 64));
  }
  if (own_io) {
    AbClock clk(8, g_up);
    std::vector<RemoveJob> rjobs;
    std::vector<MergeJob> mjobs;
    uint32_t run = 0;
    for (uint32_t c = 0; c < k; ++c) {
      if (c_out[c]) {
        rjobs.push_back(RemoveJob{h->h_off[c], h->h_len[c], c_ft[c]});
        for (uint32_t t = c_ft[c]; (uint64_t)t * 64 < h->h_len[c]; ++t) tiles.push_back(h->h_off[c] / 64u + t);
      }
      if (c_in[c]) mjobs.push_back(MergeJob{h->h_off[c], mid[c], c_in[c], run});
      run += c_in[c];
    }
    const size_t rj_b = rjobs.size() * sizeof(RemoveJob), mj_b = mjobs.size() * sizeof(MergeJob);
    if (int32_t rc = ud.jobs.reserve(rj_b + mj_b + 16)) return rc;
    if (rj_b) VERS_HIP_TRY(hipMemcpy(ud.jobs.p, rjobs.data(), rj_b, hipMemcpyHostToDevice));
    if (mj_b) VERS_HIP_TRY(hipMemcpy(ud.jobs.as<char>() + rj_b, mjobs.data(), mj_b, hipMemcpyHostToDevice));
    VERS_HIP_TRY(hipMemcpy(mid_len, mid.data(), (size_t)k * sizeof(uint32_t), hipMemcpyHostToDevice));
    // movers out: remove_batch's compaction with the bitmap the locate pass wrote
    if (!rjobs.empty())  // (a sharded handle: a rank may only gain rows, or only lose some)
    hipLaunchKernelGGL(remove_compact_kernel, dim3((unsigned)rjobs.size()), dim3(kRmWaves * 64), 0, st, (const RemoveJob*)ud.jobs.p,
                       (const uint32_t*)h->rm.bitmap.as<uint32_t>(), nt_ids, h->ld, h->rows.as<float>(), h->row_ids.as<uint32_t>());
    // movers in: insertion points against the compacted lists, then the backward merge
    if (n_mv)
    hipLaunchKernelGGL(update_positions_kernel, dim3((n_mv + 255) / 256), dim3(256), 0, st, (const uint64_t*)keys_out, n_mv, (const uint32_t*)h->list_off.as<uint32_t>(),
                       (const uint32_t*)mid_len, (const uint32_t*)h->row_ids.as<uint32_t>(), ud.pos.as<uint32_t>());
    if (!mjobs.empty())
    hipLaunchKernelGGL(update_merge_kernel, dim3((unsigned)mjobs.size()), dim3(kRmWaves * 64), 0, st, (const MergeJob*)(ud.jobs.as<char>() + rj_b),
                       (const uint32_t*)ud.pos.as<uint32_t>(), (const uint64_t*)keys_out, (const float*)ud.mstage.as<float>(), ldx, h->ld, h->rows.as<float>(),
                       h->row_ids.as<uint32_t>());
    VERS_HIP_TRY(hipGetLastError());
    std::vector<uint32_t> pos(n_mv);
    if (n_mv) VERS_HIP_TRY(hipMemcpy(pos.data(), ud.pos.p, (size_t)n_mv * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (const MergeJob& jb : mjobs)
      for (uint32_t t = upd::merge_first_tile(pos.data() + jb.in0); t <= upd::merge_last_tile(jb.len, jb.n_in); ++t) tiles.push_back(jb.off / 64u + t);
    if (int32_t rc = clk.done()) return rc;
  }
  {
    // 8. tables (as remove_batch) and the derived arrays of the touched tiles; the maxima in pre_misc only grow, as after a removal
    AbClock clk(9, g_up);
    if (moved_any) {
      std::vector<uint32_t> sl(k);
      for (uint32_t c = 0; c < k; ++c) sl[h->h_slot[c]] = nl[c];
      VERS_HIP_TRY(hipMemcpy(h->list_len.p, nl.data(), (size_t)k * sizeof(uint32_t), hipMemcpyHostToDevice));
      VERS_HIP_TRY(hipMemcpy(h->slot_len.p, sl.data(), (size_t)k * sizeof(uint32_t), hipMemcpyHostToDevice));
      h->h_len = nl;
      h->max_len = 0;
      for (uint32_t c = 0; c < k; ++c) h->max_len = std::max(h->max_len, nl[c]);
      h->set_len_asc_prefix();
    }
    {  // the union, each tile once, ascending (a mark per storage tile: a sort of one entry per updated row cost more than the kernels)
      std::vector<uint8_t> hit((size_t)(h->cap_rows / 64) + 1, 0);
      for (uint32_t t : tiles) hit[t] = 1;
      tiles.clear();
      for (size_t t = 0; t < hit.size(); ++t)
        if (hit[t]) tiles.push_back((uint32_t)t);
    }
    const uint32_t n_tiles = (uint32_t)tiles.size();
    if (n_tiles) {
      if (int32_t rc = ud.jobs.reserve((size_t)n_tiles * sizeof(uint32_t))) return rc;
      VERS_HIP_TRY(hipMemcpy(ud.jobs.p, tiles.data(), (size_t)n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice));
      if (int32_t rc = refresh_tiles(h, (const uint32_t*)ud.jobs.p, n_tiles, st)) return rc;
    }
    if (int32_t rc = clk.done()) return rc;
  }
  ab_count(2, (double)stayed, g_up);
  ab_count(3, (double)moved, g_up);
  // 9. the outputs, only now
  if (dev) {
    if (out_clusters) {
      hipLaunchKernelGGL(u32_to_u64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const uint32_t*)a32, n, out_clusters);
      VERS_HIP_TRY(hipGetLastError());
    }
    if (out_status) VERS_HIP_TRY(hipMemcpyAsync(out_status, sh ? ud.gstat.p : ud.status.p, n, hipMemcpyDeviceToDevice, st));  // (sharded: the status every rank derived)
    VERS_HIP_TRY(hipStreamSynchronize(st));
  } else {
    if (out_clusters)
      for (uint64_t i = 0; i < n; ++i) out_clusters[i] = a_host[i];
    if (out_status) std::memcpy(out_status, status.data(), n);
  }
  if (out_counts) { out_counts[0] = stayed; out_counts[1] = moved; out_counts[2] = skipped; out_counts[3] = relayouts; }
  return VERS_OK;
}

// ---- compact: back to plan_storage's capacities for the CURRENT lengths (see vers_hip.h) ------------------------------------------------
constexpr int kCompactPhases = 8;
static double g_cp[kCompactPhases] = {};  // vers_compact_phases: calls, storage rows before, after, plan + allocation, move, derive (unfused), tables (ms), reserved

// The shadow and the row-major copy of `rows` storage rows, decided as a build decides them (refresh_norms: options "shadow", "rowmajor",
// "memory"; both are optional memory with the same head-room left for the searches) and allocated through DevBuf::reserve.  *fits = false:
// a copy the options ask for found no room.
static void reserve_derived(vers_ivf* h, uint64_t rows, DevBuf& bf, DevBuf& rm, bool* fits) {
  *fits = true;
  const size_t n = (size_t)(rows ? rows : 1) * h->ld;
  size_t free_b = 0, total_b = 0;
  if (shadow_mode() != 0) {
    (void)hipMemGetInfo(&free_b, &total_b);
    if (n * sizeof(uint16_t) + (size_t(4) << 30) > free_b || bf.reserve(n * sizeof(uint16_t)) != VERS_OK) { (void)hipGetLastError(); bf.release(); *fits = false; }
  }
  const int rm_opt = (int)opt_get("rowmajor", -1);
  const int rm_mode = rm_opt < 0 && opt_get("memory", 0) == 1 ? 0 : rm_opt;
  (void)hipMemGetInfo(&free_b, &total_b);
  if (rm_mode == 1 || (rm_mode < 0 && n * sizeof(float) <= total_b / 4)) {
    if (n * sizeof(float) + (size_t(2) << 30) > free_b || rm.reserve(n * sizeof(float)) != VERS_OK) { (void)hipGetLastError(); rm.release(); *fits = false; }
  }
}

int32_t compact_locked(vers_ivf* h, uint64_t* out_before, uint64_t* out_after) {
  VERS_HIP_TRY(hipDeviceSynchronize());  // searches still in flight on any stream read the storage this call replaces
  if (out_before) *out_before = 0;
  if (out_after) *out_after = 0;
  if (h->up.open) return fail(VERS_ERR_EMPTY, "compact while a streamed upload is in progress: the handle holds no index until vers_ivf_upload_end");
  if (h->k == 0) return VERS_OK;
  const uint32_t k = h->k, ld = h->ld;
  const hipStream_t st = nullptr;
  const uint64_t before = h->cap_rows;
  std::vector<uint32_t> noff, ncap;
  std::vector<CompactJob> jobs;
  uint64_t total = 0;
  DevBuf nrows, nids, nxn, nbf, nrm, djobs, nmisc;
  const size_t lds = 64 * (size_t)(kGatherCols4 + 1) * sizeof(f32x4);
  bool fused = opt_get("compact_fused", 1) != 0;
  {
    AbClock clk(3, g_cp);
    if (int32_t rc = plan_capacities(h, h->h_len.data(), k, noff, ncap, &total)) return rc;
    for (uint32_t c = 0; c < k; ++c) {
      if (!h->h_len[c] || h->h_owner[c] != h->rank) continue;
      const uint32_t nt = (h->h_len[c] + 63u) / 64u;
      if (h->h_off[c] % 64u || (uint64_t)nt * 64 > h->h_cap[c] || (uint64_t)h->h_off[c] + h->h_cap[c] > h->cap_rows)
        return fail(VERS_ERR_HIP, "vers_ivf_compact: a list lies outside its storage (inconsistent index)");
      for (uint32_t t = 0; t < nt; ++t) jobs.push_back(CompactJob{h->h_off[c] / 64u + t, noff[c] / 64u + t});  // (t < nt <= ncap[c] / 64)
    }
    if (int32_t rc = h->pre_misc.reserve(64)) return rc;
    if (int32_t rc = nmisc.reserve(64)) return rc;  // the new maxima: pre_misc keeps the old ones until the move is done
    if (int32_t rc = scan_prepare_launch(compact_tiles_kernel, lds)) return rc;
    // the old shadow and row-major copy go first: they are derived, the new ones take their room
    h->shadow_valid = false;
    h->head_valid = false;
    h->balls_valid = false;
    h->rows_bf.release();
    h->rows_h8.release();
    h->rows_rm.release();
    const size_t rows_b = (size_t)(total ? total : 1) * ld * sizeof(float), ids_b = (size_t)(total ? total : 1) * sizeof(uint32_t);
    if (nrows.reserve(rows_b) != VERS_OK || nids.reserve(ids_b) != VERS_OK) {
      (void)hipGetLastError();
      nrows.release(); nids.release();
      if (int32_t rc = refresh_norms(h, 0, h->cap_rows, st)) return rc;  // the old index stays, with its derived arrays back
      VERS_HIP_TRY(hipStreamSynchronize(st));
      return fail(VERS_ERR_HIP, "vers_ivf_compact: the new tiles do not fit beside the old ones; the index is unchanged");
    }
    if (fused) {
      bool fits = true;
      reserve_derived(h, total, nbf, nrm, &fits);
      if (fits && (nxn.reserve(ids_b) != VERS_OK || djobs.reserve((jobs.size() ? jobs.size() : 1) * sizeof(CompactJob)) != VERS_OK)) { (void)hipGetLastError(); fits = false; }
      if (!fits) {  // not beside the old tiles: the unfused sequence allocates them once those are gone
        nbf.release(); nrm.release(); nxn.release(); djobs.release();
        fused = false;
      }
    }
    VERS_HIP_TRY(hipMemsetAsync(nids.p, 0xFF, ids_b, st));  // slack tiles of the new plan: no vector (their rows stay as allocated)
    if (int32_t rc = clk.done()) return rc;
  }
  ab_count(0, 1.0, g_cp);
  ab_count(1, (double)before, g_cp);
  ab_count(2, (double)total, g_cp);
  {
    AbClock clk(4, g_cp);
    if (fused) {
      VERS_HIP_TRY(hipMemsetAsync(nxn.p, 0, (size_t)(total ? total : 1) * sizeof(float), st));  // |x|^2 of a row without a vector: 0.0f
      VERS_HIP_TRY(hipMemsetAsync(nmisc.p, 0, 64, st));  // both maxima and the failure counter restart, as at an upload
      if (!jobs.empty()) {
        VERS_HIP_TRY(hipMemcpyAsync(djobs.p, jobs.data(), jobs.size() * sizeof(CompactJob), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(compact_tiles_kernel, dim3((unsigned)jobs.size()), dim3(256), lds, st, (const CompactJob*)djobs.p, ld,
                           (const float*)h->rows.as<float>(), (const uint32_t*)h->row_ids.as<uint32_t>(), nrows.as<float>(), nids.as<uint32_t>(),
                           nbf.as<uint16_t>(), nrm.as<float>(), nxn.as<float>(), nmisc.as<uint32_t>(), nmisc.as<uint32_t>() + 2);
        VERS_HIP_TRY(hipGetLastError());
      }
      VERS_HIP_TRY(hipMemcpyAsync(h->pre_misc.p, nmisc.p, 64, hipMemcpyDeviceToDevice, st));  // (a failure above leaves the old index and its maxima)
    } else {
      for (uint32_t c = 0; c < k; ++c) {  // relayout_for's copies with the new plan: whole 64-row tiles move as they are
        if (!h->h_len[c] || h->h_owner[c] != h->rank) continue;
        VERS_HIP_TRY(hipMemcpyAsync(nrows.as<float>() + (size_t)noff[c] * ld, h->rows.as<float>() + (size_t)h->h_off[c] * ld,
                                    (size_t)round_up(h->h_len[c], 64) * ld * sizeof(float), hipMemcpyDeviceToDevice, st));
        VERS_HIP_TRY(hipMemcpyAsync(nids.as<uint32_t>() + noff[c], h->row_ids.as<uint32_t>() + h->h_off[c], (size_t)h->h_len[c] * sizeof(uint32_t),
                                    hipMemcpyDeviceToDevice, st));
      }
    }
    VERS_HIP_TRY(hipDeviceSynchronize());
    std::swap(h->rows.p, nrows.p); std::swap(h->rows.cap, nrows.cap);
    std::swap(h->row_ids.p, nids.p); std::swap(h->row_ids.cap, nids.cap);
    nrows.release(); nids.release();
    if (fused) {
      std::swap(h->xnorm.p, nxn.p); std::swap(h->xnorm.cap, nxn.cap);
      std::swap(h->rows_bf.p, nbf.p); std::swap(h->rows_bf.cap, nbf.cap);
      std::swap(h->rows_rm.p, nrm.p); std::swap(h->rows_rm.cap, nrm.cap);
      nxn.release();
    } else {
      h->xnorm.release();  // (refresh_norms sizes it for the new plan)
    }
    if (int32_t rc = clk.done()) return rc;
  }
  {
    // tables, as after a fresh upload of the same lists: offsets, slots (order re-derived), tile -> list, the host's copies
    AbClock clk(6, g_cp);
    h->h_off = noff; h->h_cap = ncap; h->cap_rows = total;
    VERS_HIP_TRY(hipMemcpy(h->list_off.p, h->h_off.data(), (size_t)k * 4, hipMemcpyHostToDevice));
    if (int32_t rc = write_slot_tables(h, k)) return rc;
    h->set_len_asc_prefix();
    if (int32_t rc = write_tile_list(h, k)) return rc;
    if (fused) {  // what a full refresh_norms restarts besides the arrays
      for (auto& w : h->pool)
        for (auto& a : w->ahead) a.valid = false;
      h->shadow_valid = shadow_mode() != 0 && h->rows_bf.p != nullptr;
      h->shadow_off = false; h->shadow_queries = 0;
      if (shadow_mode() != 0) {
        if (!h->fail_watch) VERS_HIP_TRY(hipHostMalloc((void**)&h->fail_watch, 64, hipHostMallocDefault));
        *h->fail_watch = 0;
      }
    }
    if (int32_t rc = clk.done()) return rc;
  }
  if (!fused) {
    AbClock clk(5, g_cp);
    bool fits = true;
    reserve_derived(h, total, h->rows_bf, h->rows_rm, &fits);  // (what finds no room even now is optional memory: refresh_norms goes without)
    if (int32_t rc = refresh_norms(h, 0, h->cap_rows, st)) return rc;
    if (int32_t rc = clk.done()) return rc;
  } else {
    if (int32_t rc = build_head(h, st)) return rc;  // (the fused pass wrote every other derived array; the head is derived from the new tiles here)
    if (int32_t rc = build_balls(h, st)) return rc;
  }
  VERS_HIP_TRY(hipDeviceSynchronize());
  if (out_before) *out_before = before;
  if (out_after) *out_after = total;
  return VERS_OK;
}

// ---- recluster: build_index over the live rows in ascending vec id, the ids kept (see vers_hip.h) ----------------------------------------
constexpr int kReclusterPhases = 8;
static double g_rc[kReclusterPhases] = {};  // vers_recluster_phases: calls, live rows, gather, k-means, install, derived arrays, tables (ms), reserved

// Nothing of the handle changes before the COMMIT POINT below: the live rows are gathered into X' beside the index, run_build leaves its
// centroids in a buffer of the call's, and the new tiles are reserved while the old ones still stand (vers_ivf_compact's order).  A refusal,
// a NaN distance, a failed allocation and a call that keeps no attempt all return from above that point.
int32_t recluster_locked(vers_ivf* h, uint64_t num_clusters, uint64_t num_attempts, uint64_t max_iterations, const uint64_t* init_indices,
                         float* out_centroids, uint64_t c_stride_bytes, uint64_t* out_assignments, float* out_cost, int32_t* out_kept,
                         uint64_t* out_iterations) {
  VERS_HIP_TRY(hipDeviceSynchronize());  // searches still in flight on any stream read the storage this call replaces
  if (h->world > 1) return fail(VERS_ERR_INVALID, "vers_ivf_recluster: the handle is sharded by cluster (the build's exchanges are not wired into this call)");
  if (h->up.open) return fail(VERS_ERR_EMPTY, "recluster while a streamed upload is in progress: the handle holds no index until vers_ivf_upload_end");
  if (h->k == 0) return fail(VERS_ERR_EMPTY, "vers_ivf_recluster: the handle holds no centroids");
  uint64_t m = 0;
  for (uint32_t c = 0; c < h->k; ++c) m += h->h_len[c];
  if (m == 0) return fail(VERS_ERR_EMPTY, "vers_ivf_recluster: no live row");
  if (num_clusters == 0) return fail(VERS_ERR_EMPTY, "vers_ivf_recluster with zero clusters: min_by over no centroids (reference panics)");
  for (uint64_t i = 0; i < num_attempts * num_clusters; ++i)
    if (init_indices[i] >= m) return fail(VERS_ERR_INVALID, "vers_ivf_recluster: init index out of range (positions among the live rows, 0 .. m-1)");
  const uint32_t k_old = h->k, k = (uint32_t)num_clusters, ld = h->ld, ldx = h->ldx;
  const uint64_t n_total = h->n_total;
  const hipStream_t st = nullptr;
  double ph[kReclusterPhases] = {};  // this call's clocks: added to the totals where the call succeeds (a refused call counts nowhere)
  auto count_call = [&]() {
    ab_count(0, 1.0, g_rc);
    ab_count(1, (double)m, g_rc);
    for (int i = 2; i < kReclusterPhases; ++i) ab_count(i, ph[i], g_rc);
  };
  auto no_room = [&](const char* what) -> int32_t {
    (void)hipGetLastError();
    return fail(VERS_ERR_HIP, std::string("vers_ivf_recluster: ") + what + " do not fit beside the index; the index is unchanged");
  };
  DevBuf live, rank, L, X, dtiles, tmp;
  {
    AbClock clk(2, ph);
    std::vector<GatherJob> tiles;
    for (uint32_t c = 0; c < k_old; ++c) {
      if (!h->h_len[c]) continue;
      const uint32_t nt = (h->h_len[c] + 63u) / 64u;
      if (h->h_off[c] % 64u || (uint64_t)nt * 64 > h->h_cap[c] || (uint64_t)h->h_off[c] + h->h_cap[c] > h->cap_rows)
        return fail(VERS_ERR_HIP, "vers_ivf_recluster: a list lies outside its storage (inconsistent index)");
      for (uint32_t t = 0; t < nt; ++t) tiles.push_back(GatherJob{h->h_off[c] / 64u + t, std::min<uint32_t>(64u, h->h_len[c] - t * 64u)});
    }
    const size_t scan_tmp = range_scan_temp_bytes((size_t)n_total + 1);
    const size_t lds = 64 * (size_t)(kGatherCols4 + 1) * sizeof(f32x4) + 64 * sizeof(uint32_t);
    if (int32_t rc = scan_prepare_launch(tiles_to_live_rows_kernel, lds)) return rc;
    if (live.reserve(((size_t)n_total + 1) * sizeof(uint32_t)) != VERS_OK || rank.reserve(((size_t)n_total + 1) * sizeof(uint64_t)) != VERS_OK ||
        L.reserve((size_t)m * sizeof(uint32_t)) != VERS_OK || tmp.reserve(scan_tmp) != VERS_OK || dtiles.reserve(tiles.size() * sizeof(GatherJob)) != VERS_OK ||
        X.reserve((size_t)m * ldx * sizeof(float)) != VERS_OK)
      return no_room("the live rows");
    // the rank table: a count per vec id (+ one zero: the prefix's last entry is the number of live ids), its exclusive prefix, L
    VERS_HIP_TRY(hipMemsetAsync(live.p, 0, ((size_t)n_total + 1) * sizeof(uint32_t), st));
    VERS_HIP_TRY(hipMemcpyAsync(dtiles.p, tiles.data(), tiles.size() * sizeof(GatherJob), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(recluster_live_kernel, dim3((unsigned)((tiles.size() * 64 + 255) / 256)), dim3(256), 0, st, (const GatherJob*)dtiles.as<GatherJob>(),
                       (uint32_t)tiles.size(), (const uint32_t*)h->row_ids.as<uint32_t>(), n_total, live.as<uint32_t>());
    VERS_HIP_TRY(hipGetLastError());
    if (int32_t rc = range_scan_counts(live.as<uint32_t>(), rank.as<uint64_t>(), (size_t)n_total + 1, tmp.p, scan_tmp, st)) return rc;
    uint64_t counted = 0;
    VERS_HIP_TRY(hipMemcpyAsync(&counted, rank.as<uint64_t>() + n_total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    VERS_HIP_TRY(hipStreamSynchronize(st));
    if (counted != m) return fail(VERS_ERR_HIP, "vers_ivf_recluster: the lists do not hold as many distinct vec ids as their lengths say (inconsistent index)");
    hipLaunchKernelGGL(recluster_order_kernel, dim3((unsigned)((n_total + 255) / 256)), dim3(256), 0, st, (const uint32_t*)live.as<uint32_t>(),
                       (const uint64_t*)rank.as<uint64_t>(), n_total, m, L.as<uint32_t>());
    hipLaunchKernelGGL(tiles_to_live_rows_kernel, dim3((unsigned)tiles.size()), dim3(256), lds, st, (const float*)h->rows.as<float>(), ld, h->d, ldx,
                       (const GatherJob*)dtiles.as<GatherJob>(), (const uint32_t*)h->row_ids.as<uint32_t>(), (const uint64_t*)rank.as<uint64_t>(), n_total, m,
                       X.as<float>());
    VERS_HIP_TRY(hipGetLastError());
    if (int32_t rc = clk.done()) return rc;  // (tiles: read by the copy above, finished here)
  }
  DevBuf best_assign, newC;
  float cost = INFINITY;
  int32_t kept = 0;
  std::vector<uint64_t> iters(num_attempts ? num_attempts : 1, 0);
  {
    AbClock clk(3, ph);
    BuildShard one;
    one.n_total = m;
    if (int32_t rc = run_build(h, X.as<float>(), ldx, m, one, k, num_attempts, max_iterations, init_indices, best_assign, &cost, &kept, iters.data(), st, &newC))
      return rc;
    if (int32_t rc = clk.done()) return rc;
  }
  auto small_outputs = [&]() {
    if (out_cost) *out_cost = cost;
    *out_kept = kept;
    if (out_iterations)
      for (uint64_t a = 0; a < num_attempts; ++a) out_iterations[a] = iters[a];
  };
  if (!kept) {  // a maintenance call does not destroy what it was asked to improve: the index stays as it is (vers_ivf_build leaves an empty one)
    small_outputs();
    count_call();
    return VERS_OK;
  }
  DevBuf sorted, nrows, nids, a64;
  std::vector<uint32_t> lens, noff, ncap;
  uint64_t total = 0;
  {
    AbClock clk(4, ph);
    if (int32_t rc = group_for_install(h, m, best_assign.as<uint32_t>(), k, sorted, lens, st)) return rc;
    if (int32_t rc = plan_capacities(h, lens.data(), k, noff, ncap, &total, true)) return rc;
    // the old shadow, head and row-major copy go first: they are derived, the new tiles take their room
    h->shadow_valid = false;
    h->head_valid = false;
    h->balls_valid = false;
    h->rows_bf.release();
    h->rows_h8.release();
    h->rows_rm.release();
    if (nrows.reserve((size_t)(total ? total : 1) * ld * sizeof(float)) != VERS_OK || nids.reserve((size_t)(total ? total : 1) * sizeof(uint32_t)) != VERS_OK ||
        (out_assignments && a64.reserve((size_t)(n_total ? n_total : 1) * 8) != VERS_OK)) {
      (void)hipGetLastError();
      nrows.release(); nids.release(); a64.release();
      if (int32_t rc = refresh_norms(h, 0, h->cap_rows, st)) return rc;  // the old index stays, with its derived arrays back
      VERS_HIP_TRY(hipStreamSynchronize(st));
      return no_room("the new tiles");
    }
    if (int32_t rc = clk.done()) return rc;
  }
  // ---- COMMIT POINT: from here on the handle becomes the new index ----
  h->flt_moved += 1;  // (prepared filters: every storage row holds another vector, the tables have another k)
  std::swap(h->rows.p, nrows.p); std::swap(h->rows.cap, nrows.cap);
  std::swap(h->row_ids.p, nids.p); std::swap(h->row_ids.cap, nids.cap);
  nrows.release(); nids.release();
  std::swap(h->centroids.p, newC.p); std::swap(h->centroids.cap, newC.cap);
  newC.release();
  {
    AbClock clk(6, ph);
    if (int32_t rc = plan_storage(h, lens.data(), k, st)) return rc;  // (rows and row_ids: exactly the bytes reserved above, nothing is allocated)
    if (int32_t rc = clk.done()) return rc;
  }
  {
    AbClock clk(4, ph);
    if (int32_t rc = place_rows(h, X.as<float>(), ldx, m, best_assign.as<uint32_t>(), k, sorted, st)) return rc;
    hipLaunchKernelGGL(recluster_relabel_kernel, dim3((unsigned)((h->cap_rows + 255) / 256)), dim3(256), 0, st, h->row_ids.as<uint32_t>(), h->cap_rows,
                       (const uint32_t*)L.as<uint32_t>(), m);
    VERS_HIP_TRY(hipGetLastError());
    if (int32_t rc = clk.done()) return rc;
    X.release(); sorted.release(); L.release();  // (before the shadow and the row-major copy are allocated)
  }
  {
    AbClock clk(5, ph);
    if (int32_t rc = finish_index(h, k, n_total, st)) return rc;  // n_total: assignments.len() does not change
    if (int32_t rc = clk.done()) return rc;
  }
  if (out_centroids)
    VERS_HIP_TRY(hipMemcpy2D(out_centroids, (size_t)c_stride_bytes, h->centroids.p, (size_t)ldx * 4, (size_t)h->d * 4, k, hipMemcpyDeviceToHost));
  if (out_assignments && n_total) {
    hipLaunchKernelGGL(recluster_assign_out_kernel, dim3((unsigned)((n_total + 255) / 256)), dim3(256), 0, st, (const uint32_t*)live.as<uint32_t>(),
                       (const uint64_t*)rank.as<uint64_t>(), (const uint32_t*)best_assign.as<uint32_t>(), n_total, m, a64.as<uint64_t>());
    VERS_HIP_TRY(hipGetLastError());
    VERS_HIP_TRY(hipMemcpy(out_assignments, a64.p, n_total * 8, hipMemcpyDeviceToHost));
  }
  small_outputs();
  count_call();
  return VERS_OK;
}
}  // namespace ivf
}  // namespace vers

namespace {
// What an add / add_batch means to the prepared filters (vers_ivf::flt_moved / flt_appended), noted when the call leaves: rows written into
// list slack in place are an append; a re-layout has counted itself (relayout_for).
struct AppendNote {
  vers_ivf* h;
  uint64_t moved0, n0;
  explicit AppendNote(vers_ivf* hh) : h(hh), moved0(hh->flt_moved), n0(hh->n_total) {}
  ~AppendNote() {
    if (h->n_total != n0 && h->flt_moved == moved0) h->flt_appended += 1;
  }
};
}  // namespace

extern "C" {

int32_t vers_ivf_build(vers_ivf_t* h, const float* rows, uint64_t n, uint64_t row_stride_bytes, uint64_t num_clusters,
                       uint64_t num_attempts, uint64_t max_iterations, const uint64_t* init_indices, float* out_centroids,
                       uint64_t c_stride_bytes, uint64_t* out_assignments, float* out_cost, int32_t* out_kept,
                       uint64_t* out_iterations) {
  if (!h || (n && !rows) || row_stride_bytes < (uint64_t)(h ? h->d : 0) * 4 || row_stride_bytes % 4 ||
      (num_attempts * num_clusters && !init_indices) || n > 0xFFFFFFFFull || num_clusters > 0xFFFFFFFFull ||
      (out_centroids && num_clusters && c_stride_bytes < (uint64_t)h->d * 4))
    return fail(VERS_ERR_INVALID, "vers_ivf_build: bad arguments");
  std::unique_lock<std::shared_mutex> lk(h->index);
  h->flt_moved += 1;
  DeviceGuard g(h->device);
  DevBuf X;
  if (int32_t rc = X.reserve((n ? n : 1) * (size_t)h->ldx * sizeof(float))) return rc;
  if (n) {
    if (h->ldx != h->d) VERS_HIP_TRY(hipMemset(X.p, 0, n * (size_t)h->ldx * sizeof(float)));
    VERS_HIP_TRY(hipMemcpy2D(X.p, (size_t)h->ldx * 4, rows, row_stride_bytes, (size_t)h->d * 4, n, hipMemcpyHostToDevice));
  }
  BuildShard one;
  one.n_total = n;
  return build_common(h, X.as<float>(), h->ldx, n, one, num_clusters, num_attempts, max_iterations, init_indices, out_centroids,
                      c_stride_bytes, out_assignments, out_cost, out_kept, out_iterations);
}

int32_t vers_ivf_build_dev(vers_ivf_t* h, const float* rows_dev, uint64_t n, uint64_t ld_floats, uint64_t num_clusters,
                           uint64_t num_attempts, uint64_t max_iterations, const uint64_t* init_indices, float* out_centroids,
                           uint64_t c_stride_bytes, uint64_t* out_assignments, float* out_cost, int32_t* out_kept,
                           uint64_t* out_iterations) {
  if (!h || (n && !rows_dev) || ld_floats < (h ? h->d : 0) || ld_floats % 4 || ld_floats > 0x3FFFFFFFull ||
      (num_attempts * num_clusters && !init_indices) || n > 0xFFFFFFFFull || num_clusters > 0xFFFFFFFFull ||
      (out_centroids && num_clusters && c_stride_bytes < (uint64_t)h->d * 4))
    return fail(VERS_ERR_INVALID, "vers_ivf_build_dev: bad arguments (ld_floats must be >= d and a multiple of 4)");
  std::unique_lock<std::shared_mutex> lk(h->index);
  h->flt_moved += 1;
  DeviceGuard g(h->device);
  BuildShard one;
  one.n_total = n;
  return build_common(h, rows_dev, (uint32_t)ld_floats, n, one, num_clusters, num_attempts, max_iterations, init_indices, out_centroids, c_stride_bytes,
                      out_assignments, out_cost, out_kept, out_iterations);
}

int32_t vers_ivf_build_sharded_dev(vers_ivf_t* h, const float* rows_dev, uint64_t n_local, uint64_t ld_floats, uint64_t row_begin,
                                   uint64_t n_total, uint64_t num_clusters, uint64_t num_attempts, uint64_t max_iterations,
                                   const uint64_t* init_indices, const vers_comm_t* comm, uint64_t* out_assignments_local, float* out_cost,
                                   int32_t* out_kept, uint64_t* out_iterations) {
  if (!h || !comm || (n_local && !rows_dev) || ld_floats < (h ? h->d : 0) || ld_floats % 4 || ld_floats > 0x3FFFFFFFull ||
      (num_attempts * num_clusters && !init_indices) || n_total > 0xFFFFFFFFull || n_local > n_total || row_begin > n_total - n_local ||
      num_clusters > 0xFFFFFFFFull)
    return fail(VERS_ERR_INVALID, "vers_ivf_build_sharded_dev: bad arguments (ld_floats must be >= d and a multiple of 4; vec ids are 32-bit)");
  if (comm->world == 0 || comm->world > 255 || comm->rank >= comm->world ||
      (comm->world > 1 && (!comm->all_gather || !comm->send || !comm->recv || !comm->broadcast || !comm->all_to_all_v)))
    return fail(VERS_ERR_INVALID, "vers_ivf_build_sharded_dev: incomplete vers_comm_t");
  std::unique_lock<std::shared_mutex> lk(h->index);
  h->flt_moved += 1;
  DeviceGuard g(h->device);
  BuildShard sh;
  sh.comm = comm->world > 1 ? comm : nullptr;
  sh.rank = comm->rank; sh.world = comm->world; sh.row_begin = row_begin; sh.n_total = n_total;
  if (comm->world == 1 && (row_begin != 0 || n_local != n_total)) return fail(VERS_ERR_INVALID, "vers_ivf_build_sharded_dev: a single rank must hold every row");
  if (comm->world == 1) { h->rank = 0; h->world = 1; }
  return build_common(h, rows_dev, (uint32_t)ld_floats, n_local, sh, num_clusters, num_attempts, max_iterations, init_indices, nullptr, 0,
                      out_assignments_local, out_cost, out_kept, out_iterations);
}

int32_t vers_ivf_upload(vers_ivf_t* h, const float* rows, uint64_t n, uint64_t row_stride_bytes, const float* centroids,
                        uint64_t k, uint64_t c_stride_bytes, const uint64_t* assignments) {
  if (!h || (n && (!rows || !assignments)) || (k && !centroids) || row_stride_bytes < (uint64_t)(h ? h->d : 0) * 4 ||
      (k && c_stride_bytes < (uint64_t)h->d * 4) || n > 0xFFFFFFFFull || k > 0xFFFFFFFFull)
    return fail(VERS_ERR_INVALID, "vers_ivf_upload: bad arguments");
  // = the streamed sequence in one call: list lengths from the assignments, one chunk (staged through a bounded buffer), end
  std::vector<uint64_t> lens(k ? k : 1, 0);
  for (uint64_t i = 0; i < n; ++i) {
    if (assignments[i] >= k) return fail(VERS_ERR_INVALID, "vers_ivf_upload: assignment out of range");
    lens[assignments[i]] += 1;
  }
  std::unique_lock<std::shared_mutex> lk(h->index);
  h->flt_moved += 1;
  DeviceGuard g(h->device);
  if (int32_t rc = upload_begin_locked(h, centroids, k, c_stride_bytes, lens.data(), n)) return rc;
  if (int32_t rc = upload_chunk_host_locked(h, rows, row_stride_bytes, assignments, 0, n)) return rc;
  return upload_end_locked(h);
}

int32_t vers_ivf_upload_begin(vers_ivf_t* h, const float* centroids, uint64_t k, uint64_t c_stride_bytes, const uint64_t* list_lengths,
                              uint64_t n_total) {
  if (!h || (k && (!centroids || !list_lengths)) || (k && c_stride_bytes < (uint64_t)h->d * 4) || n_total > 0xFFFFFFFFull || k > 0xFFFFFFFFull ||
      (k == 0 && n_total != 0))
    return fail(VERS_ERR_INVALID, "vers_ivf_upload_begin: bad arguments");
  std::unique_lock<std::shared_mutex> lk(h->index);
  h->flt_moved += 1;
  DeviceGuard g(h->device);
  return upload_begin_locked(h, centroids, k, c_stride_bytes, list_lengths, n_total);
}

int32_t vers_ivf_upload_chunk(vers_ivf_t* h, const float* rows, uint64_t row_stride_bytes, const uint64_t* assignments, uint64_t first_vec_id,
                              uint64_t n) {
  if (!h || (n && (!rows || !assignments)) || row_stride_bytes < (uint64_t)(h ? h->d : 0) * 4)
    return fail(VERS_ERR_INVALID, "vers_ivf_upload_chunk: bad arguments");
  std::unique_lock<std::shared_mutex> lk(h->index);
  h->flt_moved += 1;
  DeviceGuard g(h->device);
  return upload_chunk_host_locked(h, rows, row_stride_bytes, assignments, first_vec_id, n);
}

int32_t vers_ivf_upload_chunk_dev(vers_ivf_t* h, const float* rows_dev, uint64_t ld_floats, const uint64_t* assignments_dev, uint64_t first_vec_id,
                                  uint64_t n) {
  if (!h || (n && (!rows_dev || !assignments_dev)) || ld_floats < (uint64_t)(h ? h->d : 0) || ld_floats % 4 || ld_floats > 0x3FFFFFFFull)
    return fail(VERS_ERR_INVALID, "vers_ivf_upload_chunk_dev: bad arguments (ld_floats must be >= d and a multiple of 4)");
  std::unique_lock<std::shared_mutex> lk(h->index);
  h->flt_moved += 1;
  DeviceGuard g(h->device);
  return upload_chunk_dev_locked(h, rows_dev, ld_floats, assignments_dev, first_vec_id, n);
}

int32_t vers_ivf_upload_end(vers_ivf_t* h) {
  if (!h) return fail(VERS_ERR_INVALID, "vers_ivf_upload_end: null handle");
  std::unique_lock<std::shared_mutex> lk(h->index);
  h->flt_moved += 1;
  DeviceGuard g(h->device);
  return upload_end_locked(h);
}

int32_t vers_ivf_upload_dev(vers_ivf_t* h, const float* rows_dev, uint64_t n, uint64_t ld_floats, const float* centroids_dev, uint64_t k,
                            uint64_t c_ld_floats, const uint64_t* assignments_dev) {
  if (!h || (n && (!rows_dev || !assignments_dev)) || (k && !centroids_dev) || ld_floats < (uint64_t)(h ? h->d : 0) || ld_floats % 4 ||
      ld_floats > 0x3FFFFFFFull || (k && c_ld_floats < (uint64_t)h->d) || n > 0xFFFFFFFFull || k > 0xFFFFFFFFull)
    return fail(VERS_ERR_INVALID, "vers_ivf_upload_dev: bad arguments (ld_floats must be >= d and a multiple of 4)");
  std::unique_lock<std::shared_mutex> lk(h->index);
  h->flt_moved += 1;
  DeviceGuard g(h->device);
  upload_abandon(h);
  DevBuf A, bad;
  if (int32_t rc = A.reserve((n ? n : 1) * 4)) return rc;
  if (int32_t rc = bad.reserve(16)) return rc;
  VERS_HIP_TRY(hipMemset(bad.p, 0, 16));
  if (n) {
    hipLaunchKernelGGL(u64_to_u32_checked_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, assignments_dev, n, k, A.as<uint32_t>(),
                       bad.as<uint32_t>());
    VERS_HIP_TRY(hipGetLastError());
  }
  uint32_t any_bad = 0;
  VERS_HIP_TRY(hipMemcpy(&any_bad, bad.p, 4, hipMemcpyDeviceToHost));
  if (any_bad) return fail(VERS_ERR_INVALID, "vers_ivf_upload_dev: assignment out of range");
  const size_t cbytes = ((size_t)k * h->ldx ? (size_t)k * h->ldx : 1) * sizeof(float);
  if (int32_t rc = h->centroids.reserve(cbytes)) return rc;
  if (k) {
    VERS_HIP_TRY(hipMemset(h->centroids.p, 0, cbytes));
    VERS_HIP_TRY(hipMemcpy2D(h->centroids.p, (size_t)h->ldx * 4, centroids_dev, (size_t)c_ld_floats * 4, (size_t)h->d * 4, k, hipMemcpyDeviceToDevice));
  }
  return install_index(h, rows_dev, (uint32_t)ld_floats, n, A.as<uint32_t>(), (uint32_t)k, nullptr);
}

int32_t vers_ivf_add(vers_ivf_t* h, const float* row, uint64_t* out_cluster, uint64_t* out_vec_id) {
  if (!h || !row) return fail(VERS_ERR_INVALID, "vers_ivf_add: bad arguments");
  std::unique_lock<std::shared_mutex> lk(h->index);
  AppendNote note(h);
  DeviceGuard g(h->device);
  VERS_HIP_TRY(hipDeviceSynchronize());  // searches still in flight on any stream read the rows and tables this call changes
  WsLease lease(h);
  if (lease.rc) return lease.rc;
  if (int32_t rc = lease.order_on(nullptr)) return rc;
  if (h->k == 0) return fail(VERS_ERR_EMPTY, "add on an index without centroids (reference: unwrap on None, ivfflat.rs:207)");
  HostStatusSlot slot(h);  // a NaN / spill status latched by an asynchronous _dev search stays there for vers_ivf_poll
  if (h->n_total >= 0xFFFFFFFEull) return fail(VERS_ERR_INVALID, "vec_id space exhausted");
  // (round 5: no allocation and three synchronisations fewer per call -- the row goes through the workspace's upload buffer instead of
  // a buffer allocated and freed per call, the ranked list and the status word come back in ONE copy, the three 4-byte table
  // updates are one small kernel instead of three synchronous copies: 196 -> ~100 us per vector at cfg3's geometry)
  const size_t back_off = ((size_t)h->d * sizeof(float) + 7) & ~(size_t)7;
  if (int32_t rc = W->io_q.reserve(back_off + 16)) return rc;
  VERS_HIP_TRY(hipMemcpyAsync(W->io_q.p, row, (size_t)h->d * sizeof(float), hipMemcpyHostToDevice, nullptr));
  const float* qp = nullptr;
  if (int32_t rc = stage_plain_queries(h, W->io_q.as<float>(), h->d, 1, &qp, nullptr)) return rc;
  if (int32_t rc = coarse(h, qp, 1, 1, nullptr)) return rc;  // first-minimum centroid (ivfflat.rs:201-207)
  uint64_t* const back = reinterpret_cast<uint64_t*>(W->io_q.as<char>() + back_off);  // [0] ranked list | [1] status word
  hipLaunchKernelGGL(add_fetch_kernel, dim3(1), dim3(1), 0, nullptr, (const uint64_t*)W->probe.p, W->st_word(), back);
  VERS_HIP_TRY(hipGetLastError());
  uint64_t got[2] = {0, 0};
  VERS_HIP_TRY(hipMemcpy(got, back, sizeof(got), hipMemcpyDeviceToHost));
  const uint64_t key = got[0];
  const uint32_t stw = (uint32_t)got[1];  // (add_fetch_kernel cleared the word)
  if ((stw & kStNaN) && h->k >= 2) return fail(VERS_ERR_NAN, "NaN distance in add (reference panics)");
  const uint32_t c = (uint32_t)key;
  const uint32_t vid = (uint32_t)h->n_total;  // the caller's vec_id is ignored, as in the reference (ivfflat.rs:209)
  const bool mine = h->h_owner[c] == h->rank;  // sharded: every rank picks the same list, only its owner stores the row
  uint32_t pos = 0;
  if (mine) {
    if (h->h_len[c] == h->h_cap[c])
      if (int32_t rc = relayout(h)) return rc;
    pos = h->h_off[c] + h->h_len[c];
    hipLaunchKernelGGL(scatter_row_kernel, dim3((h->ld / 4 + 63) / 64), dim3(64), 0, nullptr, qp, h->ld, (uint64_t)pos,
                       h->rows.as<float>());
    VERS_HIP_TRY(hipGetLastError());
  }
  h->h_len[c] += 1;
  hipLaunchKernelGGL(add_tables_kernel, dim3(1), dim3(1), 0, nullptr, mine ? h->row_ids.as<uint32_t>() + pos : (uint32_t*)nullptr, vid,
                     h->list_len.as<uint32_t>() + c, h->slot_len.as<uint32_t>() + h->h_slot[c], h->h_len[c]);
  VERS_HIP_TRY(hipGetLastError());
  if (mine)
    if (int32_t rc = refresh_norms(h, pos, (uint64_t)pos + 1, nullptr)) return rc;
  VERS_HIP_TRY(hipStreamSynchronize(nullptr));  // the index is consistent when the call returns (searches on any stream may follow)
  h->max_len = std::max(h->max_len, h->h_len[c]);
  h->n_total += 1;
  if (out_cluster) *out_cluster = c;
  if (out_vec_id) *out_vec_id = vid;
  return VERS_OK;
}

int32_t vers_ivf_add_batch(vers_ivf_t* h, const float* rows, uint64_t n, uint64_t row_stride_bytes, uint64_t* out_clusters, uint64_t* out_first_vec_id,
                           uint64_t* out_added) {
  if (!h || (n && !rows) || row_stride_bytes < (uint64_t)(h ? h->d : 0) * 4 || row_stride_bytes % 4)
    return fail(VERS_ERR_INVALID, "vers_ivf_add_batch: bad arguments (row_stride_bytes must be >= 4 d and a multiple of 4)");
  std::unique_lock<std::shared_mutex> lk(h->index);
  AppendNote note(h);
  DeviceGuard g(h->device);
  return add_batch_locked(h, rows, row_stride_bytes, nullptr, 0, n, out_clusters, nullptr, out_first_vec_id, out_added);
}

int32_t vers_ivf_add_batch_dev(vers_ivf_t* h, const float* rows_dev, uint64_t n, uint64_t ld_floats, uint64_t* out_clusters_dev, uint64_t* out_first_vec_id,
                               uint64_t* out_added) {
  if (!h || (n && !rows_dev) || ld_floats < (uint64_t)(h ? h->d : 0) || ld_floats % 4 || ld_floats > 0x3FFFFFFFull)
    return fail(VERS_ERR_INVALID, "vers_ivf_add_batch_dev: bad arguments (ld_floats must be >= d and a multiple of 4)");
  std::unique_lock<std::shared_mutex> lk(h->index);
  AppendNote note(h);
  DeviceGuard g(h->device);
  return add_batch_locked(h, nullptr, 0, rows_dev, ld_floats, n, nullptr, out_clusters_dev, out_first_vec_id, out_added);
}

int32_t vers_ivf_remove_batch(vers_ivf_t* h, const uint64_t* vec_ids, uint64_t n_ids, uint64_t* out_removed) {
  if (!h || (n_ids && !vec_ids)) return fail(VERS_ERR_INVALID, "vers_ivf_remove_batch: bad arguments");
  std::unique_lock<std::shared_mutex> lk(h->index);
  DeviceGuard g(h->device);
  uint64_t removed = 0;
  const int32_t rc = remove_batch_locked(h, vec_ids, nullptr, n_ids, nullptr, &removed);
  if (rc || removed) h->flt_moved += 1;  // (prepared filters: a removal compacts every touched list from its first removed row on)
  if (out_removed) *out_removed = removed;
  return rc;
}

int32_t vers_ivf_remove_batch_dev(vers_ivf_t* h, const uint64_t* vec_ids_dev, uint64_t n_ids, const vers_comm_t* comm, uint64_t* out_removed) {
  if (!h || (n_ids && !vec_ids_dev)) return fail(VERS_ERR_INVALID, "vers_ivf_remove_batch_dev: bad arguments");
  std::unique_lock<std::shared_mutex> lk(h->index);
  DeviceGuard g(h->device);
  uint64_t removed = 0;
  const int32_t rc = remove_batch_locked(h, nullptr, vec_ids_dev, n_ids, comm, &removed);
  if (rc || removed) h->flt_moved += 1;  // (prepared filters: a removal compacts every touched list from its first removed row on)
  if (out_removed) *out_removed = removed;
  return rc;
}

int32_t vers_ivf_update_batch(vers_ivf_t* h, const uint64_t* vec_ids, const float* rows, uint64_t n, uint64_t row_stride_bytes, uint64_t* out_clusters,
                              uint8_t* out_status, uint64_t* out_counts) {
  if (!h) return fail(VERS_ERR_INVALID, "vers_ivf_update_batch: null handle");
  if ((n && (!vec_ids || !rows)) || row_stride_bytes < (uint64_t)h->d * 4 || row_stride_bytes % 4)
    return fail(VERS_ERR_INVALID, "vers_ivf_update_batch: bad arguments (row_stride_bytes must be >= 4 d and a multiple of 4)");
  std::unique_lock<std::shared_mutex> lk(h->index);
  DeviceGuard g(h->device);
  return update_batch_locked(h, vec_ids, nullptr, rows, row_stride_bytes, nullptr, 0, n, false, out_clusters, out_status, out_counts);
}

int32_t vers_ivf_update_batch_dev(vers_ivf_t* h, const uint64_t* vec_ids_dev, const float* rows_dev, uint64_t n, uint64_t ld_floats, uint64_t* out_clusters_dev,
                                  uint8_t* out_status_dev, uint64_t* out_counts) {
  if (!h) return fail(VERS_ERR_INVALID, "vers_ivf_update_batch_dev: null handle");
  if ((n && (!vec_ids_dev || !rows_dev)) || ld_floats < (uint64_t)h->d || ld_floats % 4 || ld_floats > 0x3FFFFFFFull)
    return fail(VERS_ERR_INVALID, "vers_ivf_update_batch_dev: bad arguments (ld_floats must be >= d and a multiple of 4)");
  std::unique_lock<std::shared_mutex> lk(h->index);
  DeviceGuard g(h->device);
  return update_batch_locked(h, nullptr, vec_ids_dev, nullptr, 0, rows_dev, ld_floats, n, true, out_clusters_dev, out_status_dev, out_counts);
}

int32_t vers_ivf_update_batch_sharded_dev(vers_ivf_t* h, const vers_comm_t* comm, const uint64_t* vec_ids_dev, const float* rows_dev, uint64_t n, uint64_t ld_floats,
                                          uint64_t* out_clusters_dev, uint8_t* out_status_dev, uint64_t* out_counts) {
  const std::string who = "vers_ivf_update_batch_sharded_dev";
  if (!h) return fail(VERS_ERR_INVALID, who + ": null handle");
  if ((n && (!vec_ids_dev || !rows_dev)) || ld_floats < (uint64_t)h->d || ld_floats % 4 || ld_floats > 0x3FFFFFFFull || n > 0xFFFFFFFEull)
    return fail(VERS_ERR_INVALID, who + ": bad arguments (ld_floats must be >= d and a multiple of 4)");
  if (comm && (comm->world == 0 || comm->rank >= comm->world || comm->world > 255u || !comm->all_gather)) return fail(VERS_ERR_INVALID, who + ": incomplete vers_comm_t");
  std::unique_lock<std::shared_mutex> lk(h->index);
  const uint32_t world = comm ? comm->world : 1u;
  if (world != h->world || (comm && world > 1 && comm->rank != h->rank))
    return fail(VERS_ERR_INVALID, who + ": the handle is sharded as rank " + std::to_string(h->rank) + " of " + std::to_string(h->world) + ", the communicator says otherwise");
  DeviceGuard g(h->device);
  // comm == NULL on an unsharded handle: the existing call
  return update_batch_locked(h, nullptr, vec_ids_dev, nullptr, 0, rows_dev, ld_floats, n, true, out_clusters_dev, out_status_dev, out_counts, comm);
}

int32_t vers_update_phases(double* out, int32_t reset) {
  std::lock_guard<std::mutex> lk(g_ab_mu);
  if (out)
    for (int i = 0; i < kUpdatePhases; ++i) out[i] = g_up[i];
  if (reset)
    for (double& v : g_up) v = 0.0;
  return VERS_OK;
}

int32_t vers_ivf_live_count(vers_ivf_t* h, uint64_t* out_live) {
  if (!h || !out_live) return fail(VERS_ERR_INVALID, "vers_ivf_live_count: bad arguments");
  std::shared_lock<std::shared_mutex> lk(h->index);
  uint64_t live = 0;
  for (uint32_t c = 0; c < h->k; ++c) live += h->h_len[c];
  *out_live = live;
  return VERS_OK;
}

int32_t vers_ivf_compact(vers_ivf_t* h, uint64_t* out_rows_before, uint64_t* out_rows_after) {
  if (!h) return fail(VERS_ERR_INVALID, "vers_ivf_compact: null handle");
  std::unique_lock<std::shared_mutex> lk(h->index);
  h->flt_moved += 1;
  DeviceGuard g(h->device);
  return compact_locked(h, out_rows_before, out_rows_after);
}

int32_t vers_ivf_recluster(vers_ivf_t* h, uint64_t num_clusters, uint64_t num_attempts, uint64_t max_iterations, const uint64_t* init_indices,
                           float* out_centroids, uint64_t c_stride_bytes, uint64_t* out_assignments, float* out_cost, int32_t* out_kept,
                           uint64_t* out_iterations) {
  if (!h) return fail(VERS_ERR_INVALID, "vers_ivf_recluster: null handle");
  if (!out_kept || (num_attempts && num_clusters && !init_indices) || num_clusters > 0xFFFFFFFFull ||
      (num_clusters && num_attempts > 0xFFFFFFFFFFFFFFFFull / num_clusters) || (out_centroids && num_clusters && c_stride_bytes < (uint64_t)h->d * 4))
    return fail(VERS_ERR_INVALID, "vers_ivf_recluster: bad arguments (out_kept is not nullable; c_stride_bytes must be >= 4 d)");
  std::unique_lock<std::shared_mutex> lk(h->index);
  DeviceGuard g(h->device);
  return recluster_locked(h, num_clusters, num_attempts, max_iterations, init_indices, out_centroids, c_stride_bytes, out_assignments, out_cost, out_kept,
                          out_iterations);
}

int32_t vers_recluster_phases(double* out, int32_t reset) {
  std::lock_guard<std::mutex> lk(g_ab_mu);
  if (out)
    for (int i = 0; i < kReclusterPhases; ++i) out[i] = g_rc[i];
  if (reset)
    for (double& v : g_rc) v = 0.0;
  return VERS_OK;
}

int32_t vers_compact_phases(double* out, int32_t reset) {
  std::lock_guard<std::mutex> lk(g_ab_mu);
  if (out)
    for (int i = 0; i < kCompactPhases; ++i) out[i] = g_cp[i];
  if (reset)
    for (double& v : g_cp) v = 0.0;
  return VERS_OK;
}

int32_t vers_remove_phases(double* out, int32_t reset) {
  std::lock_guard<std::mutex> lk(g_ab_mu);
  if (out)
    for (int i = 0; i < kRemovePhases; ++i) out[i] = g_rm[i];
  if (reset)
    for (double& v : g_rm) v = 0.0;
  return VERS_OK;
}

int32_t vers_add_batch_phases(double* out, int32_t reset) {
  std::lock_guard<std::mutex> lk(g_ab_mu);
  if (out)
    for (int i = 0; i < kAddBatchPhases; ++i) out[i] = g_ab[i];
  if (reset)
    for (double& v : g_ab) v = 0.0;
  return VERS_OK;
}

}  // extern "C"
