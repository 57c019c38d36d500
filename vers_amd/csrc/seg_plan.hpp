// seg_plan.hpp -- the host-side geometry of the scan engine: its constants, the residency and the grid of a scan launch, and the segment
// plan of the exhaustive scans.  No HIP dependency: the host compiler alone builds it (tests/cpp/seg_plan_demo.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace vers {

// ---- geometry of the scan engine (scan.hip.h) ---------------------------------
constexpr int kWave = 64;        // CDNA4 wavefront
constexpr int kChunk = 32;       // f32 columns consumed per step
constexpr int kLoads = kChunk / 4;  // float4 loads per lane per step (1 KiB per wave each)
constexpr int kColAlign = 2 * kChunk;  // blocked matrices / padded queries: columns padded to this
constexpr int kWavesPerBlock = 4;
constexpr int kMaxTopK = 64;     // one sorted key per lane

inline uint32_t round_up(uint32_t x, uint32_t m) { return (x + m - 1) / m * m; }
inline uint64_t round_up64(uint64_t x, uint64_t m) { return (x + m - 1) / m * m; }
// a work item is addressed through one 32-bit buffer descriptor: keep it under 2 GiB
inline uint64_t max_seg_rows(uint32_t ld) { return ((1ull << 31) / ((uint64_t)ld * 4)) / 64 * 64; }

// dynamic LDS of a batched scan launch (one interleaved query block) and the resident blocks per CU it allows
inline size_t scan_lds_bytes(int QG, uint32_t ld) { return QG == 1 ? 0 : (size_t)ld * QG * sizeof(float) + 16; }
inline uint32_t scan_blocks_per_cu(int QG, uint32_t ld) {
  if (QG == 1) return 3;                                   // 12 waves/CU at <= 168 VGPRs
  const size_t b = scan_lds_bytes(QG, ld);
  const uint32_t by_lds = (uint32_t)((160u * 1024u) / (b ? b : 1));
  const uint32_t by_vgpr = 2;                              // two tiles per step: <= 256 VGPRs, 8 waves/CU
  return by_lds < 1 ? 1 : (by_lds > by_vgpr ? by_vgpr : by_lds);
}
// blocks of a scan launch over `items` work items (a wave each): no more than stay resident, nor than `cap` (the filtered scans: a counter
// slot per launched wave), at least one
inline uint32_t scan_grid(int n_cu, int QG, uint32_t ld, uint32_t items, uint32_t cap = 0xFFFFFFFFu) {
  const uint32_t blocks = (items + kWavesPerBlock - 1) / kWavesPerBlock;
  return std::max<uint32_t>(1u, std::min(std::min(blocks, (uint32_t)n_cu * scan_blocks_per_cu(QG, ld)), cap));
}

// ---- segments of an exhaustive scan ----------------------------------------------
// item = (row segment, query group): one query alone, else groups of eight; one item per resident wave when possible (static balance), at
// least one 64-row tile each, or segments of `fixed_seg_rows` rows (> 0: option "seg_rows") -- never longer than a buffer descriptor
// reaches.  QG > 1: the segments of a group are padded to quads with empty items (quads share a query block).
struct SegPlan {
  uint32_t seg_rows, n_segs, n_segs_pad, n_items, n_qg;
  int QG;
  bool too_large;  // the (query, segment) slots or the items do not fit 32 bits (n_items has wrapped): what the callers with a slot count refuse
};
inline SegPlan seg_plan(uint64_t n_rows, uint32_t b, uint32_t ld, int n_cu, int64_t fixed_seg_rows) {
  SegPlan s;
  s.QG = b == 1 ? 1 : 8;
  s.n_qg = (b + s.QG - 1) / s.QG;
  const uint32_t target_items = (uint32_t)n_cu * scan_blocks_per_cu(s.QG, ld) * kWavesPerBlock;
  const uint64_t per = (n_rows * s.n_qg + target_items - 1) / target_items;
  s.seg_rows = (uint32_t)std::min<uint64_t>(round_up64(fixed_seg_rows > 0 ? (uint64_t)fixed_seg_rows : (per ? per : 1), kWave), max_seg_rows(ld));
  s.n_segs = (uint32_t)((n_rows + s.seg_rows - 1) / s.seg_rows);
  if (s.n_segs == 0) s.n_segs = 1;
  s.n_segs_pad = s.QG == 1 ? s.n_segs : round_up(s.n_segs, 4);
  s.n_items = s.n_segs_pad * s.n_qg;
  s.too_large = (uint64_t)b * s.n_segs >= 0xFFFFFFFFull || (uint64_t)s.n_segs_pad * s.n_qg >= 0xFFFFFFFFull;
  return s;
}

}  // namespace vers
