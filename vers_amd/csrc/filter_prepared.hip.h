// filter_prepared.hip.h -- prepared filters: the masks of filter.hip.h / filter_multi.hip.h and the counts of filter_adaptive.hip.h kept in an
// object across calls (vers_ivf_filter_prepare), and the kernel that brings them up to date after an add that wrote its rows into list slack.
//
// A full build runs the existing mask and count kernels into the object's arrays.  What is new here is the TAIL REFRESH: after in-place
// appends the only rows whose bits can differ are the ones behind each grown list's old end (filter_prepared.hpp plans them on the host),
// so the cost follows the appended rows, not N.
//   filter_tail_refresh_kernel  one wave per grown list walks its tiles old_len / 64 .. (new_len - 1) / 64 and recomputes each tile WHOLE
//                               from row_ids and the bitmaps, with the mask kernels' predicate: the per-call form's word from one ballot,
//                               the per-query form's 64 row words and its tile word from a ballot per bitmap.  The change in popcount
//                               against the words that were there corrects allowed_len[f * k + L] (plain stores: a list is one wave's)
//                               and the object's allowed total (the wave's ONE atomic).
// The two forms of a one-bitmap object agree bit for bit, and an object of several bitmaps holds the per-query form only: one allowed_len
// and one total serve both.
#pragma once
#include "filter_multi.hip.h"
#include "filter_prepared.hpp"

namespace vers {

struct TailArgs {
  const TailItem* items;
  uint32_t n_items;
  const uint32_t* row_ids;   // [cap_rows]
  const uint32_t* list_off;  // [k_lists]
  uint64_t cap_rows;
  const uint64_t* bits;      // the object's bitmaps, `stride_words` apart
  uint64_t stride_words, n_bits;
  uint32_t n_filters;
  uint64_t* tile_mask;       // the per-call form, nullable (n_filters == 1 when held)
  uint64_t* row_sets;        // the per-query form, nullable together
  uint64_t* tile_sets;
  uint32_t* allowed_len;     // [n_filters][k_lists]
  uint32_t k_lists;
  unsigned long long* total;  // the object's allowed (bitmap, row) pairs
};

constexpr int kTailThreads = 256;  // four waves, an item each

static __global__ __launch_bounds__(kTailThreads) void filter_tail_refresh_kernel(TailArgs a) {
  const uint32_t i = blockIdx.x * (kTailThreads / kWave) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= a.n_items) return;  // (whole waves)
  const TailItem it = a.items[i];
  const uint64_t tile0 = (uint64_t)(a.list_off[it.list] >> 6);
  int32_t mine = 0;   // lane f: the change in bitmap f's rows of the list
  int32_t delta = 0;  // wave-uniform: the change over all bitmaps
  for (uint32_t t = tail_first_tile(it); t <= tail_last_tile(it); ++t) {
    const uint64_t T = tile0 + t;
    const uint64_t r = T * kWave + lane;
    if (T * kWave >= a.cap_rows) break;  // (a list never reaches past the storage: nothing is written there)
    const uint32_t id = r < a.cap_rows ? a.row_ids[r] : 0xFFFFFFFFu;
    const bool in = id != 0xFFFFFFFFu && (uint64_t)id < a.n_bits;
    const uint64_t* w = a.bits + (in ? (id >> 6) : 0u);
    if (a.row_sets != nullptr) {
      const uint64_t old_rs = r < a.cap_rows ? a.row_sets[r] : 0ull;
      uint64_t rs = 0ull, ts = 0ull;
      for (uint32_t f = 0; f < a.n_filters; ++f) {
        const bool ok = in && ((w[(uint64_t)f * a.stride_words] >> (id & 63)) & 1ull);
        if (ok) rs |= 1ull << f;
        const uint64_t now = __ballot(ok);
        if (now != 0ull) ts |= 1ull << f;
        const int32_t c = (int32_t)__popcll(now) - (int32_t)__popcll(__ballot((old_rs >> f) & 1ull));
        if (lane == (int)f) mine += c;
        delta += c;
      }
      a.row_sets[r] = rs;  // (row_sets covers whole tiles)
      if (lane == 0) a.tile_sets[T] = ts;
    }
    if (a.tile_mask != nullptr) {
      const bool ok = in && ((w[0] >> (id & 63)) & 1ull);
      const uint64_t now = __ballot(ok);
      if (a.row_sets == nullptr) {
        const int32_t c = (int32_t)__popcll(now) - (int32_t)__popcll(a.tile_mask[T]);
        if (lane == 0) mine += c;
        delta += c;
      }
      if (lane == 0) a.tile_mask[T] = now;
    }
  }
  if ((uint32_t)lane < a.n_filters && mine != 0) {
    uint32_t* const p = a.allowed_len + (uint64_t)lane * a.k_lists + it.list;
    *p = (uint32_t)((int32_t)*p + mine);
  }
  if (lane == 0 && delta != 0) atomicAdd(a.total, (unsigned long long)(long long)delta);
}

}  // namespace vers
