// Drives filter_tail_plan (vers_amd/csrc/filter_prepared.hpp: the host part of a prepared filter's tail refresh) under the host compiler.
// stdin, per case: k rank owned_flag first_new_id n_bits, then k lines "snap_len len owner".  stdout, per case: "n_items rows ok", then per
// item "list old_len new_len first_tile last_tile".  ok = the plan equals a brute-force restatement: row by row, which rows of which owned
// list are new, and which 64-row tiles hold one -- or nothing at all when no id handed out since the snapshot is below n_bits.
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "filter_prepared.hpp"

int main() {
  unsigned k, rank, owned;
  unsigned long long first_new_id, n_bits;
  while (std::scanf("%u %u %u %llu %llu", &k, &rank, &owned, &first_new_id, &n_bits) == 5) {
    std::vector<uint32_t> snap(k), len(k);
    std::vector<uint8_t> owner(k);
    for (unsigned L = 0; L < k; ++L) {
      unsigned a, b, o;
      if (std::scanf("%u %u %u", &a, &b, &o) != 3) return 2;
      snap[L] = a; len[L] = b; owner[L] = (uint8_t)o;
    }
    std::vector<vers::TailItem> items;
    const uint64_t rows = vers::filter_tail_plan(snap.data(), len.data(), owned ? owner.data() : nullptr, rank, k, first_new_id, n_bits, items);
    // brute force: every new row of every list this rank stores, and the tile it sits in
    std::set<std::pair<uint32_t, uint32_t>> want_tiles, got_tiles;
    uint64_t want_rows = 0;
    if (first_new_id < n_bits)
      for (unsigned L = 0; L < k; ++L) {
        if (owned && owner[L] != rank) continue;
        for (uint32_t r = snap[L]; r < len[L]; ++r) {
          want_tiles.insert({L, r / 64u});
          want_rows += 1;
        }
      }
    bool ok = rows == want_rows;
    uint32_t last_list = 0;
    for (size_t i = 0; i < items.size(); ++i) {
      const vers::TailItem& it = items[i];
      ok = ok && it.list < k && it.old_len < it.new_len && it.old_len == snap[it.list] && it.new_len == len[it.list];
      ok = ok && (i == 0 || it.list > last_list);  // one item per list, in list order: a list is one wave's
      last_list = it.list;
      if (!ok) break;
      for (uint32_t t = vers::tail_first_tile(it); t <= vers::tail_last_tile(it); ++t) got_tiles.insert({it.list, t});
    }
    ok = ok && got_tiles == want_tiles;
    std::printf("%zu %llu %d\n", items.size(), (unsigned long long)rows, ok ? 1 : 0);
    for (const vers::TailItem& it : items) std::printf("%u %u %u %u %u\n", it.list, it.old_len, it.new_len, vers::tail_first_tile(it), vers::tail_last_tile(it));
  }
  return 0;
}
