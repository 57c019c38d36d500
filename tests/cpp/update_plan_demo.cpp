// update_plan_demo.cpp -- vers_amd/csrc/update_plan.hpp under the host compiler: the locate classification and the in-place BACKWARD merge of
// vers_ivf_update_batch emulated on std::vectors, tile by tile in descending order with the kernel's own index functions (every load of a
// tile before its stores, as update_merge_kernel), against the plain restatement `retain` + sorted `insert` of include/vers_hip.h.
// Prints "OK <cases>" or the first difference.  (tests/test_update_plan_host.py builds it with -fsanitize=address,undefined.)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "update_plan.hpp"

using namespace vers;

struct List {
  uint32_t cap = 0, len = 0;
  std::vector<uint32_t> ids;    // [cap], upd::kNone behind len
  std::vector<uint64_t> rows;   // [cap] the row's payload
};
struct Update {
  uint32_t id, list;  // the new list (its first-minimum centroid)
};

static uint64_t old_payload(uint32_t id) { return (uint64_t)id * 2u + 1u; }
static uint64_t new_payload(uint32_t id) { return ((uint64_t)1 << 40) + id; }
static uint32_t round_up64(uint32_t x) { return (x + 63u) / 64u * 64u; }

static std::vector<List> make_lists(const std::vector<std::vector<uint32_t>>& ids, const std::vector<uint32_t>& caps) {
  std::vector<List> ls(ids.size());
  for (size_t c = 0; c < ids.size(); ++c) {
    ls[c].len = (uint32_t)ids[c].size();
    ls[c].cap = std::max(caps[c], round_up64(ls[c].len));
    ls[c].ids.assign(ls[c].cap, upd::kNone);
    ls[c].rows.assign(ls[c].cap, 0);
    for (uint32_t i = 0; i < ls[c].len; ++i) { ls[c].ids[i] = ids[c][i]; ls[c].rows[i] = old_payload(ids[c][i]); }
  }
  return ls;
}

// the restatement: per update, values[v] = x; if the cluster changes, retain + insert at the partition point
static void restate(std::vector<std::vector<uint32_t>>& ids, std::vector<uint64_t>& values, const std::vector<Update>& ups, std::vector<uint8_t>& status) {
  status.assign(ups.size(), upd::kSkipped);
  for (size_t i = 0; i < ups.size(); ++i) {
    const uint32_t v = ups[i].id;
    size_t cur = ids.size();
    for (size_t c = 0; c < ids.size(); ++c)
      if (std::binary_search(ids[c].begin(), ids[c].end(), v)) cur = c;
    if (cur == ids.size()) continue;
    values[v] = new_payload(v);
    if (cur == ups[i].list) { status[i] = upd::kStayed; continue; }
    status[i] = upd::kMoved;
    ids[cur].erase(std::find(ids[cur].begin(), ids[cur].end(), v));
    auto& l = ids[ups[i].list];
    l.insert(std::partition_point(l.begin(), l.end(), [&](uint32_t y) { return y < v; }), v);
  }
}

static int g_cases = 0;

static bool run_case(const char* name, const std::vector<std::vector<uint32_t>>& ids0, const std::vector<uint32_t>& caps, const std::vector<Update>& ups,
                     int expect_grow = -1) {
  ++g_cases;
  const uint32_t k = (uint32_t)ids0.size();
  uint32_t max_id = 0;
  for (auto& l : ids0) for (uint32_t v : l) max_id = std::max(max_id, v);
  for (auto& u : ups) max_id = std::max(max_id, u.id);
  // ---- restatement
  std::vector<std::vector<uint32_t>> want = ids0;
  std::vector<uint64_t> values(max_id + 1u);
  for (uint32_t v = 0; v <= max_id; ++v) values[v] = old_payload(v);
  std::vector<uint8_t> want_status;
  restate(want, values, ups, want_status);
  // ---- emulation of the device sequence
  std::vector<List> ls = make_lists(ids0, caps);
  std::vector<uint32_t> list_off(k), slot(max_id + 1u, upd::kNone);
  uint32_t total = 0;
  for (uint32_t c = 0; c < k; ++c) { list_off[c] = total; total += ls[c].cap; }
  for (size_t i = 0; i < ups.size(); ++i) slot[ups[i].id] = (uint32_t)i;
  // locate: one pass over the storage rows
  std::vector<uint8_t> status(ups.size(), upd::kSkipped);
  std::vector<uint32_t> out_cnt(k, 0), in_cnt(k, 0), first_tile(k, upd::kNone), len(k), cap(k);
  std::vector<std::vector<uint32_t>> incoming(k);
  std::vector<bool> leaves(max_id + 1u, false);
  for (uint64_t r = 0; r < total; ++r) {
    const uint32_t c = upd::list_of_row(list_off.data(), k, r), p = (uint32_t)(r - list_off[c]);
    if (ls[c].cap == 0) continue;  // (no storage: the offset belongs to the next list, list_of_row never returns c)
    const uint32_t id = ls[c].ids[p];
    if (id == upd::kNone || slot[id] == upd::kNone) continue;
    const uint32_t i = slot[id];
    status[i] = upd::classify(c, ups[i].list);
    if (status[i] == upd::kStayed) { ls[c].rows[p] = new_payload(id); continue; }  // overwrite in place
    leaves[id] = true;
    out_cnt[c] += 1;
    first_tile[c] = std::min(first_tile[c], p >> 6);
    in_cnt[ups[i].list] += 1;
    incoming[ups[i].list].push_back(id);
  }
  if (status != want_status) { std::printf("%s: status differs\n", name); return false; }
  for (uint32_t c = 0; c < k; ++c) { len[c] = ls[c].len; cap[c] = ls[c].cap; }
  std::vector<uint32_t> mid(k), fin(k);
  const bool grow = upd::plan_lengths(len.data(), out_cnt.data(), in_cnt.data(), cap.data(), k, mid.data(), fin.data());
  bool want_grow = false;
  for (uint32_t c = 0; c < k; ++c) want_grow = want_grow || want[c].size() > ls[c].cap;
  if (grow != want_grow || (expect_grow >= 0 && grow != (expect_grow != 0))) { std::printf("%s: grow flag %d\n", name, (int)grow); return false; }
  if (grow)  // the one re-layout: room for the final lengths, whole tiles
    for (uint32_t c = 0; c < k; ++c) {
      ls[c].cap = std::max(ls[c].cap, round_up64(fin[c] + std::max(64u, fin[c] / 8u)));
      ls[c].ids.resize(ls[c].cap, upd::kNone);
      ls[c].rows.resize(ls[c].cap, 0);
    }
  // movers out (remove_compact_kernel's result: survivors keep their order, slack behind them); tiles in front of first_tile untouched
  for (uint32_t c = 0; c < k; ++c) {
    if (!out_cnt[c]) continue;
    uint32_t w = first_tile[c] * 64u;
    for (uint32_t s = 0; s < w; ++s)
      if (leaves[ls[c].ids[s]]) { std::printf("%s: a leaving row in front of the first tile\n", name); return false; }
    for (uint32_t s = w; s < ls[c].len; ++s)
      if (!leaves[ls[c].ids[s]]) { ls[c].ids[w] = ls[c].ids[s]; ls[c].rows[w] = ls[c].rows[s]; ++w; }
    for (uint32_t s = w; s < round_up64(ls[c].len); ++s) { ls[c].ids[s] = upd::kNone; ls[c].rows[s] = 0; }
    if (w != mid[c]) { std::printf("%s: length in between\n", name); return false; }
    ls[c].len = w;
  }
  // movers in: the backward merge, destination tiles in descending order, all loads of a tile before its stores
  for (uint32_t c = 0; c < k; ++c) {
    const uint32_t n_in = in_cnt[c];
    if (!n_in) continue;
    std::vector<uint32_t>& nv = incoming[c];
    std::sort(nv.begin(), nv.end());
    std::vector<uint32_t> pos(n_in);
    for (uint32_t t = 0; t < n_in; ++t) pos[t] = upd::insertion_point(ls[c].ids.data(), ls[c].len, nv[t]);
    List& l = ls[c];
    const std::vector<uint32_t> before_ids = l.ids;
    const uint32_t t_first = upd::merge_first_tile(pos.data()), t_last = upd::merge_last_tile(l.len, n_in);
    if ((uint64_t)(t_last + 1u) * 64u > l.cap) { std::printf("%s: the merge leaves the list's capacity\n", name); return false; }
    // the closed forms agree with each other: every old and every new row has one destination, and merge_source inverts them
    for (uint32_t t = 0; t < n_in; ++t)
      if (upd::merge_source(pos.data(), n_in, l.len, upd::new_row_dest(pos.data(), t)) != (upd::kNewBit | t)) { std::printf("%s: new_row_dest\n", name); return false; }
    for (uint32_t s = 0; s < l.len; ++s) {
      const uint32_t dst = upd::old_row_dest(pos.data(), n_in, s);
      if (dst < s || upd::merge_source(pos.data(), n_in, l.len, dst) != s) { std::printf("%s: old_row_dest\n", name); return false; }
      if (s < t_first * 64u && dst != s) { std::printf("%s: a row in front of the first tile moves\n", name); return false; }
    }
    for (uint32_t T = t_last + 1u; T-- > t_first;) {
      uint32_t src[64], id[64];
      uint64_t row[64];
      for (uint32_t r = 0; r < 64u; ++r) {  // loads
        src[r] = upd::merge_source(pos.data(), n_in, l.len, T * 64u + r);
        id[r] = upd::kNone;
        row[r] = 0;
        if (src[r] == upd::kNone) continue;
        if (src[r] & upd::kNewBit) { id[r] = nv[src[r] & ~upd::kNewBit]; row[r] = new_payload(id[r]); }
        else {
          if (src[r] > T * 64u + r) { std::printf("%s: a source behind its destination\n", name); return false; }
          id[r] = l.ids[src[r]];
          row[r] = l.rows[src[r]];
          if (id[r] != before_ids[src[r]]) { std::printf("%s: a source was overwritten before it was read\n", name); return false; }
        }
      }
      for (uint32_t r = 0; r < 64u; ++r) { l.ids[T * 64u + r] = id[r]; l.rows[T * 64u + r] = row[r]; }  // stores
    }
    l.len += n_in;
    if (l.len != fin[c]) { std::printf("%s: final length\n", name); return false; }
  }
  // ---- comparison: ids, payloads, slack
  for (uint32_t c = 0; c < k; ++c) {
    if (ls[c].len != want[c].size()) { std::printf("%s: list %u holds %u rows, want %zu\n", name, c, ls[c].len, want[c].size()); return false; }
    for (uint32_t i = 0; i < ls[c].len; ++i)
      if (ls[c].ids[i] != want[c][i] || ls[c].rows[i] != values[want[c][i]]) { std::printf("%s: list %u row %u\n", name, c, i); return false; }
    for (uint32_t i = ls[c].len; i < ls[c].cap; ++i)
      if (ls[c].ids[i] != upd::kNone) { std::printf("%s: list %u slack row %u holds an id\n", name, c, i); return false; }
  }
  return true;
}

static std::vector<uint32_t> spaced(uint32_t n, uint32_t first, uint32_t step) {
  std::vector<uint32_t> v(n);
  for (uint32_t i = 0; i < n; ++i) v[i] = first + i * step;
  return v;
}

int main() {
  bool ok = true;
  const uint32_t sizes[] = {0, 1, 63, 64, 65, 130, 200};
  // list 0: the target, ids 10, 20, ...; list 1: the donors, ids == 5 (mod 10) so that each lands between two of the target's
  for (uint32_t L : sizes) {
    const std::vector<uint32_t> target = spaced(L, 10, 10);
    std::vector<uint32_t> donors;
    for (uint32_t i = 0; i <= L + 80u; ++i) donors.push_back(5 + 10 * i);
    const std::vector<std::vector<uint32_t>> ids = {target, donors, spaced(3, 100000, 1)};
    const std::vector<uint32_t> caps = {round_up64(L) + 128u, 0, 64};
    auto mv = [&](std::vector<uint32_t> pick) {
      std::vector<Update> u;  // (the same id twice is refused by the call: picks that coincide on a short list count once)
      for (size_t j = 0; j < pick.size(); ++j)
        if (std::find(pick.begin(), pick.begin() + j, pick[j]) == pick.begin() + j) u.push_back(Update{5 + 10 * pick[j], 0});
      return u;
    };
    ok = ok && run_case("head", ids, caps, mv({0}));
    ok = ok && run_case("tail", ids, caps, mv({L}));
    ok = ok && run_case("middle", ids, caps, mv({L / 2}));
    ok = ok && run_case("head+middle+tail", ids, caps, mv({L, 0, L / 2, L + 3}));
    if (L >= 64) ok = ok && run_case("on a tile boundary", ids, caps, mv({64}));
    if (L >= 130) ok = ok && run_case("on both tile boundaries", ids, caps, mv({128, 64}));
    {
      std::vector<uint32_t> many;  // more than 64 rows into one list, interleaved with its own and past its end
      for (uint32_t i = 0; i < 70; ++i) many.push_back((i * 7u) % (L + 80u));
      std::sort(many.begin(), many.end());
      many.erase(std::unique(many.begin(), many.end()), many.end());
      while (many.size() < 70) many.push_back(L + 10u + (uint32_t)many.size());
      std::sort(many.begin(), many.end());
      many.erase(std::unique(many.begin(), many.end()), many.end());
      ok = ok && run_case("more than 64 rows", ids, caps, mv(many));
    }
    {
      // the list both loses and gains rows; a stay among them; an id that is in no list
      std::vector<Update> u = mv({0, L / 3, L});
      for (uint32_t i = 0; i < L; i += 3) u.push_back(Update{target[i], 1});
      if (L > 1) u.push_back(Update{target[1], 0});
      u.push_back(Update{7, 0});
      ok = ok && run_case("loses and gains", ids, caps, u);
    }
    {
      std::vector<Update> u;  // every row leaves the list (into a list with slack), two enter it
      for (uint32_t v : target) u.push_back(Update{v, 2});
      ok = ok && run_case("every row leaves", ids, {round_up64(L) + 128u, 0, round_up64(L + 3) + 64u}, u);
      u.push_back(Update{5, 0});
      if (L) u.push_back(Update{10 * L + 5, 0});
      ok = ok && run_case("every row leaves, two enter", ids, {round_up64(L) + 128u, 0, round_up64(L + 3) + 64u}, u);
    }
    {
      // exactly at capacity: the last free row is taken (no growth), one more does not fit (the grow flag)
      const uint32_t capL = round_up64(L + 1);
      std::vector<uint32_t> fill;
      for (uint32_t i = 0; i < capL - L; ++i) fill.push_back(i);
      ok = ok && run_case("fills its capacity", ids, {capL, 0, 64}, mv(fill), 0);
      fill.push_back(capL - L);
      ok = ok && run_case("outgrows its capacity", ids, {capL, 0, 64}, mv(fill), 1);
    }
  }
  // rows entering an empty list that has no storage yet (capacity 0): growth
  ok = ok && run_case("empty list without storage", {{}, spaced(10, 1, 1)}, {0, 64}, {Update{3, 0}, Update{9, 0}}, 1);
  // random cases from a fixed seed
  std::mt19937 rng(0x19D);
  for (int it = 0; it < 400 && ok; ++it) {
    const uint32_t k = 1 + rng() % 5, n = rng() % 600;
    std::vector<std::vector<uint32_t>> ids(k);
    std::vector<uint32_t> all;
    for (uint32_t v = 0; v < n; ++v)
      if (rng() % 8) { ids[rng() % k].push_back(v); all.push_back(v); }  // (one id in eight is in no list)
    std::vector<uint32_t> caps(k);
    for (uint32_t c = 0; c < k; ++c) caps[c] = round_up64((uint32_t)ids[c].size()) + 64u * (rng() % 3);
    std::vector<uint32_t> picks(n);
    for (uint32_t v = 0; v < n; ++v) picks[v] = v;
    std::shuffle(picks.begin(), picks.end(), rng);
    picks.resize(n ? rng() % n : 0);
    std::vector<Update> u;
    const uint32_t hot = rng() % k;
    for (uint32_t v : picks) u.push_back(Update{v, rng() % 3 ? hot : (uint32_t)(rng() % k)});
    ok = ok && run_case("random", ids, caps, u);
  }
  if (!ok) return 1;
  std::printf("OK %d\n", g_cases);
  return 0;
}
