// vers_amd/csrc/shard_where.hpp with the host compiler alone: the decisions of the "where" round of the sharded fetch / update / search by id
// -- the agreement, the claimer per request and its errors, the row round's per-chunk counts, pad, callbacks and slots -- against a plain
// restatement, at chunk sizes 1, 64 and n, with repeats, an all-empty chunk and a rank that owns nothing.
#include <cstdio>
#include <vector>

#include "shard_where.hpp"

using namespace vers::shw;

static int bad = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); ++bad; } } while (0)

struct Table {
  uint32_t world;
  uint64_t n;
  std::vector<uint32_t> w;
  Table(uint32_t world_, uint64_t n_) : world(world_), n(n_), w((size_t)world_ * (n_ + 1), kNoWord) {
    for (uint32_t r = 0; r < world; ++r) at(r, n) = 0;
  }
  uint32_t& at(uint32_t r, uint64_t i) { return w[(size_t)r * (n + 1) + i]; }
};

// the plan restated request by request
static void check_plan(const std::vector<uint32_t>& claimer, uint32_t world, uint64_t R) {
  const uint64_t n = claimer.size(), chunks = where_chunks(n, R);
  std::vector<uint32_t> counts, pad, slot;
  const uint64_t calls = where_plan_rows(claimer.data(), n, world, R, counts, pad, slot);
  CHECK(counts.size() == chunks * world && pad.size() == chunks && slot.size() == n);
  uint64_t want_calls = 1;
  for (uint64_t j = 0; j < chunks; ++j) {
    uint32_t mx = 0;
    for (uint32_t r = 0; r < world; ++r) {
      uint32_t c = 0;
      for (uint64_t i = j * R; i < n && i < (j + 1) * R; ++i) c += claimer[i] == r;
      CHECK(counts[j * world + r] == c);
      mx = c > mx ? c : mx;
    }
    CHECK(pad[j] == mx);
    want_calls += mx != 0;
  }
  CHECK(calls == want_calls);
  for (uint64_t i = 0; i < n; ++i) {
    if (claimer[i] == kNoWord) { CHECK(slot[i] == kNoWord); continue; }
    uint32_t before = 0;  // the claimer's found requests of the chunk in front of i
    for (uint64_t t = (i / R) * R; t < i; ++t) before += claimer[t] == claimer[i];
    CHECK(slot[i] == claimer[i] * pad[i / R] + before);
    CHECK(slot[i] < world * pad[i / R]);  // inside the gathered chunk
  }
  for (uint32_t me = 0; me < world; ++me) {
    std::vector<uint32_t> req;
    std::vector<uint64_t> begin;
    where_my_requests(claimer.data(), n, me, R, req, begin);
    CHECK(begin.size() == chunks + 1 && begin[0] == 0 && begin[chunks] == req.size());
    for (uint64_t j = 0; j < chunks; ++j) {
      CHECK(begin[j + 1] - begin[j] == counts[j * world + me]);
      for (uint64_t p = begin[j]; p < begin[j + 1]; ++p) {
        CHECK(claimer[req[p]] == me && req[p] / R == j);
        CHECK(slot[req[p]] == me * pad[j] + (p - begin[j]));  // what it packs at place p is what the placing kernel reads there
        if (p > begin[j]) CHECK(req[p - 1] < req[p]);         // request order
      }
    }
  }
}

int main() {
  // 5 lists dealt to 3 ranks; rank 2 owns nothing
  const uint32_t k = 5, world = 3;
  const uint8_t owner[k] = {0, 1, 0, 1, 1};
  {
    // requests: 0 -> list 2 (rank 0), 1 -> nobody, 2 -> list 4 (rank 1), 3 -> list 0 (rank 0), 4 = request 0's id again (a repeat), 5 -> list 1 (rank 1)
    Table t(world, 6);
    t.at(0, 0) = 2; t.at(1, 2) = 4; t.at(0, 3) = 0; t.at(0, 4) = 2; t.at(1, 5) = 1;
    uint32_t who = 77;
    CHECK(where_first_failure(t.w.data(), world, 6, &who) == 0 && who == 77);
    std::vector<uint32_t> claimer(6), cluster(6);
    CHECK(where_resolve(t.w.data(), world, 6, owner, k, claimer.data(), cluster.data()) == kWhereOk);
    const uint32_t want_who[6] = {0, kNoWord, 1, 0, 0, 1}, want_c[6] = {2, kNoWord, 4, 0, 2, 1};
    for (int i = 0; i < 6; ++i) CHECK(claimer[i] == want_who[i] && cluster[i] == want_c[i]);
    // the agreement: the FIRST failing rank's status, in rank order
    t.at(2, 6) = 4; t.at(1, 6) = 5;
    CHECK(where_first_failure(t.w.data(), world, 6, &who) == 5 && who == 1);
    t.at(1, 6) = 0;
    CHECK(where_first_failure(t.w.data(), world, 6, &who) == 4 && who == 2);
    t.at(2, 6) = 0;
    // a double claim
    Table dbl = t;
    dbl.at(1, 3) = 1;
    CHECK(where_resolve(dbl.w.data(), world, 6, owner, k, claimer.data(), cluster.data()) == kWhereDoubleClaim);
    // a claim by a rank that does not own the claimed list
    Table not_owner = t;
    not_owner.at(0, 0) = kNoWord; not_owner.at(0, 4) = kNoWord; not_owner.at(2, 0) = 2;
    CHECK(where_resolve(not_owner.w.data(), world, 6, owner, k, claimer.data(), cluster.data()) == kWhereNotOwner);
    // a cluster that does not exist
    Table big = t;
    big.at(1, 1) = k;
    CHECK(where_resolve(big.w.data(), world, 6, owner, k, claimer.data(), cluster.data()) == kWhereBadCluster);
    // n = 0: one callback, nothing else
    std::vector<uint32_t> counts, pad, slot;
    CHECK(where_plan_rows(nullptr, 0, world, 64, counts, pad, slot) == 1 && pad.empty() && slot.empty());
  }
  {
    // 200 requests: ids of ranks 0 / 1 mixed, requests 64 .. 127 found by nobody (an all-empty chunk at R = 64), repeats throughout
    std::vector<uint32_t> claimer(200);
    for (uint32_t i = 0; i < 200; ++i) claimer[i] = (i >= 64 && i < 128) ? kNoWord : (i % 7 == 3 ? kNoWord : (i * 2654435761u >> 13) % 2u);
    for (uint64_t R : {(uint64_t)1, (uint64_t)64, (uint64_t)200, (uint64_t)131072}) check_plan(claimer, world, R);
    std::vector<uint32_t> counts, pad, slot;
    const uint64_t calls = where_plan_rows(claimer.data(), 200, world, 64, counts, pad, slot);
    CHECK(pad.size() == 4 && pad[1] == 0 && pad[0] != 0 && pad[2] != 0 && pad[3] != 0 && calls == 1 + 3);  // the empty chunk is skipped
    uint64_t found = 0;
    for (uint32_t c : claimer) found += c != kNoWord;
    CHECK(where_plan_rows(claimer.data(), 200, world, 1, counts, pad, slot) == 1 + found);  // R = 1: a callback per found request
    CHECK(where_plan_rows(claimer.data(), 200, world, 200, counts, pad, slot) == 2);
    CHECK(where_chunk_bytes(pad[0], 40) == (uint64_t)pad[0] * 160);
    // everything on one rank, everything nowhere
    std::vector<uint32_t> one(130, 1u), none(130, kNoWord);
    check_plan(one, world, 64);
    check_plan(none, world, 64);
    CHECK(where_plan_rows(none.data(), 130, world, 64, counts, pad, slot) == 1);
  }
  printf(bad ? "FAILED\n" : "all ok\n");
  return bad ? 1 : 0;
}
