// shard_where.hpp -- the host decisions of the "where" round that vers_ivf_fetch_sharded_dev and vers_ivf_search_by_id_sharded_dev share
// (ivf_fetch.hip; a sharded update would share it too), without HIP types.
//
// On a handle sharded by cluster, whether a vec id is live, and in which list, is known to the list's owner alone.  ONE all-gather of
// n + 1 u32 words per rank tells every rank:
//   word i (i < n)  the cluster (< k) of vec_ids[i] if THIS rank stores it in a list, else kNoWord
//   word n          the rank's local status: 0, or the VERS_ERR_* of a local failure (the agreement: a non-zero word is every rank's verdict)
// From the gathered table [world][n + 1] every rank derives the same claimer (owning rank) and cluster per request, and for the row round of
// a fetch -- chunks of R requests, one all-gather per chunk in which any rank found something, every rank's found rows packed in request
// order and padded to the largest rank's count -- the per-chunk counts, the pad, the callbacks and each request's slot in the gathered chunk.
#pragma once
#include <cstdint>
#include <vector>

namespace vers {
namespace shw {

constexpr uint32_t kNoWord = 0xFFFFFFFFu;  // the id is in no list of this rank | a request nobody claimed | a request without a slot

// what where_resolve found wrong with a table whose status words are all zero (the callers answer VERS_ERR_HIP: inconsistent index)
enum WhereError : int { kWhereOk = 0, kWhereDoubleClaim = 1, kWhereNotOwner = 2, kWhereBadCluster = 3 };

inline const uint32_t* where_row(const uint32_t* table, uint64_t n, uint32_t r) { return table + (size_t)r * (n + 1); }

// The agreement: the first rank (in rank order) whose status word is non-zero, and that word; 0 when every rank is fine.
inline uint32_t where_first_failure(const uint32_t* table, uint32_t world, uint64_t n, uint32_t* out_rank) {
  for (uint32_t r = 0; r < world; ++r) {
    const uint32_t s = where_row(table, n, r)[n];
    if (s != 0) {
      if (out_rank) *out_rank = r;
      return s;
    }
  }
  return 0;
}

// claimer[i] / cluster[i] of every request (kNoWord / kNoWord: in no list on any rank).  owner [k]: vers_shard_plan's owner of every list.
// An id claimed by two ranks, a claim by a rank that does not own the claimed list, a cluster >= k: the index is inconsistent.
inline WhereError where_resolve(const uint32_t* table, uint32_t world, uint64_t n, const uint8_t* owner, uint32_t k, uint32_t* claimer, uint32_t* cluster) {
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t who = kNoWord, c = kNoWord;
    for (uint32_t r = 0; r < world; ++r) {
      const uint32_t w = where_row(table, n, r)[i];
      if (w == kNoWord) continue;
      if (who != kNoWord) return kWhereDoubleClaim;
      if (w >= k) return kWhereBadCluster;
      if ((uint32_t)owner[w] != r) return kWhereNotOwner;
      who = r;
      c = w;
    }
    claimer[i] = who;
    cluster[i] = c;
  }
  return kWhereOk;
}

inline uint64_t where_chunks(uint64_t n, uint64_t R) { return R == 0 ? 0 : (n + R - 1) / R; }

// The row round's plan.  counts [chunks][world]: requests of chunk j that rank r found; pad [chunks]: the largest of them (0 = the chunk
// is skipped); slot [n]: a found request's row in its chunk's gathered buffer [world][pad[j]] (claimer * pad + its rank among the claimer's
// found requests of the chunk, in request order; a repeated id takes a slot per request), kNoWord for a request in no list.
// Returns the callbacks of the whole call: the where round + the non-empty chunks.
inline uint64_t where_plan_rows(const uint32_t* claimer, uint64_t n, uint32_t world, uint64_t R, std::vector<uint32_t>& counts, std::vector<uint32_t>& pad,
                                std::vector<uint32_t>& slot) {
  const uint64_t chunks = where_chunks(n, R);
  counts.assign((size_t)chunks * world, 0u);
  pad.assign((size_t)chunks, 0u);
  slot.assign((size_t)n, kNoWord);
  std::vector<uint32_t> within((size_t)n, 0u);
  for (uint64_t i = 0; i < n; ++i) {
    if (claimer[i] == kNoWord) continue;
    uint32_t& c = counts[(size_t)(i / R) * world + claimer[i]];
    within[i] = c++;
  }
  uint64_t calls = 1;
  for (uint64_t j = 0; j < chunks; ++j) {
    uint32_t m = 0;
    for (uint32_t r = 0; r < world; ++r) m = counts[(size_t)j * world + r] > m ? counts[(size_t)j * world + r] : m;
    pad[j] = m;
    if (m) ++calls;
  }
  for (uint64_t i = 0; i < n; ++i)
    if (claimer[i] != kNoWord) slot[i] = claimer[i] * pad[i / R] + within[i];
  return calls;
}

// The requests rank `me` found, in request order (what it packs), and where each chunk's run starts in that list: begin [chunks + 1].
inline void where_my_requests(const uint32_t* claimer, uint64_t n, uint32_t me, uint64_t R, std::vector<uint32_t>& req, std::vector<uint64_t>& begin) {
  const uint64_t chunks = where_chunks(n, R);
  req.clear();
  begin.assign((size_t)chunks + 1, 0);
  for (uint64_t i = 0; i < n; ++i) {
    if (claimer[i] != me) continue;
    req.push_back((uint32_t)i);
    begin[(size_t)(i / R) + 1] += 1;
  }
  for (uint64_t j = 0; j < chunks; ++j) begin[j + 1] += begin[j];
}

// bytes one rank sends in the row chunk j (rows at a pitch of exactly d floats)
inline uint64_t where_chunk_bytes(uint32_t pad, uint32_t d) { return (uint64_t)pad * d * 4u; }

}  // namespace shw
}  // namespace vers
