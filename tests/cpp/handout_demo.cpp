// Host check of the list scan's hand-out of quads (vers_amd/csrc/prescan.hip.h: pre_run_len, kPreMaxRun -- the text the test cuts
// out of the header).  n_blocks blocks draw runs from ONE counter the way prescan_kernel_g's thread 0 does: a relaxed load of the
// counter (`seen`), the run length from pre_run_len(seen, ..), then an atomicAdd of that length whose return value is where the run
// starts.  The two steps of a block are interleaved at random with every other block's, so the counter has usually moved between a
// block's load and its add; a second schedule makes EVERY block load before any block adds (the launch's first instant).  Checked:
// every quad is handed out exactly once; every run is 1 .. kPreMaxRun long; a run computed inside the hot region is one quad; a run
// computed behind the hot region never starts inside it; without a hot count the length is the guided rule's for every `seen`; a
// hot count beyond n_quads behaves like n_quads.
#include <cstdint>
#include <cstdio>
#include <vector>

#define __host__
#define __device__
#include "handout_snip.h"

using vers::kPreMaxRun;
using vers::pre_run_len;

// the rule before there was a hot region: remaining / (2 * blocks), 1 .. 8
static uint32_t guided(uint32_t seen, uint32_t n_quads, uint32_t n_blocks) {
  uint32_t r = seen < n_quads ? (n_quads - seen) / (2u * n_blocks) : 1u;
  return r < 1u ? 1u : (r > 8u ? 8u : r);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)((rng_state >> 24) % n);
}

static long long violations = 0, handouts = 0, cases = 0;
static void bad(const char* what, uint32_t nq, uint32_t hot, uint32_t nb, uint32_t seen, uint32_t start, uint32_t r) {
  if (++violations <= 20) printf("VIOLATION %s: n_quads %u hot %u blocks %u seen %u start %u run %u\n", what, nq, hot, nb, seen, start, r);
}

// schedule 0: random interleaving of loads and adds; 1: every block loads first (all see 0), then random; 2: round robin
static void replay(uint32_t nq, uint32_t hot, uint32_t nb, int schedule) {
  ++cases;
  const uint32_t hot_eff = hot < nq ? hot : nq;
  std::vector<uint32_t> times(nq, 0u), seen(nb, 0u);
  std::vector<uint8_t> has_seen(nb, 0);
  std::vector<uint32_t> live(nb);
  for (uint32_t b = 0; b < nb; ++b) live[b] = b;
  uint32_t counter = 0;
  if (schedule == 1)
    for (uint32_t b = 0; b < nb; ++b) { seen[b] = counter; has_seen[b] = 1; }
  uint64_t guard = 0, rr = 0;
  while (!live.empty()) {
    if (++guard > 64ull * ((uint64_t)nq + nb) + 1024) { bad("no termination", nq, hot, nb, 0, counter, 0); return; }
    const uint32_t at = schedule == 2 ? (uint32_t)(rr++ % live.size()) : rnd((uint32_t)live.size());
    const uint32_t b = live[at];
    if (!has_seen[b]) { seen[b] = counter; has_seen[b] = 1; continue; }   // the relaxed load
    const uint32_t r = pre_run_len(seen[b], nq, hot, nb);
    const uint32_t start = counter;                                       // the atomicAdd's return value
    counter += r;
    has_seen[b] = 0;
    ++handouts;
    if (r < 1u || r > kPreMaxRun) bad("run length out of 1 .. kPreMaxRun", nq, hot, nb, seen[b], start, r);
    if (seen[b] < hot_eff && r != 1u) bad("a run computed inside the hot region is not one quad", nq, hot, nb, seen[b], start, r);
    if (seen[b] >= hot_eff && r != guided(seen[b], nq, nb)) bad("behind the hot region: not the guided rule", nq, hot, nb, seen[b], start, r);
    if (seen[b] >= hot_eff && start < hot_eff) bad("a run computed behind the hot region starts inside it", nq, hot, nb, seen[b], start, r);
    if (start >= nq) { live[at] = live.back(); live.pop_back(); continue; }   // the kernel's `break`
    const uint32_t end = start + r < nq ? start + r : nq;
    for (uint32_t q = start; q < end; ++q) ++times[q];
  }
  for (uint32_t q = 0; q < nq; ++q)
    if (times[q] != 1u) { bad("a quad handed out other than once", nq, hot, nb, q, q, times[q]); break; }
}

int main() {
  const uint32_t nqs[] = {0u, 1u, 7u, 4096u, 5763u};
  const uint32_t nbs[] = {1u, 2u, 192u, 256u, 512u};
  for (uint32_t nq : nqs)
    for (uint32_t nb : nbs) {
      const uint32_t hots[] = {0u, 1u, nq / 2u, nq, nq + 1u, 2u * nq + 1000u, 0xFFFFFFFFu};
      for (uint32_t hot : hots) {
        for (int rep = 0; rep < 3; ++rep) replay(nq, hot, nb, 0);
        replay(nq, hot, nb, 1);
        replay(nq, hot, nb, 2);
        // a hot count beyond n_quads is n_quads', for every seen (past the end too)
        if (hot > nq)
          for (uint32_t seen = 0; seen <= nq + 8u * nb + 8u; ++seen)
            if (pre_run_len(seen, nq, hot, nb) != pre_run_len(seen, nq, nq, nb)) bad("hot count beyond n_quads not clamped", nq, hot, nb, seen, 0, 0);
      }
      // no hot count: the guided rule for EVERY seen, the counter's overshoot past n_quads included
      for (uint32_t seen = 0; seen <= nq + 8u * nb + 8u; ++seen)
        if (pre_run_len(seen, nq, 0u, nb) != guided(seen, nq, nb)) bad("without a hot count: not the guided rule", nq, 0, nb, seen, 0, 0);
      if (pre_run_len(0xFFFFFFFFu, nq, 0u, nb) != 1u || pre_run_len(0xFFFFFFFFu, nq, 0xFFFFFFFFu, nb) != 1u) bad("seen at the counter's end", nq, 0, nb, 0xFFFFFFFFu, 0, 0);
    }
  printf("CASES %lld HANDOUTS %lld VIOLATIONS %lld\n", cases, handouts, violations);
  return violations ? 1 : 0;
}
