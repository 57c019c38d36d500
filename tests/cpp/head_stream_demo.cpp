// Host check of the head filter's stream of tile prefixes (vers_amd/csrc/prescan.hip.h: kHeadPrefix, head_stream_len, head_stream_pos --
// the text the test cuts out of the header).  A wave of head_filter_kernel keeps a ring of R slots ahead in the stream: positions
// 0 .. R - 1 go out when the segment is entered, and the slot of position p is issued again with position p + R once p is consumed.
// Replayed here for n_tiles 0 .. 12 and R 2 .. 4.  Checked: every position issued maps inside [0, n_tiles) x [0, kHeadPrefix); the step
// a slot holds when it is consumed is the one the walk is at, so each (tile, step) of the prefix stream is visited exactly once and in
// order; positions past the end repeat the last valid step; a segment without tiles has no position and issues nothing.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

#define __host__
#define __device__
#include "head_stream_snip.h"

using vers::HeadStreamPos;
using vers::head_stream_len;
using vers::head_stream_pos;
using vers::kHeadPrefix;

static long long violations = 0, issues = 0, cases = 0;
static void bad(const char* what, uint32_t n_tiles, uint32_t R, uint32_t p) {
  if (++violations <= 20) printf("VIOLATION %s: n_tiles %u R %u position %u\n", what, n_tiles, R, p);
}

int main() {
  for (uint32_t n_tiles = 0; n_tiles <= 12; ++n_tiles)
    for (uint32_t R = 2; R <= 4; ++R) {
      ++cases;
      const uint32_t len = head_stream_len(n_tiles);
      if (len != n_tiles * kHeadPrefix) bad("length", n_tiles, R, len);
      // the kernel's guard, as it stands in `enter`: a segment is walked, and anything issued, only where the stream has a position
      const bool walked = head_stream_len(n_tiles) != 0u;
      if (walked != (n_tiles != 0u)) bad("guard", n_tiles, R, 0);
      if (!walked) {  // nothing is issued; the mapping is total all the same (no wrap-around to position 2^32 - 1)
        for (uint32_t p : {0u, 1u, R, 0xFFFFFFFFu}) {
          const HeadStreamPos at = head_stream_pos(p, n_tiles);
          if (at.tile != 0u || at.step != 0u) bad("without tiles: not (0, 0)", n_tiles, R, p);
        }
        continue;
      }
      std::vector<HeadStreamPos> slot(R);
      std::vector<uint32_t> seen(len, 0u);
      auto issue = [&](uint32_t p) {
        const HeadStreamPos at = head_stream_pos(p, n_tiles);
        ++issues;
        if (at.tile >= n_tiles || at.step >= kHeadPrefix) bad("outside the segment", n_tiles, R, p);
        if (p < len) {
          if (at.tile * kHeadPrefix + at.step != p) bad("not the stream's order", n_tiles, R, p);
          else ++seen[p];
        } else if (at.tile != n_tiles - 1 || at.step != kHeadPrefix - 1) {
          bad("past the end: not the last valid step", n_tiles, R, p);
        }
        slot[p % R] = at;
      };
      for (uint32_t r = 0; r < R; ++r) issue(r);
      for (uint32_t t = 0; t < n_tiles; ++t)
        for (uint32_t s = 0; s < kHeadPrefix; ++s) {
          const uint32_t p = t * kHeadPrefix + s;
          if (slot[p % R].tile != t || slot[p % R].step != s) bad("the slot does not hold the step the walk is at", n_tiles, R, p);
          issue(p + R);
        }
      for (uint32_t p = 0; p < len; ++p)
        if (seen[p] != 1u) bad("a step of the stream requested other than once", n_tiles, R, p);
      for (uint32_t p = len; p < len + 64u; ++p) {  // far past the end, and at the top of the range
        const HeadStreamPos at = head_stream_pos(p, n_tiles), hi = head_stream_pos(0xFFFFFFFFu - (p - len), n_tiles);
        if (at.tile != n_tiles - 1 || at.step != kHeadPrefix - 1 || hi.tile != at.tile || hi.step != at.step) bad("clamp", n_tiles, R, p);
      }
    }
  printf("CASES %lld ISSUES %lld VIOLATIONS %lld\n", cases, issues, violations);
  return violations != 0;
}
