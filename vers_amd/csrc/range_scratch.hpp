// range_scratch.hpp -- what a range call (range_driver.hip.h) keeps between its two passes; a workspace of the index and the flat handle own one each.
#pragma once
#include "kmeans.hpp"

namespace vers {

// hits per slot | their exclusive prefix | [0..1] total, [2] status, [3] NaN-radius flag | staging of the sorted order (keys in | keys out, and
// ids in where ids travel beside the keys) | rocPRIM's temporary; grow-only like every scratch buffer
struct RangeScratch {
  DevBuf counts, base, misc, stage, tmp;
  uint32_t* pin = nullptr;  // pinned [4]: where the call reads its total, status word and NaN-radius flag after its first synchronisation
  hipEvent_t ev[6] = {};    // phase boundaries of the most recent call (vers_range_phases), created on first use
  void release() {          // (the buffers free themselves)
    if (pin) (void)hipHostFree(pin);
    pin = nullptr;
    for (auto& e : ev)
      if (e) { (void)hipEventDestroy(e); e = nullptr; }
  }
};

}  // namespace vers
