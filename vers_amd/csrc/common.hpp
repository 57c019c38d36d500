// Shared declarations for libvers_hip.so (MI355X / gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/vers_hip.h"
#include "seg_plan.hpp"  // the scan engine's geometry: kWave, kChunk, ..., round_up, scan_grid, SegPlan

namespace vers {

// ---- error plumbing (thread-local message behind vers_last_error) ----------
void set_error(const std::string& msg);
int32_t fail(int32_t status, const std::string& msg);

#define VERS_HIP_TRY(expr)                                                                     \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess)                                                                      \
      return ::vers::fail(VERS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));    \
  } while (0)

constexpr uint64_t kKeyMax = 0xFFFFFFFFFFFFFFFFull;

// the option table (core.hip): vers_set_option / VERS_OPTIONS="name=value,..." -- the value when set, else `dflt`
int64_t opt_get(const char* name, int64_t dflt);
bool opt_set(const char* name, int64_t v);  // false: no such option
uint32_t scan_debug_flags();  // option "scan_debug" (diagnosis only; 0 in production)

// Device-side view of the result of a scan: `k` ascending keys per slot.
// key = (order-preserving f32 bits << 32) | seq, seq = tie-break position.

}  // namespace vers
