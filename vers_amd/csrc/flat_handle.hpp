// flat_handle.hpp -- the handle behind vers_flat_* (flat.hip owns it; the test library's flat hooks, csrc/testhooks/flat_audit.hip,
// read its shadow through this header).
#pragma once
#include <mutex>

#include "flat_shadow.hpp"
#include "range_scratch.hpp"

struct vers_flat {
  int device = 0;
  uint32_t d = 0, ld = 0;  // ld = round_up(d, kColAlign): columns of the blocked corpus and of padded queries
  uint64_t n = 0;
  float* rows = nullptr;   // lane-transposed tiles (scan.hip.h)
  size_t rows_cap = 0;
  int n_cu = 256;
  // workspace (grown on demand, never inside a steady-state call)
  float* q_stage = nullptr;
  size_t q_stage_cap = 0;
  float* q_up = nullptr;  // host-pointer calls: uploaded queries (grow-only: no allocation in a steady-state call)
  size_t q_up_cap = 0;
  float* zero_q = nullptr;
  uint32_t zero_q_len = 0;
  uint64_t* partials = nullptr;  // partial slots, then one pruning bound per query
  size_t partials_cap = 0;
  uint64_t* lower = nullptr;     // top_k > 64: the previous pass's last key per query
  size_t lower_cap = 0;
  size_t bounds_off = 0;
  uint32_t* status_dev = nullptr;
  uint64_t* o_ids = nullptr;
  float* o_dist = nullptr;
  uint32_t* o_cnt = nullptr;
  size_t o_cap = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool ev_valid = false;
  // range search (flat.hip: flat_range_dev_locked; grow-only like the rest): the protocol's scratch | staged queries | radii and CSR limits
  // of a host-pointer call (its ids / distances land in o_ids / o_dist)
  vers::RangeScratch rg;
  vers::DevBuf rg_q, rg_rad, rg_lims;
  vers::FlatShadow shadow;  // fp16 shadow of the rows + what a single query's exact finish needs (flat_shadow.hpp); empty when it did not fit
  std::mutex mu;
};
