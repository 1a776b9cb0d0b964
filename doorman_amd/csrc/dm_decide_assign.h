// dm_decide_assign.h — what the host decides of a round's Assign (dm_decide_assign,
// dm_decide.cpp) beyond the round's plan (dm_decide_plan.h): which requests' values the store
// takes, and from that the element count of every device buffer the Assign adds to the round
// (dm_decide_round.h AssignCols holds the buffers).  The reference ends every Decide with
// store.Assign (resource.go:100-113, store.go:153-167), so after a round a row holds the values
// of the last request made on it; the requests before it on the same row were seen by the
// decisions between them (the round's scratch copy) and are overwritten.  The gather kernel
// (dm_decide_assign.hip) trusts these numbers: a position past the round or a count too small
// is an access out of bounds.  Plain C++17, no HIP: tested on the CPU
// (tests/test_decide_assign_plan.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <unordered_set>
#include <vector>

#include "dm_decide_plan.h"

namespace dm {

// The selection: the grouped positions (RoundPlan::order's indices) of the last request on
// each distinct row, ascending.  The grouped order is stable within a resource and a row
// belongs to one resource, so a row's last grouped position is its last request in the
// caller's order.  One entry per distinct row: the rows of the selection are unique, which
// is what the upsert's row step asks of a call.
struct AssignSel {
  std::vector<int64_t> sel;  // [m], 1 <= m <= n for a round of n >= 1 requests
  int64_t n = 0;             // the round's requests
  int64_t m() const { return (int64_t)sel.size(); }
};

// plan: the round's (without error); rows: the caller's n request rows.
inline AssignSel assign_selection(const RoundPlan& plan, const int64_t* rows) {
  AssignSel a;
  a.n = plan.n;
  std::unordered_set<int64_t> seen;
  seen.reserve((size_t)(2 * plan.n));
  for (int64_t i = plan.n - 1; i >= 0; --i)
    if (seen.insert(rows[plan.order[(size_t)i]]).second) a.sel.push_back(i);
  std::reverse(a.sel.begin(), a.sel.end());
  return a;
}

// The buffers the Assign adds to the round (AssignCols' members of the same names), and the
// one rule of how many elements each holds.
enum class AssignBuf : uint8_t {
  sel,                         // the selection
  rows, has, wants, sub, exp,  // the compact columns the upsert's row step reads: one entry per selected request
  safe                         // SetSafeCapacity's value per request, in grouped order
};
constexpr int kAssignBufs = (int)AssignBuf::safe + 1;

inline int64_t assign_count(const AssignSel& a, AssignBuf buf) {
  return buf == AssignBuf::safe ? a.n : a.m();  // [n requests], else [distinct rows]
}

}  // namespace dm
