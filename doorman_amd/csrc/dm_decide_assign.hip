// dm_decide_assign.hip — the two kernels dm_decide_assign (dm_decide.cpp) adds around the
// upsert's row step, which is the round's Assign (dm_update.hip k_check_rows, k_upsert,
// k_clear_rows, launched by dm_store_update.cpp as for dm_store_upsert_device):
//   k_assign_gather   before it: the values of the selected requests (dm_decide_assign.h:
//                     the last request on each distinct row), gathered from the round's
//                     grouped columns into the compact columns the row step reads
//   k_safe_capacity   after it: SetSafeCapacity's value (resource.go:81-96) of every
//                     request's resource, from the count the Assign left
// Neither writes the store, adds to a running sum or uses an atomic: the store is written by
// the upsert's kernels alone.  Both move a few bytes per lane; what they are for is that the
// round's results stay in device memory between the decision and the Assign.
#include <hip/hip_runtime.h>

#include "dm_kernel_util.h"
#include "dm_launch.h"
#include "dm_update_util.h"

namespace dm {

// One lane per selected request: lane i reads position sel[i] of the grouped columns (sel
// ascends, so a wave's loads fall within a short span) and stores entry i of the compact ones
// (consecutive lanes, consecutive words).  The host made sel from the plan the grouped columns
// were staged by: 0 <= sel[i] < n, and every compact column holds m entries.
__global__ __launch_bounds__(256) void k_assign_gather(ReqArgs q, AssignArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.m) return;
  const int64_t k = a.sel[i];
  a.rows[i] = q.rows[k];
  a.has[i] = q.gets[k];
  a.wants[i] = q.wants[k];
  a.sub[i] = q.sub[k];
  a.exp[i] = q.expiry[k];
}

// One lane per request in grouped order: its row's resource (the requests of a resource are
// adjacent, so a wave reads one or a few resources' records) and safe_capacity_of
// (dm_device.h) of that resource's configuration and running count.  rows were checked
// against the store's N by the round's plan.
__global__ __launch_bounds__(256) void k_safe_capacity(int64_t n, const int64_t* __restrict__ rows, RowIndex ix,
                                                       const ResCfg* __restrict__ cfg, const ResCold* __restrict__ cold,
                                                       const ResAgg* __restrict__ agg, double* __restrict__ safe) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int seg = seg_of_row(ix, rows[k]);
  safe[k] = safe_capacity_of(cfg[seg].capacity, cold[seg].safe_capacity, agg[seg].count);
}

hipError_t launch_assign_gather(const ReqArgs& q, const AssignArgs& a, hipStream_t st) {
  if (a.m <= 0) return hipSuccess;
  k_assign_gather<<<(unsigned)((a.m + 255) / 256), 256, 0, st>>>(q, a);
  return hipGetLastError();
}

hipError_t launch_safe_capacity(int64_t n, const int64_t* rows, const RowIndex& ix, const ResCfg* cfg,
                                const ResCold* cold, const ResAgg* agg, double* safe, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  k_safe_capacity<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(n, rows, ix, cfg, cold, agg, safe);
  return hipGetLastError();
}

}  // namespace dm
