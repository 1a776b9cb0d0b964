// dm_hier.hip — the hierarchy kernels: k_publish (what a server sends upstream) and
// k_hier_tick (the root's round over its servers' requests).
#include <hip/hip_runtime.h>

#include "dm_hier_round.h"
#include "dm_kernel_util.h"
#include "dm_launch.h"

namespace dm {

// server.go:234-255: what an intermediate server sends upstream -- {SumWants, Count}
// of every resource it holds (a band only when SumWants > 0, :241) -- plus the root's
// validation of that request (:858-868), computed here once instead of by every
// root copy: a band with Count < 1 fails the whole GetServerCapacity with
// InvalidArgument (:863-866), and a Count beyond the root's 32-bit subclients
// column is rejected the same way (kHierCountRange).  dst[1 + r] = the record of
// resource r; dst[0] = {the flags of the whole request, 0}, written by the last
// workgroup to arrive (sync[0] accumulates the workgroups' flags, sync[1] counts
// them; both return to zero for the next launch).
__global__ __launch_bounds__(256) void k_publish(int64_t R, const ResAgg* __restrict__ agg, double2* __restrict__ dst,
                                                 uint32_t* sync, int nblocks) {
  __shared__ uint32_t wf[4];
  uint32_t f = 0;
  // a few workgroups striding over the records: each one arrives at the counter once
  // (hundreds of contended arrivals cost ~10 us per launch at R = 100k)
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < R; r += (int64_t)nblocks * 256) {
    const ResAgg a = agg[r];
    double2 v;
    v.x = a.sum_wants;
    v.y = __longlong_as_double(a.count);
    dst[1 + r] = v;
    if (a.sum_wants > 0.0) {  // a band (server.go:241)
      if (a.count < 1) f |= kHierInvalid;
      if (a.count > kSubMax) f |= kHierCountRange;
    }
  }
  const uint32_t w = (__ballot(f & kHierInvalid) ? kHierInvalid : 0u) | (__ballot(f & kHierCountRange) ? kHierCountRange : 0u);
  if ((threadIdx.x & 63) == 0) wf[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x < 64) {
    if (threadIdx.x == 0) {
      const uint32_t all = wf[0] | wf[1] | wf[2] | wf[3];
      if (all) (void)__hip_atomic_fetch_or((gu32*)sync, all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (arrive_last(sync + 1, nblocks) && threadIdx.x == 0) {
      const uint32_t flags = __hip_atomic_load((gu32*)sync, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store((gu32*)sync, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      double2 v;
      v.x = __longlong_as_double((long long)flags);
      v.y = 0.0;
      dst[0] = v;
    }
  }
}

// One exchange round of the root.  The requests of the servers that ask for a
// resource -- {has 0 (the intermediate never fills Has, server.go:244,873), wants
// SumWants_g, subclients Count_g} -- are decided by Resource.Decide one after
// another in server order, as the root's res.mu serialises the GetServerCapacity
// calls (resource.go:103-104): Clean once (resource.go:106, store.go:169-181;
// nothing else expires within the round), then per request Learn or the algorithm
// (algorithm.go:95-302, with the request's own values for its server) against
// the store as the Assigns of the earlier requests left it, then its Assign
// (store.go:153-167: the row and the running sums).  So the root never grants
// more than the reference would: a FairShare resource with capacity C and G
// servers that each want C grants C, 0, ... in the first round, not G x C.
// Servers that do not request keep their root lease until Clean expires it.  The
// running sums follow the reference's update sequence -- Clean's releases in row
// order, then one Assign per request in server order -- bit for bit.
//
// Layouts (HierArgs): replicated -- every server holds every resource, the root
// store has K = G rows per resource (row r*G + g = server g); sharded -- server g
// holds resources [lo[g], lo[g+1]) (contiguous resource-id ranges),
// so only the owner ever requests resource r and the root store has one row per
// resource (K = 1); there each rank decides only its own range [r_lo, r_hi): no
// other server requests those resources and no other resource's root rows reach this
// server's leaf, so the launch shrinks with the shard (the other ranks decide theirs).
// A server whose published flags are set (a band with
// num_clients < 1, server.go:863-866, or a Count beyond 2^31 - 2) requests nothing
// this round.
//
// K <= 64 rows: a wave holds 64 / P whole resources (P = K rounded up to a power
// of two), one lane per row.  For each row q in order, the lanes of a resource
// walk its rows in row order by shuffles for the decision's loops over store.Map
// (round 1, round 2, ProportionalShare's extra capacity / need: the sums of a
// sequential Map, bit for bit the oracle's); lane q then takes the Assign.  O(K)
// per decision, K decisions per resource.
// The lane of `ha.server` then writes that server's template for each of its
// resources exactly as performRequests + LoadConfig do (server.go:279-313,
// resource.go:117-125): a requested resource takes the root's grant as capacity,
// its expiry (Unix seconds) as the parent expiry, and the root's algorithm
// (kind, lease length, refresh) and configured safe capacity (0 when unset,
// server.go:894); a resource it did not request drops to the "*" default
// template (server.go:53-63: capacity 0, safe 0, FAIR_SHARE, lease 20 s, refresh
// 1 s, no parent expiry); a rejected round keeps the templates it had
// (performRequests returns before LoadConfig, :268-272).  learningModeEndTime is
// kept (set once, resource.go:163).
__global__ __launch_bounds__(256) void k_hier_tick(DevParams p, HierArgs ha) {
  const int K = ha.K;
  const int P = K <= 1 ? 1 : 1 << (32 - __builtin_clz((unsigned)(K - 1)));
  const int per = 64 / P;  // resources per wave
  const int lane = threadIdx.x & 63;
  const int rl = lane / P, g0 = lane - rl * P;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x < ha.G)  // the round's per-server flags (dm_hier_status)
    ha.status_out[threadIdx.x] = pub_flags(ha.gathered[(int64_t)threadIdx.x * ha.stride].x);
  const int64_t r = ha.r_lo + wave * per + rl;
  if (ha.r_lo + wave * per >= ha.r_hi) return;  // whole waves only
  HierLane ln;
  ln.valid = g0 < K && r < ha.r_hi;
  ln.rr = r < ha.r_hi ? r : ha.r_lo;
  ln.row = ln.rr * K + (ln.valid ? g0 : 0);
  ln.g0 = g0;
  ln.base = rl * P;  // first lane of this resource
  // the server this row belongs to, and its record of the resource
  ln.g = ha.shard_lo ? hier_owner(ha.shard_lo, ha.G, ln.rr) : g0;
  ln.rec = ha.shard_lo ? ln.rr - ha.shard_lo[ln.g] : ln.rr;
  ln.mine = ln.valid && ln.g == ha.server;
  // the lane's body (dm_hier_round.h): the loads, then Clean, the decisions, the Assigns, the stores
  const HierLoads ld = hier_round_load(p, ha, ln);
  hier_round_decide<false>(p, ha, ln, ld);
}

// --------------------------------------------------------------------------
// host-side launchers (called by dm_hier_host.cpp)
// --------------------------------------------------------------------------
hipError_t launch_publish(int64_t R, const ResAgg* agg, void* dst, uint32_t* sync, hipStream_t st) {
  const int nb = (int)std::min<int64_t>(64, std::max<int64_t>(1, (R + 255) / 256));
  k_publish<<<(unsigned)nb, 256, 0, st>>>(R, agg, (double2*)dst, sync, nb);
  return hipGetLastError();
}

hipError_t launch_hier_tick(const DevParams& p, const HierArgs& ha, hipStream_t st) {
  if (ha.R <= 0) return hipSuccess;
  int P = 1;
  while (P < ha.K) P <<= 1;
  const int64_t per = 64 / P;
  // at least one workgroup: block 0 also writes the round's per-server flags
  const int64_t waves = std::max<int64_t>(1, (ha.r_hi - ha.r_lo + per - 1) / per);
  k_hier_tick<<<(unsigned)((waves + 3) / 4), 256, 0, st>>>(p, ha);
  return hipGetLastError();
}

}  // namespace dm
