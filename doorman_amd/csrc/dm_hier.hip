// dm_hier.hip — the hierarchy kernels: k_publish (what a server sends upstream) and
// k_hier_tick (the root's round over its servers' requests).
#include <hip/hip_runtime.h>

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
__device__ __forceinline__ int hier_owner(const int64_t* lo, int G, int64_t r) {
  int a = 0, b = G;  // lo[a] <= r < lo[b]
  while (b - a > 1) {
    const int m = (a + b) >> 1;
    if (lo[m] <= r) a = m;
    else b = m;
  }
  return a;
}

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
  const bool valid = g0 < K && r < ha.r_hi;
  const int64_t rr = r < ha.r_hi ? r : ha.r_lo;
  const int64_t row = rr * K + (valid ? g0 : 0);
  // the server this row belongs to, and its record of the resource
  const int g = ha.shard_lo ? hier_owner(ha.shard_lo, ha.G, rr) : g0;
  const int64_t rec = ha.shard_lo ? rr - ha.shard_lo[g] : rr;
  double w = 0.0, h = 0.0, rw = 0.0;
  int s = 0, rs = 0;
  int64_t e = kReleased;
  bool req = false;
  uint32_t flags = 0;
  const Res rs_cfg = load_res(p, (int)rr);
  // every load the round needs is issued here, before the first is consumed: the
  // expiry column (root rows are explicit; read unconditionally instead of after the
  // subclients word) and this server's template inputs (one round trip instead of three)
  const bool mine = valid && g == ha.server;
  const int64_t li = mine ? rr - ha.leaf_lo : 0;  // the resource's index in this server's leaf
  int64_t learn = 0;
  ResCold rcc{0.0, 0, 0};
  if (mine) {
    learn = ha.leaf_prev_cfg[li].learning_end_ns;  // kept (resource.go:163)
    rcc = ha.root_cold[rr];
  }
  if (valid) {
    w = p.wants[row];
    h = p.has[row];
    const int32_t raw = p.sub[row];  // expiry encoding (dm_device.h): root rows are explicit or released
    const int64_t xe = p.expiry[row];
    s = sub_value(raw);
    e = sub_released(raw) ? kReleased : (raw < 0 ? xe : rs_cfg.follow_exp);
    const double2* blk = ha.gathered + (int64_t)g * ha.stride;
    flags = pub_flags(blk[0].x);
    const double2 v = blk[1 + rec];
    req = flags == 0u && v.x > 0.0;  // count in [1, kSubMax] when the flags are clear
    rw = v.x;
    rs = req ? (int)__double_as_longlong(v.y) : 0;
  }
  const bool released = e == kReleased;
  bool live = valid && !released && !(p.now > e);          // present after Clean (store.go:174)
  const bool expired = valid && !released && (p.now > e);  // released by this round's Clean
  const int base = rl * P;                                 // first lane of this resource
  auto src = [&](int q) { return base + q; };

  // Clean on the running sums, in row order (store.go:169-181 -> :142-151)
  long long count = rs_cfg.agg_count;
  double sh = rs_cfg.agg_has, sw = rs_cfg.agg_wants;
  const int xp = expired ? 1 : 0;
  if (__any(xp)) {
    for (int q = 0; q < K; ++q) {
      const double hj = shfl_d(h, src(q)), wj = shfl_d(w, src(q));
      const int sj = shfl_i(s, src(q)), xj = shfl_i(xp, src(q));
      if (xj) {
        sw -= wj;
        sh -= hj;
        count -= sj;
      }
    }
  }
  if (!live) {  // this row is absent from the store the round starts with
    h = 0.0;
    w = 0.0;
    s = 0;
  }

  const double C = rs_cfg.C;
  const bool ps = !rs_cfg.learning && rs_cfg.kind == 2;
  const int rq = req ? 1 : 0;
  double my_gets = 0.0;
  for (int q = 0; q < K; ++q) {
    const int rq_q = shfl_i(rq, src(q));
    if (!__any(rq_q)) continue;  // no resource of this wave has server q's request
    const double rw_q = shfl_d(rw, src(q));
    const int rs_q = shfl_i(rs, src(q));
    const int live_q = shfl_i(live ? 1 : 0, src(q));
    const double old_h = shfl_d(h, src(q)), old_w = shfl_d(w, src(q));  // store.Get: zero when absent
    const int old_s = shfl_i(s, src(q));
    // Decide (algorithm.go) for server q's request against the store as it is now
    double gets = 0.0, eq = 0.0, ds = 0.0, avail = 0.0;
    bool loop1 = false;
    if (rq_q) {
      if (rs_cfg.learning) {
        gets = 0.0;  // Learn: the request's Has (never filled by an intermediate)
      } else if (rs_cfg.kind == 0) {
        gets = rw_q;
      } else if (rs_cfg.kind == 1) {
        gets = minF(C, rw_q);
      } else if (ps) {
        const long long cnt = count + (live_q ? 0 : rs_q);  // :217-225
        eq = C / (double)cnt;                               // :229
        ds = eq * (double)rs_q;                             // :233 equalSharePerClient
        avail = C - sh + old_h;                             // :239 unusedCapacity
        if (sw <= C || rw_q <= ds) gets = minF(rw_q, avail);  // :245
        else loop1 = true;
      } else {
        const long long cnt = count - old_s + rs_q;  // :115
        avail = C - sh + old_h;                      // :120
        eq = C / (double)cnt;                        // :123
        ds = eq * (double)rs_q;                      // :126
        if (rw_q <= ds) gets = minF(rw_q, avail);    // :131
        else loop1 = true;
      }
    }
    if (__any(loop1)) {
      // store.Map over the rows in row order (absent rows are not in the map)
      const int sl = live ? s : ~s;  // subclients + live bit (s >= 0)
      double x = 0.0, y = 0.0;
      long long wx = rs_q;  // FairShare wantExtra starts at the request's subclients (:148)
      for (int j = 0; j < K; ++j) {
        const double wj = shfl_d(w, src(j));
        const int sj = shfl_i(sl, src(j));
        if (!loop1 || sj < 0) continue;
        if (ps) {  // with server q's own request values for its row (:259-279)
          const double wv = (j == q) ? rw_q : wj;
          const int sv = (j == q) ? rs_q : sj;
          const double esp = eq * (double)sv;  // :273
          if (wv < esp)
            x += esp - wv;  // :275
          else
            y += wv - esp;  // :277
        } else if (j != q) {  // FairShare round 1, the requesting server skipped (:156-171)
          const double d = (double)sj * eq;  // :160
          if (wj < d)
            x += d - wj;  // :164
          else if (wj > d)
            wx += sj;  // :168
        }
      }
      bool loop2 = false;
      double dE = 0.0, T = 0.0;
      if (loop1) {
        if (ps) {
          gets = minF(ds + (rw_q - ds) * (x / y), avail);  // :283,290
        } else {
          dE = (x / (double)wx) * (double)rs_q;  // :175
          if (rw_q < ds + dE) gets = minF(rw_q, avail);  // :179
          else {
            T = dE + ds;  // :197 deservedExtra + deservedShare
            loop2 = true;
          }
        }
      }
      if (__any(loop2)) {
        double ee = 0.0;
        long long wee = rs_q;  // :189
        for (int j = 0; j < K; ++j) {
          const double wj = shfl_d(w, src(j));
          const int sj = shfl_i(sl, src(j));
          if (!loop2 || sj < 0 || j == q) continue;
          if (!(wj > (double)sj * eq)) continue;  // wantExtraClients (:165-169)
          if (wj < T)
            ee += T - wj;  // :197-198
          else if (wj > T)
            wee += sj;  // :199-200
        }
        if (loop2) gets = minF(ds + dE + (ee / (double)wee) * (double)rs_q, avail);  // :203-204
      }
    }
    // Assign (store.go:153-167): the running sums, and server q's row
    if (rq_q) {
      sh += gets - old_h;
      sw += rw_q - old_w;
      count += rs_q - old_s;
      if (g0 == q) {  // this lane is row q
        h = gets;
        w = rw_q;
        s = rs_q;
        live = true;
        my_gets = gets;
      }
    }
  }

  // the round's rows: the requests' leases, and the rows this round's Clean released
  const int64_t exp_new = rs_cfg.exp_out;
  if (valid) {
    if (req) {  // the root store is written in place (out_* alias its columns)
      p.out_gets[row] = my_gets;
      p.out_wants[row] = rw;
      p.out_sub[row] = (int32_t)((uint32_t)rs | kSubExplicit);
      p.out_expiry[row] = exp_new;
    } else if (expired) {
      p.out_gets[row] = 0.0;
      p.out_wants[row] = 0.0;
      p.out_sub[row] = (int32_t)kSubReleased;
      p.out_expiry[row] = kReleased;
    }
  }
  if (valid && g0 == 0) {  // the resource's first lane
    ResAgg a;
    a.count = count;
    a.sum_has = sh;
    a.sum_wants = sw;
    a.follow_exp = rs_cfg.follow_exp;
    p.res[rr] = a;
    p.expl[rr] = 1;  // the rows this tick writes carry explicit expiries
  }

  // this server's new template for the resource (server.go:279-313)
  if (mine) {
    ResCfg* c = ha.leaf_cfg + li;
    ResCold* cc = ha.leaf_cold + li;
    if (flags != 0u) {  // rejected: the templates stay (a staged slot takes a copy)
      if (ha.leaf_prev_cfg != ha.leaf_cfg) {
        *c = ha.leaf_prev_cfg[li];
        *cc = ha.leaf_prev_cold[li];
      }
    } else if (req) {
      const int64_t sec = exp_new >= 0 ? exp_new / kNs : -((-exp_new + kNs - 1) / kNs);  // time.Unix(sec, 0)
      ResCfg t;
      t.capacity = my_gets;               // :293
      t.learning_end_ns = learn;
      t.parent_expiry_ns = sec * kNs;     // :287-288
      // :295 Algorithm, from the config loaded up front (no reload after the stores above)
      t.lease_len_s = (int32_t)((exp_new - p.now) / kNs);
      t.kind = rs_cfg.kind;
      *c = t;
      ResCold tc;
      tc.safe_capacity = __builtin_isnan(rcc.safe_capacity) ? 0.0 : rcc.safe_capacity;  // :294, :894
      tc.refresh_s = rcc.refresh_s;
      tc.pad = 0;
      *cc = tc;
    } else {  // the "*" default template (server.go:53-63, :305)
      ResCfg t;
      t.capacity = 0.0;
      t.learning_end_ns = learn;
      t.parent_expiry_ns = INT64_MAX;  // expiryTimes has no entry: nil
      t.lease_len_s = 20;
      t.kind = 3;
      *c = t;
      ResCold tc;
      tc.safe_capacity = 0.0;
      tc.refresh_s = 1;
      tc.pad = 0;
      *cc = tc;
    }
  }
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
