// dm_hier_round.h — one lane's share of the root's exchange round: the body of k_hier_tick
// (dm_hier.hip has the account of the round and of its layouts), in two steps so that a caller
// can put loads of its own between them: hier_round_load issues every load the lane needs,
// hier_round_decide consumes them (Clean, the K decisions in server order, the Assigns, the
// root row and sums stores where a word's bits changed, this server's template).
//
// ONE: K = 1 fixed at compile time, one server (G = 1, so g = 0 and the record of resource r
// is record 1 + r of block 0): a lane is a whole resource, the shuffles are identities, the
// `j != q` loops are empty, and no lane needs another, so the lanes of a wave may diverge
// around the call.  k_block_fused's ROOT build (dm_tick_fused.hip) calls it so; k_hier_tick
// calls the general form.  One source: the floating-point statements are the same in both,
// and both units build with -ffp-contract=off.
#pragma once
#include "dm_kernel_util.h"

namespace dm {

__device__ __forceinline__ int hier_owner(const int64_t* lo, int G, int64_t r) {
  int a = 0, b = G;  // lo[a] <= r < lo[b]
  while (b - a > 1) {
    const int m = (a + b) >> 1;
    if (lo[m] <= r) a = m;
    else b = m;
  }
  return a;
}

// Which row of which resource a lane holds.
struct HierLane {
  int64_t rr;   // the resource (a valid one even where the lane is not: loads stay in bounds)
  int64_t row;  // its root row
  int g0;       // the row's index within the resource = the server it belongs to (replicated)
  int base;     // first lane of this resource in the wave
  int g;        // the server this row belongs to
  int64_t rec;  // ... and that server's record of the resource
  bool valid, mine;
};

// Everything the round reads, as loaded.
struct HierLoads {
  Res rs_cfg;
  int64_t learn;
  ResCold rcc;
  double w, h;
  int32_t raw;
  int64_t xe;
  double b0;  // record 0 of the server's block: its flags
  double2 v;  // the server's record of the resource
};

// every load the round needs is issued here, before the first is consumed: the
// expiry column (root rows are explicit; read unconditionally instead of after the
// subclients word) and this server's template inputs (one round trip instead of three)
__device__ __forceinline__ HierLoads hier_round_load(const DevParams& p, const HierArgs& ha, const HierLane& ln) {
  HierLoads ld;
  ld.rs_cfg = load_res(p, (int)ln.rr);
  ld.learn = 0;
  ld.rcc = ResCold{0.0, 0, 0};
  ld.w = ld.h = 0.0;
  ld.raw = 0;
  ld.xe = 0;
  ld.b0 = 0.0;
  ld.v = double2{0.0, 0.0};
  if (ln.mine) {
    ld.learn = ha.leaf_prev_cfg[ln.rr - ha.leaf_lo].learning_end_ns;  // kept (resource.go:163)
    ld.rcc = ha.root_cold[ln.rr];
  }
  if (ln.valid) {
    ld.w = p.wants[ln.row];
    ld.h = p.has[ln.row];
    ld.raw = p.sub[ln.row];  // expiry encoding (dm_device.h): root rows are explicit or released
    ld.xe = p.expiry[ln.row];
    const double2* blk = ha.gathered + (int64_t)ln.g * ha.stride;
    ld.b0 = blk[0].x;
    ld.v = blk[1 + ln.rec];
  }
  return ld;
}

template <bool ONE>
__device__ __forceinline__ void hier_round_decide(const DevParams& p, const HierArgs& ha, const HierLane& ln,
                                                  const HierLoads& ld) {
  const int K = ONE ? 1 : ha.K;
  const bool valid = ln.valid, mine = ln.mine;
  const int64_t rr = ln.rr, row = ln.row;
  const int g0 = ln.g0;
  const Res& rs_cfg = ld.rs_cfg;
  const int64_t li = mine ? rr - ha.leaf_lo : 0;  // the resource's index in this server's leaf
  const int64_t learn = ld.learn;
  const ResCold rcc = ld.rcc;
  double w = 0.0, h = 0.0, rw = 0.0;
  int s = 0, rs = 0;
  int64_t e = kReleased;
  bool req = false;
  uint32_t flags = 0;
  if (valid) {
    w = ld.w;
    h = ld.h;
    s = sub_value(ld.raw);
    e = sub_released(ld.raw) ? kReleased : (ld.raw < 0 ? ld.xe : rs_cfg.follow_exp);
    flags = pub_flags(ld.b0);
    req = flags == 0u && ld.v.x > 0.0;  // count in [1, kSubMax] when the flags are clear
    rw = ld.v.x;
    rs = req ? (int)__double_as_longlong(ld.v.y) : 0;
  }
  const bool released = e == kReleased;
  bool live = valid && !released && !(p.now > e);          // present after Clean (store.go:174)
  const bool expired = valid && !released && (p.now > e);  // released by this round's Clean
  // a resource's lanes read each other's rows by shuffles; with one row there is no other
  auto sh_d = [&](double x, int q) { return ONE ? x : shfl_d(x, ln.base + q); };
  auto sh_i = [&](int x, int q) { return ONE ? x : shfl_i(x, ln.base + q); };
  auto any = [&](int x) { return ONE ? x != 0 : __any(x) != 0; };

  // Clean on the running sums, in row order (store.go:169-181 -> :142-151)
  long long count = rs_cfg.agg_count;
  double sh = rs_cfg.agg_has, sw = rs_cfg.agg_wants;
  const int xp = expired ? 1 : 0;
  if (any(xp)) {
    for (int q = 0; q < K; ++q) {
      const double hj = sh_d(h, q), wj = sh_d(w, q);
      const int sj = sh_i(s, q), xj = sh_i(xp, q);
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
    const int rq_q = sh_i(rq, q);
    if (!any(rq_q)) continue;  // no resource of this wave has server q's request
    const double rw_q = sh_d(rw, q);
    const int rs_q = sh_i(rs, q);
    const int live_q = sh_i(live ? 1 : 0, q);
    const double old_h = sh_d(h, q), old_w = sh_d(w, q);  // store.Get: zero when absent
    const int old_s = sh_i(s, q);
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
    if (any(loop1)) {
      // store.Map over the rows in row order (absent rows are not in the map)
      const int sl = live ? s : ~s;  // subclients + live bit (s >= 0)
      double x = 0.0, y = 0.0;
      long long wx = rs_q;  // FairShare wantExtra starts at the request's subclients (:148)
      for (int j = 0; j < K; ++j) {
        const double wj = sh_d(w, j);
        const int sj = sh_i(sl, j);
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
      if (any(loop2)) {
        double ee = 0.0;
        long long wee = rs_q;  // :189
        for (int j = 0; j < K; ++j) {
          const double wj = sh_d(w, j);
          const int sj = sh_i(sl, j);
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
  // The root store is written in place (out_* alias its columns, res its sums), so the words
  // this lane loaded (ld, as loaded: not w / h / s, which Clean zeroed) are the words it would
  // store over, and in a steady exchange most hold the round's result already.  A word is
  // stored only where its bits differ (bits, not ==: a -0.0 in memory gives way to a computed
  // +0.0, and a NaN equals itself); a word left alone stays clean in the cache, and the next
  // kernel's boundary has that much less to write back.  The aliasing is tested here, once and
  // uniformly, so that a caller without it stores everything; store_all (DM_ROUND_STORES=0)
  // does so too.  Nothing is remembered across launches.
  const bool keep = !ha.store_all && p.out_gets == p.has && p.out_wants == p.wants && p.out_sub == p.sub &&
                    p.out_expiry == p.expiry && p.res == p.agg;
  auto put_d = [&](double* at, double v, double had) {
    if (!keep || __double_as_longlong(v) != __double_as_longlong(had)) *at = v;
  };
  if (valid) {
    if (req) {
      const int32_t sub_new = (int32_t)((uint32_t)rs | kSubExplicit);
      put_d(p.out_gets + row, my_gets, ld.h);
      put_d(p.out_wants + row, rw, ld.w);
      if (!keep || sub_new != ld.raw) p.out_sub[row] = sub_new;
      if (!keep || exp_new != ld.xe) p.out_expiry[row] = exp_new;
    } else if (expired) {
      put_d(p.out_gets + row, 0.0, ld.h);
      put_d(p.out_wants + row, 0.0, ld.w);
      if (!keep || (int32_t)kSubReleased != ld.raw) p.out_sub[row] = (int32_t)kSubReleased;
      if (!keep || kReleased != ld.xe) p.out_expiry[row] = kReleased;
    }
  }
  if (valid && g0 == 0) {  // the resource's first lane
    // (load_res zeroes the sums it returns under recompute: then they are not the memory's)
    const bool same = keep && !p.recompute && count == rs_cfg.agg_count &&
                      __double_as_longlong(sh) == __double_as_longlong(rs_cfg.agg_has) &&
                      __double_as_longlong(sw) == __double_as_longlong(rs_cfg.agg_wants);
    if (!same) {  // (follow_exp is copied through: it never differs)
      ResAgg a;
      a.count = count;
      a.sum_has = sh;
      a.sum_wants = sw;
      a.follow_exp = rs_cfg.follow_exp;
      p.res[rr] = a;
    }
    if (!keep || rs_cfg.xstate != 1) p.expl[rr] = 1;  // the rows this tick writes carry explicit expiries
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

// The lane of root resource r in the one-server form.
__device__ __forceinline__ HierLane hier_lane_one(const HierArgs& ha, int64_t r) {
  HierLane ln;
  ln.rr = r;
  ln.row = r;
  ln.g0 = 0;
  ln.base = 0;
  ln.g = 0;
  ln.rec = r;
  ln.valid = true;
  ln.mine = ha.server == 0;
  return ln;
}

}  // namespace dm
