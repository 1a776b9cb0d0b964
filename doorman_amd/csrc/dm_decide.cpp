// dm_decide.cpp — dm_decide and dm_decide_assign: the host side of a round of requests
// (dm_round.hip, dm_decide_fast.hip) and of the Assign that may end it (dm_decide_assign.hip).
// The round's plan is dm_decide_plan.h's, the Assign's selection dm_decide_assign.h's, their
// device buffers dm_decide_round.h's (dm_ctx::round); this unit carries the plan out.
#include "dm_ctx.h"

// The device work of a planned and staged round, in stream order: per fast item Clean, the
// verdict and the totals, the requests' deltas and their scan, the sort of its wants; every
// event block in one segmented sort; per fast item the structures over the sorted areas and
// the grants; then k_decide for every item the fast path did not take.
static hipError_t launch_round(const DecideRound& r, const RoundPlan& plan, const DevParams& p, const ReqArgs& q,
                               const FastArgs& fa, hipStream_t st) {
  const int nfast = (int)plan.fitems.size();
  hipError_t e = hipSuccess;
  for (int s = 0; s < nfast; ++s) {
    const FastItem& f = plan.fitems[(size_t)s];
    const ReqItem& it = plan.items[(size_t)f.item];
    if ((e = fd_rows(p, it, f, s, q, fa, st)) != hipSuccess) return e;
    if ((e = fd_item(p, it, f, s, q, fa, r.part.p, st)) != hipSuccess) return e;
    size_t bytes = r.tmp.n;
    if ((e = r.sort_keys(f, r.tmp.p, &bytes, st)) != hipSuccess) return e;
  }
  if (nfast > 0) {
    size_t bytes = r.tmp.n;
    if ((e = r.sort_events(plan, r.tmp.p, &bytes, st)) != hipSuccess) return e;
  }
  for (int s = 0; s < nfast; ++s) {
    const FastItem& f = plan.fitems[(size_t)s];
    if ((e = fd_item_sorted(p, plan.items[(size_t)f.item], f, s, q, fa, r.part.p, st)) != hipSuccess) return e;
  }
  return launch_decide(p, r.items.p, (int)plan.items.size(), q, st);
}

// A round of requests, each decided by Resource.Decide in the caller's order and
// seeing the Assigns of the requests before it on the same resource
// (dm_round.hip).  Requests are ordered by resource on the host (stable: a
// resource's requests keep the caller's order); one workgroup per resource with
// requests, over a scratch copy of its rows.
// One body with two endings.  dm_decide (assign false): the decisions cross PCIe, the host
// waits, the store is as it was.  dm_decide_assign: behind the round, on the context stream,
// the selected requests' values are gathered into the round's compact columns
// (dm_decide_assign.h, dm_decide_assign.hip) and assigned by the upsert's row step
// (dm_store_update.cpp upsert_round: dm_store_upsert_device's body), whose end carries the
// call's one wait; the safe capacities (when asked for) and the decisions' copies are
// enqueued before that wait and taken after it.
static int decide(dm_ctx* c, bool assign, int64_t now_ns, int64_t n, const int64_t* rows, const double* has,
                  const double* wants, const int64_t* subclients, double* gets, int64_t* expiry_ns, double* safe) {
  DM_ENTER(c);
  int rc = ready(c);
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!rows || !has || !wants || !subclients || !gets || !expiry_ns)))
    return c->fail(DM_E_INVAL, "bad requests");
  if (n == 0) return DM_OK;
  c->expl_rows = true;  // decided rows take explicit expiries
  c->rows_changed();
  DecideRound& r = c->round;
  const RoundPlan plan = plan_round(c->h_seg_off.data(), c->R, c->N, rows, subclients, n, r.fast, kSubMax);
  if (plan.error == RoundError::row_range) return c->fail(DM_E_RANGE, "request row out of range");
  if (plan.error == RoundError::subclients) return c->fail(DM_E_INVAL, "subclients must be in [0, 2^31-2]");
  // the requests' columns in the plan's order, and what the plan holds for the device
  std::vector<int64_t> srows((size_t)n), ssub((size_t)n);
  std::vector<double> shas((size_t)n), swants((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t k = plan.order[(size_t)i];
    srows[(size_t)i] = rows[k];
    shas[(size_t)i] = has[k];
    swants[(size_t)i] = wants[k];
    ssub[(size_t)i] = subclients[k];
  }
  hipStream_t st = c->stream;
  DM_HIP(c, upload(r.rows, srows.data(), (size_t)n, st), "stage requests");
  DM_HIP(c, upload(r.has, shas.data(), (size_t)n, st), "stage requests");
  DM_HIP(c, upload(r.wants, swants.data(), (size_t)n, st), "stage requests");
  DM_HIP(c, upload(r.sub, ssub.data(), (size_t)n, st), "stage requests");
  DM_HIP(c, upload(r.items, plan.items.data(), plan.items.size(), st), "stage requests");
  DM_HIP(c, r.ensure(plan), "request buffers");
  if (plan.fast()) {
    DM_HIP(c, upload(r.prev, plan.prev.data(), plan.prev.size(), st), "fast path");
    DM_HIP(c, upload(r.bounds, plan.bounds.data(), plan.bounds.size(), st), "fast path");
    DM_HIP(c, r.ensure_sort(plan, st), "fast path");
  }
  DevParams p{};
  p.seg_off = c->seg_off.p;
  p.wants = c->wants.p;
  p.has = c->has.p;
  p.sub = c->sub.p;
  p.expiry = c->expiry.p;
  p.cfg = c->cfg.p;
  p.agg = c->agg.p;
  p.expl = c->expl.p;
  p.now = now_ns;
  p.recompute = 0;
  const ReqArgs q = r.req_args(plan);
  const FastArgs fa = r.fast_args();
  // one profiling class: dm_kernel_times "decide"
  DM_HIP(c, c->timed(KC_DECIDE, st, [&] { return launch_round(r, plan, p, q, fa, st); }), "decide requests");
  // the decisions' copies into the staging vectors (their first use is over: the uploads above
  // are enqueued behind copies of their own), and their way into the caller's order
  auto read_decisions = [&]() -> hipError_t {
    const hipError_t e = download(shas.data(), (const double*)r.gets.p, 0, n, st);
    return e == hipSuccess ? download(ssub.data(), (const int64_t*)r.exp.p, 0, n, st) : e;
  };
  auto give_decisions = [&] {
    for (int64_t i = 0; i < n; ++i) {
      gets[plan.order[(size_t)i]] = shas[(size_t)i];
      expiry_ns[plan.order[(size_t)i]] = ssub[(size_t)i];
    }
  };
  if (!assign) {
    DM_HIP(c, read_decisions(), "read decisions");
    if (int rs = c->synced("decide requests")) return rs;
    give_decisions();
    return DM_OK;
  }
  const AssignSel a = assign_selection(plan, rows);
  DM_HIP(c, r.ensure_assign(a), "assign buffers");
  DM_HIP(c, upload(r.a_sel, a.sel.data(), a.sel.size(), st), "stage selection");
  DM_HIP(c, launch_assign_gather(q, r.assign_args(a), st), "gather assigns");
  std::vector<double> ssafe(safe ? (size_t)n : 0);
  UpsertTail tail;
  tail.enqueue = [&]() -> int {
    if (safe) {
      DM_HIP(c, launch_safe_capacity(n, r.rows.p, c->row_index(), c->cfg.p, c->cold.p, c->agg.p, r.safe.p, st),
             "safe capacity");
      DM_HIP(c, download(ssafe.data(), (const double*)r.safe.p, 0, n, st), "read safe capacity");
    }
    DM_HIP(c, read_decisions(), "read decisions");
    return DM_OK;
  };
  tail.landed = [&] {
    give_decisions();
    for (int64_t i = 0; safe && i < n; ++i) safe[plan.order[(size_t)i]] = ssafe[(size_t)i];
  };
  return upsert_round(c, a.m(), r.a_rows.p, r.a_has.p, r.a_wants.p, r.a_sub.p, r.a_exp.p, tail);
}

int dm_decide(dm_ctx* c, int64_t now_ns, int64_t n, const int64_t* rows, const double* has, const double* wants,
              const int64_t* subclients, double* gets, int64_t* expiry_ns) {
  return decide(c, false, now_ns, n, rows, has, wants, subclients, gets, expiry_ns, nullptr);
}

int dm_decide_assign(dm_ctx* c, int64_t now_ns, int64_t n, const int64_t* rows, const double* has, const double* wants,
                     const int64_t* subclients, double* gets, int64_t* expiry_ns, double* safe_capacity) {
  return decide(c, true, now_ns, n, rows, has, wants, subclients, gets, expiry_ns, safe_capacity);
}
