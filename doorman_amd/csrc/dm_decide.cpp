// dm_decide.cpp — dm_decide: the host side of a round of requests (dm_round.hip,
// dm_decide_fast.hip).
#include <unordered_map>

#include "dm_ctx.h"

// A round of requests, each decided by Resource.Decide in the caller's order and
// seeing the Assigns of the requests before it on the same resource
// (dm_round.hip).  Requests are ordered by resource on the host (stable: a
// resource's requests keep the caller's order); one workgroup per resource with
// requests, over a scratch copy of its rows.
int dm_decide(dm_ctx* c, int64_t now_ns, int64_t n, const int64_t* rows, const double* has, const double* wants,
              const int64_t* subclients, double* gets, int64_t* expiry_ns) {
  DM_ENTER(c);
  int rc = ready(c);
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!rows || !has || !wants || !subclients || !gets || !expiry_ns)))
    return c->fail(DM_E_INVAL, "bad requests");
  if (n == 0) return DM_OK;
  c->expl_rows = true;  // decided rows take explicit expiries
  c->rows_changed();
  std::vector<int64_t> seg_of((size_t)n);
  for (int64_t k = 0; k < n; ++k) {
    const int64_t r = rows[k];
    if (r < 0 || r >= c->N) return c->fail(DM_E_RANGE, "request row out of range");
    if (subclients[k] < 0 || subclients[k] > kSubMax) return c->fail(DM_E_INVAL, "subclients must be in [0, 2^31-2]");
    seg_of[(size_t)k] = std::upper_bound(c->h_seg_off.begin(), c->h_seg_off.end(), r) - c->h_seg_off.begin() - 1;
  }
  std::vector<int64_t> order((size_t)n);
  for (int64_t i = 0; i < n; ++i) order[(size_t)i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return seg_of[(size_t)a] < seg_of[(size_t)b]; });
  std::vector<int64_t> srows((size_t)n), ssub((size_t)n);
  std::vector<double> shas((size_t)n), swants((size_t)n);
  std::vector<ReqItem> items;
  int64_t scratch = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t k = order[(size_t)i], seg = seg_of[(size_t)k];
    srows[(size_t)i] = rows[k];
    shas[(size_t)i] = has[k];
    swants[(size_t)i] = wants[k];
    ssub[(size_t)i] = subclients[k];
    if (items.empty() || items.back().seg != (int32_t)seg) {
      items.push_back(ReqItem{(int32_t)seg, 0, i, i, scratch});
      scratch += c->h_seg_off[seg + 1] - c->h_seg_off[seg];
    }
    items.back().qhi = i + 1;
  }
  // Resources with many requests try the fast path (dm_decide_fast.hip): per request
  // the previous request of the round on the same row (its Assign is what the row
  // holds then), per resource its scan / sort areas.  The device decides whether the
  // round qualifies (FastRes::ok); k_decide takes every item it does not.
  std::vector<FastItem> fitems;
  std::vector<int64_t> prev;
  int64_t m_off = 0, e_off = 0, b_off = 0, c_off = 0;
  for (size_t ii = 0; c->decide_fast && ii < items.size(); ++ii) {
    ReqItem& itm = items[ii];
    const int64_t K = itm.qhi - itm.qlo;
    if (K < kFdMin) continue;
    if (prev.empty()) prev.assign((size_t)n, -1);
    FastItem f{};
    f.item = (int32_t)ii;
    f.k0 = itm.qlo;
    f.K = K;
    f.n = c->h_seg_off[itm.seg + 1] - c->h_seg_off[itm.seg];
    f.nblk = (int32_t)((K + kFdBlock - 1) / kFdBlock);
    f.m0 = m_off;
    f.e0 = e_off;
    f.b0 = b_off;
    f.c0 = c_off;
    f.nch = (int32_t)std::max<int64_t>(1, (f.n + kFdRows - 1) / kFdRows);
    m_off += f.n + 1;
    e_off += 2 * K;
    b_off += f.nblk;
    c_off += f.nch;
    itm.fast = (int32_t)fitems.size() + 1;
    fitems.push_back(f);
    std::unordered_map<int64_t, int64_t> last;
    last.reserve((size_t)(2 * K));
    for (int64_t k = itm.qlo; k < itm.qhi; ++k) {
      auto f2 = last.find(srows[(size_t)k]);
      if (f2 != last.end()) {
        prev[(size_t)k] = f2->second;
        fitems.back().repeats = 1;
      }
      last[srows[(size_t)k]] = k;
    }
  }
  hipStream_t st = c->stream;
  DM_HIP(c, upload(c->rq_rows, srows.data(), (size_t)n, st), "stage requests");
  DM_HIP(c, upload(c->rq_has, shas.data(), (size_t)n, st), "stage requests");
  DM_HIP(c, upload(c->rq_wants, swants.data(), (size_t)n, st), "stage requests");
  DM_HIP(c, upload(c->rq_sub, ssub.data(), (size_t)n, st), "stage requests");
  DM_HIP(c, upload(c->rq_items, items.data(), items.size(), st), "stage requests");
  DM_HIP(c, c->rq_gets.ensure((size_t)n), "request results");
  DM_HIP(c, c->rq_exp.ensure((size_t)n), "request results");
  DM_HIP(c, c->rq_sc_has.ensure((size_t)std::max<int64_t>(scratch, 1)), "request scratch");
  DM_HIP(c, c->rq_sc_wants.ensure((size_t)std::max<int64_t>(scratch, 1)), "request scratch");
  DM_HIP(c, c->rq_sc_sub.ensure((size_t)std::max<int64_t>(scratch, 1)), "request scratch");
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
  const int nfast = (int)fitems.size();
  FastArgs fa{};
  const int64_t *d_eb = nullptr, *d_ee = nullptr;
  int neb = 0;
  size_t need = 0, need2 = 0;
  if (nfast > 0) {
    DM_HIP(c, upload(c->fd_items, fitems.data(), fitems.size(), st), "fast path");
    DM_HIP(c, upload(c->fd_prev, prev.data(), prev.size(), st), "fast path");
    DM_HIP(c, c->fd_res.ensure((size_t)nfast), "fast path");
    DM_HIP(c, c->fd_pw.ensure((size_t)n), "fast path");
    DM_HIP(c, c->fd_v.ensure((size_t)n), "fast path");
    DM_HIP(c, c->fd_sc.ensure((size_t)n), "fast path");
    DM_HIP(c, c->fd_keys.ensure((size_t)m_off), "fast path");
    DM_HIP(c, c->fd_keys_s.ensure((size_t)m_off), "fast path");
    DM_HIP(c, c->fd_ps.ensure((size_t)m_off), "fast path");
    DM_HIP(c, c->fd_ev_in.ensure((size_t)e_off), "fast path");
    DM_HIP(c, c->fd_evs_in.ensure((size_t)e_off), "fast path");
    DM_HIP(c, c->fd_ev.ensure((size_t)e_off), "fast path");
    DM_HIP(c, c->fd_evs.ensure((size_t)e_off), "fast path");
    DM_HIP(c, c->fd_ecnt.ensure((size_t)(b_off * (2 * kFdBlock + 1))), "fast path");
    DM_HIP(c, c->fd_esum.ensure((size_t)(b_off * (2 * kFdBlock + 1))), "fast path");
    DM_HIP(c, c->fd_bdc.ensure((size_t)b_off), "fast path");
    DM_HIP(c, c->fd_bds.ensure((size_t)b_off), "fast path");
    DM_HIP(c, c->fd_pc.ensure((size_t)c_off), "fast path");
    DM_HIP(c, c->fd_pt.ensure((size_t)c_off), "fast path");
    DM_HIP(c, c->fd_ld.ensure((size_t)n), "fast path");
    int64_t most = 1;
    for (const FastItem& f : fitems) most = std::max(most, std::max(f.K, f.n + 1));
    DM_HIP(c, c->fd_part.ensure((size_t)((most + kFdChunk - 1) / kFdChunk)), "fast path");
    // segment bounds of the event blocks' sort
    std::vector<int64_t> eb, ee;
    for (const FastItem& f : fitems)
      for (int64_t b = 0; b < f.nblk; ++b) {
        eb.push_back(f.e0 + 2 * b * kFdBlock);
        ee.push_back(f.e0 + 2 * std::min<int64_t>(f.K, (b + 1) * kFdBlock));
      }
    neb = (int)eb.size();
    std::vector<int64_t> bounds(eb);
    bounds.insert(bounds.end(), ee.begin(), ee.end());
    DM_HIP(c, upload(c->fd_bounds, bounds.data(), bounds.size(), st), "fast path");
    d_eb = c->fd_bounds.p;
    d_ee = d_eb + eb.size();
    fa = FastArgs{c->fd_items.p, c->fd_res.p,    c->fd_prev.p, c->fd_pw.p,    c->fd_v.p,      c->fd_sc.p,
                  c->fd_keys.p,  c->fd_keys_s.p, c->fd_ps.p,   c->fd_ev_in.p, c->fd_evs_in.p, c->fd_ev.p,
                  c->fd_evs.p,   c->fd_ecnt.p,   c->fd_esum.p, c->fd_bdc.p,   c->fd_bds.p,    c->fd_pc.p,
                  c->fd_pt.p,    c->fd_ld.p};
    for (const FastItem& f : fitems) {
      size_t b1 = 0;
      DM_HIP(c, fd_sort_keys(nullptr, &b1, c->fd_keys.p + f.m0, c->fd_keys_s.p + f.m0, f.n, st), "fast path");
      need = std::max(need, b1);
    }
    DM_HIP(c, fd_sort_pairs(nullptr, &need2, c->fd_ev_in.p, c->fd_ev.p, c->fd_evs_in.p, c->fd_evs.p, e_off, neb, d_eb,
                            d_ee, st),
           "fast path");
    DM_HIP(c, c->fd_tmp.ensure(std::max<size_t>(std::max(need, need2), 1)), "fast path");
  }
  const ReqArgs q{c->rq_rows.p, c->rq_has.p,     c->rq_wants.p,    c->rq_sub.p,   c->rq_gets.p,
                  c->rq_exp.p,  c->rq_sc_has.p,  c->rq_sc_wants.p, c->rq_sc_sub.p, nfast ? c->fd_res.p : nullptr};
  // the device work of the round (one profiling class: dm_kernel_times "decide")
  auto launches = [&]() -> hipError_t {
    hipError_t e = hipSuccess;
    if (nfast > 0) {
      for (int s2 = 0; s2 < nfast; ++s2) {
        const FastItem& f = fitems[(size_t)s2];
        if ((e = fd_rows(p, items[(size_t)f.item], f, s2, q, fa, st)) != hipSuccess) return e;
        if ((e = fd_item(p, items[(size_t)f.item], f, s2, q, fa, c->fd_part.p, st)) != hipSuccess) return e;
        size_t t1 = c->fd_tmp.n;
        if ((e = fd_sort_keys(c->fd_tmp.p, &t1, c->fd_keys.p + f.m0, c->fd_keys_s.p + f.m0, f.n, st)) != hipSuccess)
          return e;
      }
      size_t t2 = c->fd_tmp.n;
      if ((e = fd_sort_pairs(c->fd_tmp.p, &t2, c->fd_ev_in.p, c->fd_ev.p, c->fd_evs_in.p, c->fd_evs.p, e_off, neb,
                             d_eb, d_ee, st)) != hipSuccess)
        return e;
      for (int s2 = 0; s2 < nfast; ++s2)
        if ((e = fd_item_sorted(p, items[(size_t)fitems[(size_t)s2].item], fitems[(size_t)s2], s2, q, fa,
                                c->fd_part.p, st)) != hipSuccess)
          return e;
    }
    return launch_decide(p, c->rq_items.p, (int)items.size(), q, st);
  };
  DM_HIP(c, c->timed(KC_DECIDE, st, launches), "decide requests");
  DM_HIP(c, download(shas.data(), (const double*)c->rq_gets.p, 0, n, st), "read decisions");
  DM_HIP(c, download(ssub.data(), (const int64_t*)c->rq_exp.p, 0, n, st), "read decisions");
  if (int rs = c->synced("decide requests")) return rs;
  for (int64_t i = 0; i < n; ++i) {
    gets[order[(size_t)i]] = shas[(size_t)i];
    expiry_ns[order[(size_t)i]] = ssub[(size_t)i];
  }
  return DM_OK;
}
