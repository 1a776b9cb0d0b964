// dm_decide_round.h — the device half of a round of requests as the host holds it: the one
// owner of the buffers dm_decide (dm_decide.cpp) stages a round into and its kernels
// (dm_round.hip, dm_decide_fast.hip) work in, kept from round to round and grown by whichever
// round needs most.  dm_decide_plan.h plans a round and says how many elements each buffer
// holds (plain C++, tested on the CPU); DecideRound applies the counts and names the buffers
// to the kernels (ReqArgs, FastArgs).
// Part of dm_ctx.h, which includes it below the buffer types it uses.
#pragma once

namespace dm {

struct DecideRound {
  bool fast = true;  // the fast path's switch (DM_DECIDE_FAST=0 turns it off; read by dm_create)
  // the members carry RoundBuf's names (dm_decide_plan.h): the requests in grouped order, their
  // results, the work items, the working copy of the requested resources' rows
  DBuf<int64_t> rows, sub, exp;
  DBuf<double> has, wants, gets;
  DBuf<ReqItem> items;
  DBuf<double> sc_has, sc_wants;
  DBuf<int32_t> sc_sub;
  // the fast path (what each holds: FastArgs, dm_device.h); the scans' partials, the pair
  // sort's segment bounds, the sorts' temporary storage
  DBuf<FastRes> res;
  DBuf<int64_t> prev, bounds;
  DBuf<double> pw, v, keys, keys_s, ev_in, ev;
  DBuf<FdScan> sc, ps, pt, part;
  DBuf<int32_t> evs_in, evs, ecnt, bdc;
  DBuf<double2> esum, bds;
  DBuf<FdClean> pc;
  DBuf<FdLind> ld;
  DBuf<uint8_t> tmp;

  // Every buffer at the plan's count, in RoundBuf's order.  A round without fast items asks 0
  // of the fast path's buffers, which leaves them as they are.
  hipError_t ensure(const RoundPlan& p) {
    using B = RoundBuf;
    hipError_t e = hipSuccess;
    auto need = [&](auto& buf, B id) {
      if (e == hipSuccess) e = buf.ensure((size_t)round_count(p, id));
    };
    need(rows, B::rows), need(has, B::has), need(wants, B::wants), need(sub, B::sub);
    need(gets, B::gets), need(exp, B::exp), need(items, B::items);
    need(sc_has, B::sc_has), need(sc_wants, B::sc_wants), need(sc_sub, B::sc_sub);
    need(res, B::res), need(prev, B::prev), need(pw, B::pw), need(v, B::v), need(sc, B::sc), need(ld, B::ld);
    need(keys, B::keys), need(keys_s, B::keys_s), need(ps, B::ps);
    need(ev_in, B::ev_in), need(evs_in, B::evs_in), need(ev, B::ev), need(evs, B::evs);
    need(ecnt, B::ecnt), need(esum, B::esum), need(bdc, B::bdc), need(bds, B::bds);
    need(pc, B::pc), need(pt, B::pt), need(part, B::part), need(bounds, B::bounds);
    return e;
  }

  ReqArgs req_args(const RoundPlan& p) const {
    ReqArgs q{};
    q.rows = rows.p, q.has = has.p, q.wants = wants.p, q.sub = sub.p;
    q.gets = gets.p, q.expiry = exp.p;
    q.sc_has = sc_has.p, q.sc_wants = sc_wants.p, q.sc_sub = sc_sub.p;
    q.fast = p.fast() ? res.p : nullptr;
    return q;
  }
  FastArgs fast_args() const {
    FastArgs a{};
    a.fr = res.p, a.prev = prev.p, a.pw = pw.p, a.v = v.p, a.sc = sc.p, a.ld = ld.p;
    a.keys = keys.p, a.keys_s = keys_s.p, a.ps = ps.p;
    a.ev_in = ev_in.p, a.evs_in = evs_in.p, a.ev = ev.p, a.evs = evs.p;
    a.ecnt = ecnt.p, a.esum = esum.p, a.bdc = bdc.p, a.bds = bds.p;
    a.pc = pc.p, a.pt = pt.p;
    return a;
  }

  // dm_decide_assign's buffers, which a round that ends with its Assign adds (dm_decide_assign.h
  // AssignBuf names them and assign_count sizes them; dm_decide itself never touches them): the
  // selection, the compact columns the upsert's row step reads in place, the requests' safe
  // capacities in grouped order.
  DBuf<int64_t> a_sel, a_rows, a_sub, a_exp;
  DBuf<double> a_has, a_wants, safe;
  hipError_t ensure_assign(const AssignSel& a) {
    using B = AssignBuf;
    hipError_t e = hipSuccess;
    auto need = [&](auto& buf, B id) {
      if (e == hipSuccess) e = buf.ensure((size_t)assign_count(a, id));
    };
    need(a_sel, B::sel), need(a_rows, B::rows), need(a_has, B::has), need(a_wants, B::wants);
    need(a_sub, B::sub), need(a_exp, B::exp), need(safe, B::safe);
    return e;
  }
  AssignArgs assign_args(const AssignSel& a) const {
    return AssignArgs{a.m(), a_sel.p, a_rows.p, a_has.p, a_wants.p, a_sub.p, a_exp.p};
  }

  // The round's two kinds of sort over the plan's areas: each fast item's wants (keys into
  // keys_s), and every event block as a segment of one pair sort (bounds: the begins, then the
  // ends).  temp null: the storage they need, into *bytes.
  hipError_t sort_keys(const FastItem& f, void* temp, size_t* bytes, hipStream_t st) const {
    return fd_sort_keys(temp, bytes, keys.p + f.m0, keys_s.p + f.m0, f.n, st);
  }
  hipError_t sort_events(const RoundPlan& p, void* temp, size_t* bytes, hipStream_t st) const {
    return fd_sort_pairs(temp, bytes, ev_in.p, ev.p, evs_in.p, evs.p, p.e, (int)p.b, bounds.p, bounds.p + p.b, st);
  }
  // The temporary storage at the most any sort of the round asks for (after ensure: the
  // queries are given the buffers' addresses).
  hipError_t ensure_sort(const RoundPlan& p, hipStream_t st) {
    if (!p.fast()) return hipSuccess;
    size_t most = 0, one = 0;
    hipError_t e = hipSuccess;
    for (const FastItem& f : p.fitems) {
      one = 0;
      if ((e = sort_keys(f, nullptr, &one, st)) != hipSuccess) return e;
      most = std::max(most, one);
    }
    one = 0;
    if ((e = sort_events(p, nullptr, &one, st)) != hipSuccess) return e;
    return tmp.ensure(std::max<size_t>(std::max(most, one), 1));
  }
};
static_assert(!std::is_copy_constructible<DecideRound>::value, "the round's buffers have one owner");

}  // namespace dm
