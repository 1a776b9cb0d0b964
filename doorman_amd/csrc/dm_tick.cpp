// dm_tick.cpp — dm_apportion: one tick's launches over the plan's work classes and their
// streams (struct Tick), and what a tick does first: the readiness check, a pipelined
// leaf's staged templates, the queue calibration's windows.  Which stream waits for which
// is asked of dm_tick_order.h and carried out by the context's owners (dm_ctx.h StreamOrder,
// TickDone, TemplatePipe, QueueCalibration).
// A workgroup bin's stream part (Tick::bin_part) works on its split slot (dm_ctx.h
// SplitSlot): it reads the slot's host-mapped words, asks dm_split_form.h for the form of
// this tick's launches (try_split, choose_form: the one place the forms and the key rule
// are written), and hands the form to launch_fused, launch_dense_form, launch_rest or
// launch_mixed.
// The large-resource chain (Tick::large_chain) works on its owner (dm_large_chain.h
// LargeChain): Tick::outputs asks dm_large_form.h once for the tick's output column and the
// chain's form (choose_large), and large_chain launches the form's phases in order.
#include <ctime>

#include "dm_ctx.h"

int dm::ready(dm_ctx* c) {
  if (!c->store_loaded) return c->fail(DM_E_STATE, "no store loaded");
  if (int rc = c->check_device()) return rc;
  if (!c->cfg_loaded || (int64_t)c->h_refresh_s.size() != c->R)
    return c->fail(DM_E_STATE, "no configuration loaded for the store's resources");
  return DM_OK;
}

// Pipelined hierarchy (dm_hier_pipeline): before a leaf tick, take the templates of
// the exchanges enqueued before the previous tick (stream-ordered after their root
// kernels); the slot they replace becomes free once the ticks that read it are done.
static int commit_templates(dm_ctx* c) {
  TemplatePipe& tp = c->tpl;
  const int take = tp.q.take();
  if (take < 0) return DM_OK;
  const StreamOrder::XsTok& rt = tp.ready[take];
  const bool host_wait = rt.rec && rt.s && rt.s != c->stream;
  const TakeOrder o = take_templates(c->done.sig, host_wait);
  if (o.join) DM_HIP(c, c->order.join(), "join");
  if (host_wait) {
    // poll: the wake-up of a blocking wait comes too late for the next launch to be
    // queued in time.  Bounded by time (the exchange may wait on a slower rank's
    // all-gather): after 50 us of polling, a blocking wait frees the core.
    hipError_t q = hipEventQuery(c->order.xs_ev[rt.w]);
    if (q == hipErrorNotReady) {
      timespec t0{}, t1{};
      clock_gettime(CLOCK_MONOTONIC, &t0);
      do {
        q = hipEventQuery(c->order.xs_ev[rt.w]);
        clock_gettime(CLOCK_MONOTONIC, &t1);
      } while (q == hipErrorNotReady &&
               (t1.tv_sec - t0.tv_sec) * 1000000000LL + (t1.tv_nsec - t0.tv_nsec) < 50000);
    }
    if (q == hipErrorNotReady) q = hipEventSynchronize(c->order.xs_ev[rt.w]);
    if (q != hipSuccess) return c->hip_fail(q, "staged templates");
  } else {
    DM_HIP(c, c->order.xs_wait(rt, c->stream), "staged templates");
  }
  if (o.dirty) c->order.main_has_work();  // the class streams fork after the wait
  std::swap(c->cfg, tp.cfg[take]);
  std::swap(c->cold, tp.cold[take]);
  // the old templates (now in slot `take`) are free after the ticks enqueued so far: the
  // next exchange into it waits on the last tick's events (every stream part's) when its
  // last kernels complete them, else on a (lazy) event
  tp.free_seq[take] = o.free_seq;
  c->order.xs_signal_lazy(StreamOrder::XS_FREE0 + take, c->stream, &tp.free[take]);
  tp.free_rec[take] = true;
  tp.q.release(take);
  return DM_OK;
}

// The queue calibration (dm_tick_order.h QueueCalib says what each forked writeback tick
// does, before it forks).  Window boundaries join every class stream into the context
// stream (so the next window's assignment starts after the last one's work: a class's
// consecutive ticks on two streams are then still ordered) and record an event there.
static hipError_t calib_apply(dm_ctx* c, const QueueCalib::Perm& pm) {
  hipError_t e = c->order.join();
  if (e != hipSuccess) return e;
  for (int i = 0; i < kAux; ++i) {
    c->qcal.perm[i] = pm[(size_t)i];
    c->order.aux[i] = c->qcal.phys[pm[(size_t)i]];
  }
  c->order.main_has_work();  // the next tick forks: every class stream waits for the context stream
  return hipSuccess;
}

static hipError_t calib_mark(dm_ctx* c, bool end) {
  if (end) {
    hipEvent_t ev;
    hipError_t e = c->order.join();
    if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e == hipSuccess) e = hipEventRecord(ev, c->stream);
    if (e != hipSuccess) return e;
    c->qcal.ev.back().second = ev;
    c->order.main_has_work();
    return hipSuccess;
  }
  hipEvent_t ev;
  hipError_t e = hipEventCreate(&ev);
  if (e == hipSuccess) e = hipEventRecord(ev, c->stream);
  if (e != hipSuccess) return e;
  c->qcal.ev.push_back({ev, nullptr});
  return hipSuccess;
}

static hipError_t calib_step(dm_ctx* c) {
  using Action = QueueCalib::Action;
  QueueCalibration& qc = c->qcal;
  Action a = qc.cal.on_tick(c->order.aux_own_queue);
  hipError_t e = hipSuccess;
  if (a.kind == Action::start)  // the first window: the streams as they were created
    for (int i = 0; i < kAux; ++i) qc.phys[i] = c->order.aux[i];
  if (a.kind == Action::close_then_start || a.kind == Action::close_then_wait) e = calib_mark(c, true);
  if (a.kind == Action::poll) {  // the last window's end event done?  then every window's time
    e = hipEventQuery(qc.ev.back().second);
    if (e == hipErrorNotReady) return hipSuccess;
    std::vector<float> ms(qc.ev.size(), 0.0f);
    for (size_t w = 0; w < qc.ev.size() && e == hipSuccess; ++w)
      e = hipEventElapsedTime(&ms[w], qc.ev[w].first, qc.ev[w].second);
    if (e != hipSuccess) return e;
    a = qc.cal.on_times(ms);
    qc.free();
  }
  if (e != hipSuccess) return e;
  if (a.kind == Action::none || a.kind == Action::close_then_wait) return hipSuccess;
  e = calib_apply(c, a.perm);
  return e == hipSuccess && a.kind != Action::done ? calib_mark(c, false) : e;
}

// Once per row epoch, after a writeback tick of a workgroup bin's stream part (its split
// slot sl): count its items left without a dense hint (k_count_undense -> sl.rec).  A
// count of 0 lets the following ticks of the epoch skip the part's k_block_rest.
static hipError_t check_dense(dm_ctx* c, SplitSlot& sl, hipStream_t s) {
  const int64_t n = sl.items();
  // Again within the epoch after a kept wants refresh (dm_row_epoch.h) when the epoch's count
  // found items that are not dense: the refresh may have repaired the NaN that ended a
  // resource's dense state, and nothing else would count the part again before the next epoch
  // (tests/test_keep_keys_gpu.py::test_nan_and_rejection: the keys come back after the repair).
  // And again after the first writeback tick that follows a kept update (dm_ctx::update_kept),
  // which withdrew the record: this count, behind that tick on the part's stream, is the
  // first that may prove the part dense again.
  bool again = sl.recount;
  if (!again && sl.ver_epoch == c->row_epoch && sl.ver_write != c->write_epoch)
    again = __atomic_load_n(sl.rec.h + 1, __ATOMIC_ACQUIRE) == c->row_epoch &&
            (uint32_t)__atomic_load_n(sl.rec.h, __ATOMIC_RELAXED) != 0;
  if ((sl.ver_epoch == c->row_epoch && !again) || n <= 0) return hipSuccess;
  sl.ver_epoch = c->row_epoch;
  sl.ver_write = c->write_epoch;
  sl.recount = false;
  return launch_count_undense(c->bins[sl.b].p + sl.lo[0], (int)n, (unsigned long long*)sl.rec.d,
                              (unsigned long long)c->row_epoch, s);
}

namespace {
// One dm_apportion call: what its steps share, and the steps in the order they run.  Each
// step returns DM_OK or the failure dm_apportion returns (DM_HIP returns from the step).
struct Tick {
  dm_ctx* c;
  int64_t now_ns;
  uint32_t flags;
  bool wb = false, pingpong = false;
  bool cycle_want = false;  // the tick writes the alternate column for the cycle form's sake (FormInputs::cycle_want)
  DevParams p{};
  LargeForm lf;  // the output column and the chain's form (dm_large_form.h), chosen in outputs()
  hipStream_t st = nullptr, s_large = nullptr, s_small = nullptr;
  int nch = 0;
  int32_t *gl = nullptr, *gc = nullptr;  // k_general's worklist and its count
  bool general = false, fork = false, one_class = false;
  // A root round carried for this leaf (dm_carry_rule.h), when the tick's shape lets it ride:
  // bin_part places it once the part's form is chosen.
  dm_ctx* ride_root = nullptr;
  TickShape shape;

  template <typename F>
  hipError_t timed(int cls, hipStream_t s, F&& fn) {
    return c->timed(cls, s, fn);
  }
  hipStream_t cls_stream(int cls) const { return fork ? c->order.aux[c->class_stream[cls]] : st; }

  int outputs();      // the output columns and DevParams
  int streams();      // the worklist, the streams in use and the fork
  int large_chain();  // the large-resource chain
  int subs();         // the sub-wave launch
  int bins();         // the workgroup bins ...
  // ... and one stream part of one: what its launches share, the form's choice
  // (dm_split_form.h), then the form's launches
  struct Part {
    SplitSlot& sl;
    BinItems w;      // its items, in the launchers' shape
    hipStream_t s;
    DevParams p;     // the tick's, with the part's own flags word
    hipEvent_t done;  // the part's tick event, for its last kernel (null: no queue waits for the tick)
  };
  int bin_part(int b, int lb, int nparts, int j);
  // the sweep, its row kernel and the rest kernel as one launch; round: the root round it carries, or null
  int launch_fused(Part& pt, const PartForm& f, const RootRound* round);
  int launch_dense_form(Part& pt, const PartForm& f);  // the dense kernel in the form's build, or the sweep
  int launch_rest(Part& pt, const PartForm& f);        // the rest kernel over what it queued
  int launch_mixed(Part& pt);                          // the one-kernel form
  int finish();       // the join, the general kernel and the state updates
};

int Tick::outputs() {
  wb = flags & DM_WRITEBACK;
  p.seg_off = c->seg_off.p;
  p.wants = c->wants.p;
  p.has = c->has.p;
  p.sub = c->sub.p;
  p.expiry = c->expiry.p;
  p.cfg = c->cfg.p;
  p.agg = c->agg.p;
  p.expl = c->expl.p;
  p.rmask = c->rmask.p;
  // Every tick decides every row's lease (released rows included).  A writeback tick
  // writes its gets in place, into the has column, where the dense kernels skip the
  // gets store of every 64-row run the tick leaves unchanged (dm_tick_group.h
  // group_segment: a third of a quiescent resource's bytes).  It writes the alternate
  // column, which becomes the store's has after the tick, when the caller asks for it,
  // when it may take the speculative large chain (dm_large_form.h), and on a store beyond the
  // Infinity Cache whose rows a call has written since the last writeback tick (the row
  // epoch): such a tick has little to skip, and separate columns stream ~2 % faster than
  // reading and writing the same lines (C3 without the skip 427 against 435 us, C4's
  // kernel 616 against 630 us).  A cache-resident store (C1)
  // always preferred in place.  A store's ticks switch modes freely: after either kind
  // c->has is complete.
  if ((flags & DM_WB_INPLACE) && (flags & DM_WB_ALTERNATE))
    return c->fail(DM_E_INVAL, "DM_WB_INPLACE and DM_WB_ALTERNATE are exclusive");
  // (an asynchronous store batch still in flight may bring NaN wants or other subclient
  // counts: the tick is ready for k_general until the batch is retired)
  general = (c->maybe_general || c->async_may_general()) && c->n_nonsmall > 0;
  nch = (int)c->h_chunks.size();
  LargeChain& lc = c->chain;
  LargeInputs in;
  in.spec_chain = lc.spec_chain;
  in.writeback = wb;
  in.recompute = (flags & DM_AGG_RECOMPUTE) != 0;
  in.inplace = (flags & DM_WB_INPLACE) != 0;
  in.alternate = (flags & DM_WB_ALTERNATE) != 0;
  in.expl_rows = c->expl_rows;
  in.may_general = general;
  in.nchunks = nch;
  in.live_ok = lc.live_ok;
  in.stream_written = c->N * 48 > kStreamBytes && c->wb_epoch != c->row_epoch;
  in.redo_light = lc.redo_light;
  in.same_write_epoch = lc.redo_epoch == c->write_epoch;
  in.cycle = c->cycle_ok && c->cycle_asked();
  cycle_want = in.cycle || in.alternate;
  lf = choose_large(in);
  lc.live_ok = false;
  pingpong = lf.pingpong;
  if (wb) {
    c->wb_inplace = pingpong ? 0 : 1;  // dm_plan_info slot 19
    c->wb_epoch = c->row_epoch;
  }
  // A writeback tick writes no per-lease expiry: the leases it grants follow their
  // resource's expiry (dm_device.h), so only gets (and rare subclients words) move.
  if (!wb) {
    DM_HIP(c, c->out_gets.ensure((size_t)std::max<int64_t>(c->N, 1)), "alloc out_gets");
    DM_HIP(c, c->out_expiry.ensure((size_t)std::max<int64_t>(c->N, 1)), "alloc out_expiry");
    p.out_gets = c->out_gets.p;
    p.out_expiry = c->out_expiry.p;
  } else if (pingpong) {
    DM_HIP(c, c->out_gets.ensure((size_t)std::max<int64_t>(c->N, 1)), "alloc out_gets");
    p.out_gets = c->out_gets.p;
    p.out_expiry = nullptr;
  } else {
    p.out_gets = c->has.p;
    p.out_expiry = nullptr;
  }
  p.writeback = wb ? 1 : 0;
  if (wb) {
    p.out_wants = c->wants.p;
    p.out_sub = c->sub.p;
    p.res = c->agg.p;
  } else {
    DM_HIP(c, c->res.ensure((size_t)std::max<int64_t>(c->R, 1)), "alloc res");
    p.out_wants = nullptr;
    p.out_sub = nullptr;
    p.res = c->res.p;
  }
  p.now = now_ns;
  p.recompute = (flags & DM_AGG_RECOMPUTE) ? 1 : 0;
  if (wb && !c->pub_ring.empty()) {
    const int64_t n = (int64_t)c->pub_ring.size();
    p.pub = c->pub_ring[(size_t)(c->pub_k % n)];
    p.pub_clear = c->pub_ring[(size_t)((c->pub_k + 1) % n)];
    p.pub_word = -1;  // (a split bin's parts set their own)
    p.pub_first = 0;
    c->pub_k += 1;
  }
  return DM_OK;
}

int Tick::streams() {
  st = c->stream;
  gl = c->glist.p;
  gc = c->gcount.p;
  if (general) {  // only non-small resources are ever appended to the worklist
    DM_HIP(c, hipMemsetAsync(gc, 0, sizeof(int32_t), st), "worklist reset");
    c->order.main_has_work();
  }
  // Independent work classes: large resources (a 5-kernel chain), big groups,
  // small groups + packed.  With more than one class present they run on the
  // auxiliary streams concurrently, forked from and joined back to the main stream.
  unsigned used = 0;  // auxiliary streams with work this tick
  for (int b = 0; b < kNumBins; ++b)
    if (!c->h_bins[b].empty()) {
      used |= 1u << c->class_stream[b];
      if (c->bin_parts[b] > 1) used |= 1u << c->part_stream(b, 1);
    }
  if (!c->h_tiles.empty()) used |= 1u << c->class_stream[kNumBins];
  if (nch > 0) used |= 1u << c->class_stream[kNumBins + 1];
  fork = __builtin_popcount(used) > 1;
  int nonempty_bins = 0;
  for (int b = 0; b < kNumBins; ++b) nonempty_bins += c->h_bins[b].empty() ? 0 : 1;
  // one work class (on the context stream, or in stream parts): its split bin's last
  // kernel completes the tick's event (only check_dense's hint count may follow it)
  bool parts_only = false;
  for (int b = 0; b < kNumBins; ++b) parts_only |= !c->h_bins[b].empty() && c->bin_parts[b] > 1;
  one_class = (!fork || parts_only) && nch == 0 && c->h_tiles.empty() && !general && nonempty_bins == 1;
  if (fork && wb && !c->done.sig.wanted) DM_HIP(c, calib_step(c), "queue calibration");
  s_large = cls_stream(kNumBins + 1);
  s_small = cls_stream(kNumBins);
  if (!fork) {  // everything on the context stream, after any deferred class work
    DM_HIP(c, c->order.join(), "join");
    c->order.main_has_work();
  } else {  // class streams wait for what the context stream holds
    DM_HIP(c, c->order.fork(used), "fork");
  }
  return DM_OK;
}

int Tick::large_chain() {
  if (lf.n == 0) return DM_OK;
  LargeChain& lc = c->chain;
  const int nls = (int)c->h_large.size();
  LargeArgs a{c->chunks.p, c->large.p, lc.partials(), SpecArgs{}, gl, gc};
  // heterogeneous-subclient FairShare is decided on the chain when the store may
  // hold it (k_large_t, k_large_c_het, k_large_e, k_large_map_het)
  if (lf.het) DM_HIP(c, lc.with_het(a.P, nls, nch, s_large), "heterogeneous partials");
  a.P.b_first = lf.b_first ? 1 : 0;
  a.P.s_live = lf.s_live ? 1 : 0;
  // the steady state: one speculative launch, verified per resource, and a redo launch
  // that only the resources whose totals moved use
  if (lf.spec) {
    a.S = lc.spec_args(nch);
    if (lf.ask_seen && lc.take_seen()) lf.seen();
    lc.redo_epoch = c->write_epoch;
  }
  for (int i = 0; i < lf.n; ++i) {
    const LargePhase ph = lf.seq[i];
    DM_HIP(c, timed(kLargePhaseRows[(int)ph].cls, s_large,
                    [&] { return launch_large(ph, lc.grid(ph, nch, nls, lf.b_first), p, a, s_large); }),
           "large-resource kernels");
  }
  return DM_OK;
}

int Tick::subs() {
  // the sub-wave bins (8x2, 16x2, 16x4, 32x4, 64x4) in one launch on bin 0's stream
  SubBins sb{};
  int nonempty = 0;
  for (int k = 0; k < kSubShapes; ++k) {  // each sub-wave bin's items by shape (build_plan)
    const int b = kSubShapeBin[k], n = (int)c->h_shape_n[k];
    const int per = 256 / kSubShapeG[k];
    sb.items[k] = c->bins[b].p + c->h_shape_lo[k];
    sb.n[k] = n;
    sb.blocks[k] = (n + per - 1) / per;
    nonempty += n > 0;
  }
  if (nonempty > 0) {
    hipStream_t s = cls_stream(0);
    DM_HIP(c, timed(KC_SUBS, s, [&] { return launch_subs(p, sb, gl, gc, s); }), "sub-wave kernel");
  }
  return DM_OK;
}

int Tick::bin_part(int b, int lb, int nparts, int j) {
  SplitSlot& sl = c->slot(b, j);
  const int n = (int)sl.items();
  if (n == 0) return DM_OK;
  Part pt{sl, BinItems{lb, c->bins[b].p + sl.lo[0], n}, j == 0 ? cls_stream(b) : c->order.aux[c->part_stream(b, j)], p,
          nullptr};
  if (nparts > 1 && p.pub) {  // the part's own flags word (DevParams::pub_word)
    pt.p.pub_word = j;
    pt.p.pub_first = c->h_bins[b][(size_t)sl.lo[0]].seg;
  }
  // the tick's last kernel of this part (the dense kernel, or the rest kernel after
  // it) completes the part's tick event when another queue waits for the tick
  if (c->done.sig.carries(one_class)) {
    pt.done = c->done.event(j);
    c->done.sig.add_part(fork ? 1u << c->part_stream(b, j) : 0u);
  }
  // what the host knows of the part and of the tick -> the form of the part's launches
  FormInputs in;
  in.hints = c->hints_set;  // only a writeback tick sets hints, so the split form follows one
  in.dense_split = (c->dense_split >> (b - 3)) & 1;
  in.steady_ok = c->steady_ok;
  in.fixed_ok = c->fixed_ok;
  in.sweep_ok = c->sweep_ok;
  in.nparts = nparts;
  in.row_epoch = c->row_epoch;
  in.recompute = p.recompute;
  in.writeback = wb;
  in.inplace = pt.p.out_gets == pt.p.has;
  in.fix_live = sl.fix_live;
  in.cycle_ok = c->cycle_ok;
  in.cycle_want = cycle_want;
  in.cyc_live = sl.cyc_live;
  in.refreshed = c->kept_rows;
  in.keep_updates = (c->keep_mode & kKeepUpdates) != 0;
  in.keep_free = (c->keep_mode & kKeepFreeSlots) != 0;
  in.n = n;
  in.fused_ok = c->fused_ok != 0;
  in.unjudged = sl.cyc.on && !sl.cyc.judged;
  in.fused_max = c->fused_ok == 2 ? INT64_MAX / 2 : fused_limit(n);
  const bool may_split = in.hints && in.dense_split;
  if (may_split) in.queued = sl.read_queued();
  const bool tried = may_split && try_split(in.queued, n, sl.skip, sl.wait);
  if (tried) sl.read_records(in);
  const PartForm f = sl.last = choose_form(in, tried);
  sl.fix_live = f.fix_live;  // the key rule (SplitSlot::fix_live): every launch of the part passes here
  sl.cyc_live = f.cyc_live;
  // whether the part asks the next tick for the alternate column (only a tick without the
  // caller's column flags tells: with either the choice is the caller's)
  if (wb && !(flags & (DM_WB_INPLACE | DM_WB_ALTERNATE))) {
    CycleAutoIn ai;
    ai.cycle_ok = c->cycle_ok;
    ai.stream_store = c->N * 48 > c->cycle_bytes;
    ai.row_epoch = c->row_epoch;
    ai.told_valid = in.sw_epoch == c->row_epoch;
    ai.told = in.sw_told;
    ai.told_seq = in.sw_stamp;
    ai.refreshed = in.refreshed;
    cycle_auto_step(sl.cyc, ai, f);
  }
  int rc = DM_OK;
  const RootRound* round = nullptr;
  if (ride_root) {  // the carried round: in this part's one launch, or ahead of its launches
    if (place_round(shape, f.fused) == RoundPlace::ride) {
      round = &ride_root->carried_round;
    } else {
      if ((rc = launch_carried(ride_root))) return c->fail(rc, "carried root round: " + ride_root->err);
      ride_root = nullptr;
    }
  }
  if (f.fused)
    rc = launch_fused(pt, f, round);
  else if (!f.split)
    rc = launch_mixed(pt);
  else if (!(rc = launch_dense_form(pt, f)) && !f.skip_rest)
    rc = launch_rest(pt, f);
  if (rc) return rc;
  if (wb) DM_HIP(c, check_dense(c, sl, pt.s), "dense split check");
  return DM_OK;
}

// The fused form tells the host its listed count through the word the row kernel tells through
// (SplitSlot::sweep), and each of the two writes only what differs from what it last told
// itself.  So when the form changes, the kernel that takes over must not take its own last
// word for the host's: a fused launch after another form is told so (FusedArgs::fresh), and
// the first row kernel after a fused launch finds its last-told words cleared (a change of
// form is rare; a steady part pays nothing).  The rest items have a host word of their own
// (SplitSlot::fused_queued), read in place of `queued` until the next split launch.
int Tick::launch_fused(Part& pt, const PartForm& f, const RootRound* round) {
  SplitSlot& sl = pt.sl;
  if (!sl.fu_cnt.p) {
    DM_HIP(c, sl.fu_cnt.ensure(8), "fused count");  // k_block_fused has the layout
    DM_HIP(c, hipMemsetAsync(sl.fu_cnt.p, 0, 8 * sizeof(int32_t), pt.s), "fused count");
    sl.fpar = 0;
  }
  const FusedArgs a{sl.keys(), f.cycle ? sl.aux() : nullptr, sl.fu_cnt.p, sl.fpar, !sl.ran_fused,
                    (unsigned long long*)sl.sweep.d, (unsigned long long)c->row_epoch, sl.fused_queued.d, gl, gc};
  DM_HIP(c, timed(KC_DENSE3 + (sl.b - 3), pt.s, [&] { return launch_bin_fused(pt.w, pt.p, a, round, pt.done, pt.s); }),
         "group kernel (fused)");
  if (round) {  // the round ran in the launch
    ride_root->carried = false;
    ride_root->rounds_in_tick += 1;
    c->rounds_in_tick += 1;
    ride_root = nullptr;
  }
  sl.fpar ^= 1;
  sl.ran_fused = true;
  return DM_OK;
}

int Tick::launch_dense_form(Part& pt, const PartForm& f) {
  SplitSlot& sl = pt.sl;
  if (sl.ran_fused) {  // (launch_fused has the account)
    if (sl.sw_cnt.p) DM_HIP(c, hipMemsetAsync(sl.sw_cnt.p + 2, 0xFF, 2 * sizeof(int32_t), pt.s), "sweep count");
    sl.ran_fused = false;
  }
  // the guard and the tick's event go to a dense launch that no rest launch follows
  const SplitArgs a{sl.queue.p, sl.qcnt.p, sl.qpar, gl, gc, f.skip_rest ? sl.guard.d : nullptr};
  FixKey* keys = f.fixed || f.cycle ? sl.keys() : nullptr;
  if (f.sweep || f.cycle) {
    DM_HIP(c, sl.sw_list.ensure((size_t)pt.w.n), "sweep list");
    if (!sl.sw_cnt.p) {
      DM_HIP(c, sl.sw_cnt.ensure(4), "sweep count");  // two-slot count + the last {count, epoch} told the host
      DM_HIP(c, hipMemsetAsync(sl.sw_cnt.p, 0, 4 * sizeof(int32_t), pt.s), "sweep count");
      sl.lpar = 0;
    }
  }
  DM_HIP(c, timed(KC_DENSE3 + (sl.b - 3), pt.s, [&] {
           const SweepArgs sw{keys, sl.sw_list.p, sl.sw_cnt.p, sl.lpar, (unsigned long long*)sl.sweep.d,
                              (unsigned long long)c->row_epoch, f.list_grid};
           const unsigned stamp = sl.cyc.on ? sl.cyc.seq : 0u;
           const bool tell = sl.cyc.on && !sl.cyc.judged;
           if (f.cycle) return launch_bin_cycle(pt.w, pt.p, a, sw, f.masked, sl.aux(), f.use_keys, stamp, tell, pt.s);
           if (f.sweep) return launch_bin_sweep(pt.w, pt.p, a, sw, f.masked, pt.s);
           return launch_bin_dense(pt.w, pt.p, a, f.skip_rest ? pt.done : nullptr, f.steady, f.masked, keys, f.use_keys,
                                   pt.s);
         }),
         "group kernel (dense split)");
  if (f.sweep || f.cycle) sl.lpar ^= 1;
  return DM_OK;
}

int Tick::launch_rest(Part& pt, const PartForm& f) {
  SplitSlot& sl = pt.sl;
  const SplitArgs a{sl.queue.p, sl.qcnt.p, sl.qpar, gl, gc, nullptr};
  DM_HIP(c, timed(KC_REST3 + (sl.b - 3), pt.s,
                  [&] { return launch_bin_rest(pt.w, pt.p, a, sl.queued.d, f.rest_grid, pt.done, pt.s); }),
         "group kernel (dense split)");
  sl.qpar ^= 1;
  return DM_OK;
}

int Tick::launch_mixed(Part& pt) {
  if (pt.done) c->done.sig.unflag();  // (a tick in the one-kernel form carries no event: consumers join instead)
  DM_HIP(c, timed(KC_BIN0 + pt.sl.b, pt.s, [&] { return launch_bin(pt.w, pt.p, gl, gc, pt.s); }), "group kernel");
  return DM_OK;
}

int Tick::bins() {
  for (SplitSlot& s : c->split) s.last = PartForm{};  // (dm_plan_info: the forms of this tick's launches)
  for (int b = kNumBins - 1; b >= 0; --b) {
    if (c->h_bins[b].empty()) continue;
    if (!dm_ctx::is_split_bin(b)) continue;  // the sub-wave bins: k_subs
    const int lb = (b == 6 && c->bin6_wide)   ? kBin6Wide
                   : (b == 4 && c->bin4_wave) ? kBin4Wave
                                              : b;  // the launchers' bin (shape)
    const int nparts = c->bin_parts[b];
    c->done.sig.flag(one_class, nparts);
    for (int j = 0; j < nparts; ++j)
      if (int rc = bin_part(b, lb, nparts, j)) return rc;
  }
  c->kept_rows = c->kept_upd_rows = 0;  // (every part's sweep is sized: FormInputs::refreshed)
  return DM_OK;
}

int Tick::finish() {
  if (!c->h_tiles.empty())
    DM_HIP(c, timed(KC_SMALL, s_small, [&] { return launch_tile_small(p, c->tiles.p, c->tile_list.p, (int)c->h_tiles.size(), s_small); }),
           "small kernel");
  if (fork) {
    c->order.forked();
    // k_general consumes every class's worklist appends on the context stream
    const bool defer = (flags & DM_ASYNC) && (flags & DM_DEFER_JOIN) && !general;
    if (!defer) DM_HIP(c, c->order.join(), "join");
  }
  if (general) {
    const int blocks = (int)std::min<int64_t>(c->n_nonsmall, 1024);
    DM_HIP(c, timed(KC_GENERAL, st, [&] { return launch_general(p, gl, gc, blocks, st); }), "general kernel");
    c->order.main_has_work();
  }
  if (pingpong) std::swap(c->has, c->out_gets);  // the written column becomes the store's (stream order)
  c->last_writeback = wb;
  c->have_result = true;
  if (wb) c->hints_set = true;
  if (wb) c->expl_rows = false;
  c->chain.live_ok = lf.leaves_live;
  if (!(flags & DM_ASYNC)) {
    const int rc = c->synced("tick");
    c->collect_profile();
    return rc;
  }
  return DM_OK;
}

}  // namespace

int dm_apportion(dm_ctx* c, int64_t now_ns, uint32_t flags) {
  DM_CHECK_CTX(c);
  int rc = ready(c);
  if (rc) return rc;
  if (c->tpl.on && (rc = commit_templates(c))) return rc;
  c->tpl.q.tick();
  c->done.sig.begin();
  Tick t{c, now_ns, flags};
  // A round carried for this leaf is still here only under dm_hier_step's hold (every other
  // entry launched it): it rides if the tick can only be one launch of a workgroup bin over
  // every resource, else it runs ahead of the tick's launches, where it ran before.
  if (dm_ctx* root = c->carry_root; root && root->carried) {
    TickShape& sh = t.shape;
    sh.work_classes = (c->h_tiles.empty() ? 0 : 1) + (c->h_chunks.empty() ? 0 : 1);
    sh.split_bin = false;
    for (int b = 0; b < kNumBins; ++b) {
      if (c->h_bins[b].empty()) continue;
      sh.work_classes += 1;
      sh.split_bin = dm_ctx::is_split_bin(b);
      sh.parts = c->bin_parts[b];
      sh.items = (int64_t)c->h_bins[b].size();
    }
    sh.general = (c->maybe_general || c->async_may_general()) && c->n_nonsmall > 0;
    sh.writeback = (flags & DM_WRITEBACK) != 0;
    sh.resources = c->R;
    if (may_ride(sh) && root->stream == c->stream) {
      t.ride_root = root;
    } else if ((rc = launch_carried(root))) {
      return c->fail(rc, "carried root round: " + root->err);
    }
  }
  if ((rc = t.outputs()) || (rc = t.streams()) || (rc = t.large_chain()) || (rc = t.subs()) ||
      (rc = t.bins()))
    return rc;
  return t.finish();
}
