// dm_split_form.h — which launches one stream part of a workgroup bin (bins 3-6) runs this
// tick: the one decision behind Tick::bin_part (dm_tick.cpp), from what the host knows of
// the part (its split slot, dm_ctx.h SplitSlot) and of the tick.  Plain C++17, no HIP: the
// rules are tested on the CPU (tests/test_split_form.py).
//
// The forms, in the order the tests below admit them:
//   mixed           k_block over every item, hint or not
//   dense + rest    k_block_dense over the items whose hint is set, k_block_rest over the
//                   items it queued
//   dense alone     the rest launch skipped (skip_rest): every item verified dense in this
//                   row epoch, so nothing can be queued (the guard catches the impossible)
//   steady          k_block_dense's steady builds, then the rest launch
//   FIXED           the steady build of a writeback tick in place, rewriting every key ...
//   FIXED with keys ... or trusting them (use_keys) ...
//   the sweep       ... as k_sweep and k_block_list over its worklist
//   the cycle form  FIXED's twin for a steady writeback tick on the alternate column:
//                   the cycle builds of k_sweep and k_block_list (dm_device.h CycAux)
//   masked          any of the steady forms above, launched as the kernels' kMasked builds
//                   (dm_keep_keys' DM_KEEP_FREE_SLOTS: items that hold released rows are items
//                   of the form like any other)
//   fused           the sweep or the cycle form with keys in use, as one launch: k_block_fused
//                   (dm_tick_fused.hip) sweeps, and decides the few items the sweep would list
//                   or the row kernel queue itself; no row kernel, no rest launch
#pragma once
#include <algorithm>
#include <cstdint>

namespace dm {

struct PartForm {
  bool split = false;      // the split form (else the mixed kernel, and nothing below is set)
  bool steady = false;     // the steady builds
  bool skip_rest = false;  // no rest launch: the dense launch carries the guard and the tick's event
  bool fixed = false;      // the FIXED build
  bool use_keys = false;   // ... trusting the items' valid keys
  bool sweep = false;      // ... as the sweep and the row kernel over its worklist
  int rest_grid = 0;       // k_block_rest's workgroups
  int list_grid = 0;       // k_block_list's workgroups
  // The part's fix_live after this tick: the row epoch when the FIXED build is launched,
  // else 0 (the mixed kernel included).  This one assignment is the key rule: a key is
  // trusted only while nothing but FIXED launches touched the part in this row epoch.
  // Fixed points (dm_device.h FixKey, dm_tick_group.h group_segment kFixed): a part that
  // runs a steady build on a writeback tick in place runs the FIXED build, which keeps a
  // key per item and loads no row of an item whose valid key matches its capacity and
  // kind.  A valid key says that nothing but FIXED builds has touched the item's rows,
  // running sums or state since it was set; the device cannot know that, so the host
  // does: fix_live is the row epoch in which the part's last tick launched the FIXED
  // build (0: it did not).  Keys are in use for a launch only while that is the current
  // epoch; every other launch of the part (the mixed kernel, a plain or non-skipping
  // dense build, an alternate-column, non-writeback or recompute tick, DM_STEADY=2) and
  // every rows_changed() clears it, and the first FIXED launch after that ignores and
  // rewrites every key.
  uint64_t fix_live = 0;
  // The cycle form (with use_keys: trusting the keys' states, else rewriting every key) and
  // the part's cyc_live after this tick, under fix_live's discipline: the row epoch when the
  // cycle form is launched, else 0.  A key's states speak of both has columns, so nothing but
  // cycle-form launches may have touched the part: a non-writeback tick writes its gets into
  // the alternate column, an in-place tick leaves it behind, and so every other launch of
  // the part, like every rows_changed(), ends the keys.  A FIXED launch clears cyc_live and
  // a cycle-form launch fix_live: neither trusts the other's keys.
  bool cycle = false;
  uint64_t cyc_live = 0;
  // The steady form's launches are the masked builds (group_segment kMasked).  The choice never
  // affects results: a non-masked launch hands a masked item to the rest kernel, a masked
  // launch handles a non-masked item identically, and both maintain keys by the same rules,
  // so fix_live and cyc_live need no new discipline.
  bool masked = false;
  // The sweep (or the cycle form's) and what follows it as one launch, k_block_fused: chosen
  // only where keys are trusted (so fixed / sweep / cycle / use_keys, fix_live and cyc_live are
  // what they are without it: a fused launch is a FIXED or cycle-form launch for the key rule)
  // and the device last told of few listed items.  list_grid and rest_grid are then unused.
  bool fused = false;
};

// The most listed items (the sweep's worklist: row items and rest items) a part of n items may
// have been told of and still run fused.  A fused workgroup decides the listed items of its
// chunk one after another, where the row kernel spreads a list over the GPU at the price of two
// more launches.  Measured on the C3-shaped store of 100,000 items (tools/fused_ab.py,
// profiles/fused_ab.md; the tick's host time, fused against two-kernel): 15.3 against 19.3 us
// with nothing listed, 20.8 against 25.3 us with 10 items, 29.6 against 25.8 us with 100, 51.4
// against 31.4 us with 1,000.  Between 10 and 100 the two lines cross at about 59 items, a
// share of 5.9e-4; the threshold is half of that, a 3,400th of the part's items, so that a hint
// a few ticks stale still picks the cheaper form.  At least 4: the measured 10 win by 4.5 us.
constexpr int kFusedShareDenom = 3400;
inline int64_t fused_limit(int n) { return std::max<int64_t>(4, n / kFusedShareDenom); }

// The back-off of the split form.  The 128-thread bins split by the dense hint unless the
// last split tick the host has heard of queued more than a quarter of the part's items for
// k_block_rest; then the part runs the mixed kernel and tries again after `wait` ticks (64
// at first), doubling the wait after every try that still queued too many, up to 4096 (C2's
// bins, whose resources keep released rows, run 21 % slower split, and a try's k_block_rest
// strides over thousands of items).  Returns whether to try the split form this tick.
inline bool try_split(int64_t queued, int n, int& skip, int& wait) {
  const bool good = 4 * queued <= n;
  if (good) wait = 64;
  if (!good && ++skip < wait) return false;
  if (!good) wait = std::min(2 * wait, 4096);
  skip = 0;
  return true;
}

struct FormInputs {
  bool hints = false;        // the work items carry dense hints (only a writeback tick sets them)
  bool dense_split = false;  // the bin's bit of DM_DENSE_SPLIT
  int steady_ok = 1;         // DM_STEADY (2: the steady ticks' launches with the plain builds)
  bool fixed_ok = true;      // DM_FIXED
  bool sweep_ok = true;      // DM_SWEEP
  int nparts = 1;            // the bin's stream parts
  uint64_t row_epoch = 0;
  uint64_t rec_epoch = 0;    // the density record: the epoch of the part's last check ...
  uint64_t rec_counts = 0;   // ... low half: items not dense; high half: dense items with released rows or arrivals
  bool recompute = false, writeback = false;
  bool inplace = false;      // the gets go to the column the has came from
  uint64_t fix_live = 0;     // the part's, before this tick
  uint64_t sw_epoch = 0;     // the sweep record: the epoch of the count the device last told ...
  int64_t sw_told = 0;       // ... and the count
  uint32_t sw_stamp = 0;     // ... and, from the cycle form's row kernel, the stamp of the launch that told it
  int64_t refreshed = 0;     // kept refreshes' values and kept updates' rows since the last tick: each may have cleared a key
  int n = 0;                 // the part's items
  int64_t queued = 0;        // items the last split tick the host has heard of queued
  // dm_keep_keys' DM_KEEP_UPDATES (dm_row_epoch.h).  The defaults are every other context's.
  bool keep_updates = false;  // the bit is set
  bool rec_kept = false;      // the record is the host's copy from before a kept update: an estimate, no proof
  int64_t upd_rows = 0;       // rows kept updates wrote since the record's count
  // The cycle form.  The defaults give the answers choose_form gave without it.
  bool cycle_ok = true;     // DM_CYCLE
  bool cycle_want = false;  // the tick writes the alternate column for it: the caller's DM_WB_ALTERNATE, or a part asked (CycleAuto)
  uint64_t cyc_live = 0;    // the part's, before this tick
  // dm_keep_keys' DM_KEEP_FREE_SLOTS.  The defaults give the answers choose_form gave without it.
  bool keep_free = false;    // the bit is set
  int64_t rec_arrivals = 0;  // the density record's third count: dense items with an arrival bit
  // The fused form.  The defaults give the answers choose_form gave without it.
  bool fused_ok = false;    // DM_FUSED
  bool unjudged = false;    // the part asked for the alternate column and awaits its judgement (CycleAuto: on && !judged)
  int64_t fused_max = 0;    // fused_limit(n) (DM_FUSED=2, a measuring hook: no limit)
};

// `tried`: try_split's answer (asked only of a part with hints in a bin that splits).
inline PartForm choose_form(const FormInputs& in, bool tried) {
  PartForm f;
  f.split = in.hints && in.dense_split && tried;
  if (!f.split) return f;  // the mixed kernel keeps no key
  const bool verified = in.rec_epoch == in.row_epoch;
  // The steady builds: every item verified dense and none with released rows or arrivals
  // (the counts' high half), no recompute.  What the host cannot rule out is a lapse of
  // the followers (lease lengths change on the device), so the steady kernel queues such
  // an item and the rest kernel always follows it, with the tick's event; the guard is
  // for launches that queue nothing.
  // Not for a bin in stream parts: its ticks are short enough for the rest launch to
  // cost more than the pass saves (C1: kernel 33.7 -> 29.3 us, step 37.8 -> 39.6 us,
  // profiles/steady_ab.md).
  // With DM_KEEP_UPDATES the counts need not be zero for a tick that can run the FIXED
  // build (writeback in place): the steady kernels test every item themselves and queue what
  // is not dense or carries a mask bit, so a few such items cost a few items of the rest
  // launch, not the part its keys.  A few: the items not dense, those with mask bits and the
  // rows kept updates wrote since the count (each may have ended a dense state or set a bit)
  // are together at most a quarter of the part's items, try_split's bound for "too many for
  // the rest kernel".  Above it the part runs the forms it always ran.
  // With DM_KEEP_FREE_SLOTS an item that holds released rows is no odd one: the masked builds
  // decide it in the steady form and keep its key.  Odd are then the items not dense, those
  // with an arrival bit (the record's third count) and the rows kept updates wrote since; the
  // bound holds with or without DM_KEEP_UPDATES (a store with free slots and no updates is the
  // common case), and a record without an undense or arrival item is clean on any tick.
  const int64_t marked = in.keep_free ? in.rec_arrivals : (int64_t)(in.rec_counts >> 32);
  const int64_t odd = (int64_t)(uint32_t)in.rec_counts + marked + in.upd_rows;
  const bool cycle_tick = in.cycle_ok && in.fixed_ok && in.cycle_want && in.writeback && !in.inplace;
  const bool few = (in.keep_updates || in.keep_free) && in.writeback && (in.inplace || cycle_tick) && 4 * odd <= in.n;
  const bool none_odd = in.keep_free ? (uint32_t)in.rec_counts == 0 && in.rec_arrivals == 0 : in.rec_counts == 0;
  const bool clean = none_odd && !in.rec_kept;
  const bool steady_form = in.steady_ok && in.nparts == 1 && verified && (clean || few) && !in.recompute;
  f.steady = steady_form && in.steady_ok != 2;
  // The dense kernel alone takes the record as a proof that nothing can be queued, which a
  // copy from before a kept update is not: k_count_undense counts hint words, and an update
  // that ended a dense state left the hint word set and stale (the guard would mark the store
  // lost).  Not before a count taken after a later writeback tick.
  f.skip_rest = !steady_form && verified && !in.rec_kept && (uint32_t)in.rec_counts == 0;
  // The FIXED build: a steady build on a writeback tick in place.  It may trust the
  // items' keys when the part's last tick was one too, in this row epoch; otherwise it
  // rewrites every key and the next one may.
  f.fixed = f.steady && in.fixed_ok && in.writeback && in.inplace;
  f.use_keys = f.fixed && in.fix_live == in.row_epoch;
  f.fix_live = f.fixed ? in.row_epoch : 0;
  f.sweep = f.use_keys && in.sweep_ok;
  // The cycle form: the same steady conditions on a writeback tick that writes the alternate
  // column because the caller or a part asked for it (a tick that alternates for the large
  // chain's sake or after a write keeps the plain builds).
  f.cycle = f.steady && cycle_tick;
  if (f.cycle) f.use_keys = in.cyc_live == in.row_epoch;
  f.cyc_live = f.cycle ? in.row_epoch : 0;
  // The masked builds: only where the record, or its kept estimate, shows an item with a mask
  // bit (or a kept update may have set one since), so a store without free slots launches the
  // kernels it always launched.
  f.masked = f.steady && in.keep_free && ((in.rec_counts >> 32) != 0 || (in.rec_kept && in.upd_rows > 0));
  // Grids are hints: both kernels stride over their lists, so correctness never depends
  // on them.  The rest kernel's is sized from the last split tick's queue (an empty queue
  // costs 16 workgroups that read one count); the row kernel's from the count the device
  // last told in this row epoch (and the keys that kept refreshes and updates may have cleared since),
  // plus an eighth and 64 (the part's items until then).
  f.rest_grid = (int)std::min<int64_t>(512, std::max<int64_t>(16, in.queued));
  f.list_grid = in.n;
  if (in.sw_epoch == in.row_epoch) {
    const int64_t told = in.sw_told + in.refreshed;
    f.list_grid = (int)std::min<int64_t>(in.n, std::max<int64_t>(16, told + told / 8 + (told ? 64 : 0)));
  }
  // The fused form: keys are trusted (the first key-rewriting launch of an epoch lists every
  // item and stays the two-kernel form at full occupancy), no masked build, no judgement
  // pending (it needs the row kernel's stamp, which a fused launch does not tell), and the
  // sweep record is of this row epoch with few items listed, those that kept refreshes and
  // updates may have added since included.
  f.fused = in.fused_ok && (f.sweep || (f.cycle && f.use_keys)) && !f.masked && !in.unjudged &&
            in.sw_epoch == in.row_epoch && in.sw_told + in.refreshed <= in.fused_max;
  return f;
}

// When a part asks for the alternate column by itself.  A caller's DM_WB_ALTERNATE gets the
// cycle form wherever the steady conditions hold; without a flag only a store beyond the
// Infinity Cache (48 * N > kStreamBytes) ever leaves in-place FIXED, and only once in place
// has shown it is not enough: the part's in-place sweep has told the host a non-empty
// worklist on kCycleTrigger consecutive ticks of one row epoch (items that are never at a
// fixed point).  The part then asks, and a tick goes alternate if any part asks.  It is
// judged by the count of its kCycleSettle-th cycle-form tick (the first rewrites every key,
// the second proves).  The host enqueues ticks far ahead of the device, so a tick of its own
// count proves nothing about what the device has told: every cycle-form launch of an engaged
// part carries a stamp (seq) that the row kernel tells with its count, on every tick until
// the judgement, and the host judges when the told stamp has reached seq0 + kCycleSettle.
// It stays if that count fell to half of what it was when it engaged at most; otherwise it returns to in place and tries again after `wait`
// ticks, doubling from kCycleWait0 to kCycleWaitMax, as try_split does.  A new row epoch
// starts the count over (the keys are gone with it) and keeps the wait.  A store without
// persistent non-fixed items never gets here.
// Items that kept refreshes and updates put on the list do not count: a row written under
// dm_keep_keys clears its resource's key, which is back within a few ticks, and on such a store
// the alternate column only loses (it stores every run where in place skips the unchanged
// ones: profiles/cycle_ab.md).  A tick counts towards the trigger only when the told count
// exceeds `recent`, a running sum of the kept rows of about the last eight ticks.
// An engaged part whose ticks cannot run the form (it stopped being steady, or the caller
// keeps it in place) gets no stamp and so no judgement: after kCycleIdle such ticks in a row
// it gives the ask up as a failed try does, so that it does not keep every other part off
// in-place FIXED until the next row epoch.
// The told word's high half: a part back in place tells through k_block_list's in-place build, which
// writes no stamp and tells only a changed count, so the last cycle-form stamp may stay there
// under an in-place count.  It is harmless: only an engaged part reads it, against a seq0
// taken at or after that stamp, and kCycleSettle launches later at the earliest.
constexpr int kCycleTrigger = 8, kCycleSettle = 8, kCycleWait0 = 64, kCycleWaitMax = 4096, kCycleIdle = 16;
struct CycleAuto {
  bool on = false;  // the part asks for the alternate column
  int seen = 0;     // consecutive in-place sweep ticks with a non-empty list told
  uint32_t seq = 0, seq0 = 0;  // the part's cycle-form launches while engaged, ever, and when it last engaged
  bool judged = false;
  int idle = 0;  // consecutive ticks of an engaged part that could not run the form
  int64_t recent = 0;  // rows kept refreshes and updates wrote lately: recent := recent - recent / 8 + this tick's
  int skip = 0, wait = kCycleWait0;
  int64_t base = 0;  // the count told when it engaged
  uint64_t epoch = 0;
};
struct CycleAutoIn {
  bool cycle_ok = true;
  bool stream_store = false;  // 48 * N > kStreamBytes
  uint64_t row_epoch = 0;
  bool told_valid = false;  // the sweep record is of this row epoch
  int64_t told = 0;
  uint32_t told_seq = 0;  // the stamp told with it (0: an in-place sweep's count)
  int64_t refreshed = 0;  // FormInputs::refreshed: rows kept refreshes and updates wrote since the last tick
};
// Once per part and tick, after the form is chosen; returns whether the part asks.
inline bool cycle_auto_step(CycleAuto& a, const CycleAutoIn& in, const PartForm& f) {
  if (!in.cycle_ok || !in.stream_store) {
    a = CycleAuto{};
    return false;
  }
  a.recent = a.recent - a.recent / 8 + in.refreshed;
  if (a.epoch != in.row_epoch) {
    a.on = false;
    a.seen = 0;
    a.epoch = in.row_epoch;
  }
  if (!a.on) {
    if (a.skip > 0) {
      --a.skip;
      a.seen = 0;
      return false;
    }
    a.seen = (f.sweep && in.told_valid && in.told > a.recent) ? a.seen + 1 : 0;
    if (a.seen >= kCycleTrigger) {
      a.on = true;
      a.judged = false;
      a.seen = a.idle = 0;
      a.seq0 = a.seq;
      a.base = in.told;
    }
    return a.on;
  }
  if (f.cycle) ++a.seq;  // this launch's stamp (a tick that could not run the form has none)
  a.idle = f.cycle ? 0 : a.idle + 1;
  if (a.idle >= kCycleIdle) {
    a.on = false;
    a.skip = a.wait;
    a.wait = std::min(2 * a.wait, kCycleWaitMax);
    return false;
  }
  const uint32_t done = in.told_seq - a.seq0;  // cycle-form ticks of this try the device has told of
  if (!a.judged && in.told_valid && done >= (uint32_t)kCycleSettle && done < 0x80000000u) {
    a.judged = true;
    if (2 * in.told <= a.base) {
      a.wait = kCycleWait0;
    } else {
      a.on = false;
      a.skip = a.wait;
      a.wait = std::min(2 * a.wait, kCycleWaitMax);
    }
  }
  return a.on;
}

}  // namespace dm
