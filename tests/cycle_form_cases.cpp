// The host rule of the cycle form (doorman_amd/csrc/dm_split_form.h, dm_large_form.h) on the
// CPU: every combination of choose_form's inputs checked against the rule as the header
// states it, then the sequences of cycle_auto_step; one line per case for
// tests/test_cycle_form.py.  Stand-alone: it may be built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>

#include "dm_large_form.h"
#include "dm_split_form.h"

using namespace dm;

static bool same_but_cycle(const PartForm& a, const PartForm& b) {
  return a.split == b.split && a.steady == b.steady && a.skip_rest == b.skip_rest && a.fixed == b.fixed &&
         a.use_keys == b.use_keys && a.sweep == b.sweep && a.rest_grid == b.rest_grid && a.list_grid == b.list_grid &&
         a.fix_live == b.fix_live;
}

#define CHECK(x)                                                      \
  do {                                                                \
    if (!(x)) {                                                       \
      std::printf("FAILED %s (line %d, case %ld)\n", #x, __LINE__, n); \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

// every input of choose_form that a rule mentions, 2^17 x 3 x 2 combinations
static void table() {
  long n = 0, cycles = 0, trusted = 0, parent_same = 0;
  for (unsigned m = 0; m < (1u << 17); ++m)
    for (int steady_ok = 0; steady_ok <= 2; ++steady_ok)
      for (int counts = 0; counts <= 1; ++counts) {
        auto bit = [m](int i) { return (m >> i & 1) != 0; };
        FormInputs in;
        in.hints = bit(0), in.dense_split = bit(1);
        const bool tried = bit(2);
        in.steady_ok = steady_ok;
        in.fixed_ok = bit(3), in.sweep_ok = bit(4);
        in.nparts = bit(5) ? 2 : 1;
        in.row_epoch = 7;
        in.rec_epoch = bit(6) ? 7 : 6;
        in.rec_counts = counts ? 3 : 0;
        in.recompute = bit(7), in.writeback = bit(8), in.inplace = bit(9);
        in.fix_live = bit(10) ? 7 : 5;
        in.cyc_live = bit(11) ? 7 : 5;
        in.keep_updates = bit(12), in.rec_kept = bit(13);
        in.cycle_ok = bit(14), in.cycle_want = bit(15);
        in.sw_epoch = bit(16) ? 7 : 0, in.sw_told = 8;
        in.n = 1000;
        ++n;
        const PartForm f = choose_form(in, tried);
        // the parent's answer: the same inputs with the cycle form's at their defaults
        FormInputs was = in;
        was.cycle_ok = true, was.cycle_want = false, was.cyc_live = 0;
        const PartForm p = choose_form(was, tried);
        CHECK(!p.cycle && p.cyc_live == 0);
        const bool may = in.cycle_ok && in.fixed_ok && in.cycle_want && in.writeback && !in.inplace;
        CHECK(f.cycle == (f.steady && may));
        CHECK(f.cyc_live == (f.cycle ? in.row_epoch : 0));  // every other launch ends the keys
        if (!in.cycle_ok || !in.cycle_want || in.inplace || !in.writeback || !in.fixed_ok) {
          CHECK(!f.cycle && same_but_cycle(f, p) && f.cyc_live == 0);  // DM_CYCLE=0, DM_WB_INPLACE: the parent's answers
          ++parent_same;
        }
        if (f.cycle) {
          ++cycles;
          CHECK(f.split && f.steady && !f.fixed && !f.sweep && !f.skip_rest && f.fix_live == 0);
          CHECK(!in.recompute && in.nparts == 1 && in.rec_epoch == in.row_epoch && in.steady_ok == 1);
          CHECK(f.use_keys == (in.cyc_live == in.row_epoch));  // never the FIXED build's fix_live
          trusted += f.use_keys;
        } else if (!same_but_cycle(f, p)) {
          // the one other difference: under DM_KEEP_UPDATES a few odd items do not keep a part
          // out of the steady builds on a tick that could run the cycle form
          CHECK(may && in.keep_updates && !f.steady);
        }
        if (f.fixed) CHECK(in.inplace && f.cyc_live == 0);
      }
  std::printf("table cases=%ld cycle=%ld trusted=%ld parent_same=%ld\n", n, cycles, trusted, parent_same);
}

static PartForm sweep_form() {
  PartForm f;
  f.split = f.steady = f.fixed = f.use_keys = f.sweep = true;
  return f;
}
static PartForm cycle_form() {
  PartForm f;
  f.split = f.steady = f.cycle = f.use_keys = true;
  return f;
}

// ticks until the part asks, from a fresh state, told the given count on every in-place sweep tick
static int ticks_to_engage(CycleAuto& a, const CycleAutoIn& in, int limit) {
  for (int t = 1; t <= limit; ++t)
    if (cycle_auto_step(a, in, sweep_form())) return t;
  return -1;
}

static void rule() {
  CycleAutoIn in;
  in.stream_store = true, in.row_epoch = 7, in.told_valid = true, in.told = 30600;
  {
    CycleAuto a;
    std::printf("engages_after %d\n", ticks_to_engage(a, in, 100));
    std::printf("engaged on=%d base=%ld\n", a.on, (long)a.base);
  }
  {
    CycleAuto a;
    CycleAutoIn x = in;
    x.told = 0;
    std::printf("empty_list %d\n", ticks_to_engage(a, x, 100));
    x = in, x.told_valid = false;
    std::printf("record_of_another_epoch %d\n", ticks_to_engage(a, x, 100));
    x = in, x.stream_store = false;
    std::printf("cache_resident_store %d\n", ticks_to_engage(a, x, 100));
    x = in, x.cycle_ok = false;
    std::printf("dm_cycle_0 %d\n", ticks_to_engage(a, x, 100));
  }
  {  // a list that kept refreshes fill does not count; items beyond their rows do
    CycleAuto a;
    CycleAutoIn x = in;
    x.told = 100, x.refreshed = 100;
    std::printf("refresh_driven_list %d\n", ticks_to_engage(a, x, 1000));
    CycleAuto b;
    x.told = 30600, x.refreshed = 1000;
    const int tb = ticks_to_engage(b, x, 1000);
    std::printf("persistent_beyond_refreshes %d recent=%ld\n", tb, (long)b.recent);
    CycleAuto c;
    x.told = 30600, x.refreshed = 10000;
    std::printf("refreshes_outweigh %d\n", ticks_to_engage(c, x, 1000));
  }
  {  // a tick that is no in-place sweep, or an empty list, starts the count over
    CycleAuto a;
    for (int t = 0; t < kCycleTrigger - 1; ++t) cycle_auto_step(a, in, sweep_form());
    cycle_auto_step(a, in, PartForm{});
    std::printf("interrupted_then %d\n", ticks_to_engage(a, in, 100));
  }
  {  // a new row epoch starts the count over, and ends an engaged part's ask
    CycleAuto a;
    for (int t = 0; t < kCycleTrigger - 1; ++t) cycle_auto_step(a, in, sweep_form());
    CycleAutoIn x = in;
    x.row_epoch = 8;
    std::printf("new_epoch_then %d\n", ticks_to_engage(a, x, 100));
    x.row_epoch = 9;
    std::printf("engaged_new_epoch on=%d\n", cycle_auto_step(a, x, cycle_form()));
  }
  {  // the judgement, by the count the device told with the stamp of the try's kCycleSettle-th tick
    for (long told : {0L, 15300L, 15301L, 30600L}) {
      CycleAuto a;
      ticks_to_engage(a, in, 100);
      CycleAutoIn x = in;
      x.told = told;
      int on = 1, t = 0;
      for (; t < 100 && on; ++t) {
        x.told_seq = a.seq;  // the device keeps up with the host
        on = cycle_auto_step(a, x, cycle_form());
      }
      std::printf("judged told=%ld stays=%d after=%d skip=%d wait=%d\n", told, on, on ? -1 : t, a.skip, a.wait);
    }
    CycleAuto a;  // the host runs ahead: no judgement before the device has told the settle-th tick
    ticks_to_engage(a, in, 100);
    CycleAutoIn x = in;
    for (int t = 0; t < 50; ++t) {
      x.told_seq = a.seq0 + (t < 3 ? t : 3);
      cycle_auto_step(a, x, cycle_form());
    }
    std::printf("device_behind on=%d judged=%d launches=%u\n", a.on, a.judged, a.seq - a.seq0);
    x.told_seq = a.seq0 + kCycleSettle, x.told = 0;
    cycle_auto_step(a, x, cycle_form());
    std::printf("device_caught_up on=%d judged=%d\n", a.on, a.judged);
    CycleAuto u;  // ticks that could not run the form carry no stamp, and kCycleIdle of them in a row end the try
    ticks_to_engage(u, in, 100);
    for (int t = 0; t < kCycleIdle - 1; ++t) cycle_auto_step(u, in, PartForm{});
    std::printf("idle_ticks on=%d judged=%d launches=%u idle=%d\n", u.on, u.judged, u.seq - u.seq0, u.idle);
    cycle_auto_step(u, in, cycle_form());  // (one tick that runs the form starts the count over)
    for (int t = 0; t < kCycleIdle - 1; ++t) cycle_auto_step(u, in, PartForm{});
    std::printf("idle_again on=%d idle=%d\n", u.on, u.idle);
    cycle_auto_step(u, in, PartForm{});
    std::printf("idle_gives_up on=%d skip=%d wait=%d\n", u.on, u.skip, u.wait);
    CycleAuto v;  // a second try: an in-place count (stamp 0) or the first try's stamp judges nothing
    ticks_to_engage(v, in, 100);
    CycleAutoIn y = in;
    for (int t = 0; t < 9; ++t) y.told_seq = v.seq, cycle_auto_step(v, y, cycle_form());
    const uint32_t stale = v.seq;
    ticks_to_engage(v, in, 100000);
    y.told_seq = 0;
    for (int t = 0; t < 20; ++t) cycle_auto_step(v, y, cycle_form());
    std::printf("second_try_stamp_0 on=%d judged=%d\n", v.on, v.judged);
    y.told_seq = stale - 1;
    for (int t = 0; t < 20; ++t) cycle_auto_step(v, y, cycle_form());
    std::printf("second_try_stale_stamp on=%d judged=%d\n", v.on, v.judged);
  }
  {  // the back-off: the waits between tries that do not help
    CycleAuto a;
    std::printf("backoff");
    for (int k = 0; k < 9; ++k) {
      const int t = ticks_to_engage(a, in, 100000);
      CycleAutoIn x = in;  // the count did not fall
      for (int s = 0; s <= kCycleSettle; ++s) x.told_seq = a.seq, cycle_auto_step(a, x, cycle_form());
      std::printf(" %d", t);
    }
    std::printf(" wait=%d\n", a.wait);
  }
}

static void column() {
  for (int m = 0; m < 16; ++m) {
    LargeInputs in;
    in.writeback = m & 1, in.inplace = (m & 2) != 0, in.recompute = (m & 4) != 0, in.cycle = (m & 8) != 0;
    LargeInputs was = in;
    was.cycle = false;
    const LargeForm f = choose_large(in), p = choose_large(was);
    const bool want = in.writeback && !in.inplace && in.cycle;
    if (f.pingpong != (p.pingpong || want) || f.spec != p.spec || f.n != p.n) {
      std::printf("FAILED column %d\n", m);
      std::exit(1);
    }
  }
  std::printf("column ok\n");
}

int main() {
  table();
  rule();
  column();
  return 0;
}
