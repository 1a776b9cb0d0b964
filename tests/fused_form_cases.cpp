// The host rule of the fused form (doorman_amd/csrc/dm_split_form.h choose_form,
// PartForm::fused) on the CPU: every combination of the inputs a rule mentions checked against
// a transcription of the rule as the issue states it; one line per table for
// tests/test_fused_form.py.  Stand-alone: it may be built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>

#include "dm_split_form.h"

using namespace dm;

static bool same_but_fused(const PartForm& a, const PartForm& b) {
  return a.split == b.split && a.steady == b.steady && a.skip_rest == b.skip_rest && a.fixed == b.fixed &&
         a.use_keys == b.use_keys && a.sweep == b.sweep && a.rest_grid == b.rest_grid && a.list_grid == b.list_grid &&
         a.fix_live == b.fix_live && a.cycle == b.cycle && a.cyc_live == b.cyc_live && a.masked == b.masked;
}

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::printf("FAILED %s (line %d, case %ld)\n", #x, __LINE__, n); \
      std::exit(1);                                                    \
    }                                                                  \
  } while (0)

// 2^20 combinations x 3 values of DM_STEADY x 4 told counts around the threshold
static void table() {
  long n = 0, fused = 0, fused_cycle = 0, fused_sweep = 0;
  const int items = 1000;
  const int64_t limit = fused_limit(items);
  const int64_t told[4] = {0, limit - 1, limit, limit + 1};
  for (unsigned m = 0; m < (1u << 20); ++m)
    for (int steady_ok = 0; steady_ok <= 2; ++steady_ok)
      for (int k = 0; k < 4; ++k) {
        auto bit = [m](int i) { return (m >> i & 1) != 0; };
        FormInputs in;
        in.hints = bit(0), in.dense_split = bit(1);
        const bool tried = bit(2);
        in.steady_ok = steady_ok;
        in.fixed_ok = bit(3), in.sweep_ok = bit(4);
        in.nparts = bit(5) ? 2 : 1;
        in.row_epoch = 7;
        in.rec_epoch = bit(6) ? 7 : 6;
        in.rec_counts = bit(7) ? (1ull << 32) : 0;  // an item with a released row: masked under DM_KEEP_FREE_SLOTS
        in.recompute = bit(8), in.writeback = bit(9), in.inplace = bit(10);
        in.fix_live = bit(11) ? 7 : 5;
        in.cyc_live = bit(12) ? 7 : 5;
        in.keep_free = bit(13);
        in.cycle_ok = bit(14), in.cycle_want = bit(15);
        in.sw_epoch = bit(16) ? 7 : 3;
        in.sw_told = told[k];
        in.refreshed = bit(17) ? 1 : 0;
        in.n = items;
        in.fused_ok = bit(18);
        in.unjudged = bit(19);
        in.fused_max = limit;
        ++n;
        const PartForm f = choose_form(in, tried);
        // the parent's answer: the same inputs with the fused form's at their defaults
        FormInputs was = in;
        was.fused_ok = false, was.unjudged = false, was.fused_max = 0;
        const PartForm p = choose_form(was, tried);
        CHECK(!p.fused);
        CHECK(same_but_fused(f, p));  // fix_live / cyc_live and every launch's form are unchanged by the bit
        if (!in.fused_ok) CHECK(!f.fused);
        // the rule, transcribed
        const bool want = in.fused_ok && (p.sweep || (p.cycle && p.use_keys)) && !p.masked && !in.unjudged &&
                          in.sw_epoch == in.row_epoch && in.sw_told + in.refreshed <= limit;
        CHECK(f.fused == want);
        if (f.fused) {
          ++fused;
          fused_cycle += f.cycle;
          fused_sweep += f.sweep;
          CHECK(f.split && f.steady && f.use_keys && !f.masked && !in.unjudged && !f.skip_rest);
          CHECK(f.cycle != f.sweep);
          CHECK(f.cycle ? f.cyc_live == in.row_epoch && f.fix_live == 0 : f.fix_live == in.row_epoch && f.cyc_live == 0);
          CHECK(in.writeback && !in.recompute && in.nparts == 1 && in.steady_ok == 1);
        }
      }
  std::printf("table cases=%ld fused=%ld cycle=%ld sweep=%ld\n", n, fused, fused_cycle, fused_sweep);
}

static void defaults_and_limit() {
  long n = 0;
  // a default-constructed FormInputs never runs fused, whatever else holds
  FormInputs in;
  in.hints = in.dense_split = true;
  in.row_epoch = in.rec_epoch = in.fix_live = in.sw_epoch = 7;
  in.writeback = in.inplace = true;
  in.n = 1000;
  PartForm f = choose_form(in, true);
  CHECK(f.sweep && !f.fused);
  in.fused_ok = true;  // and with the bit alone the threshold is 0: only an empty list
  f = choose_form(in, true);
  CHECK(f.fused);
  in.sw_told = 1;
  CHECK(!choose_form(in, true).fused);
  in.fused_max = in.n;  // DM_FUSED=2: whatever the device told
  in.sw_told = in.n;
  CHECK(choose_form(in, true).fused);
  std::printf("limit %ld %ld %ld %ld %ld\n", (long)fused_limit(1), (long)fused_limit(799), (long)fused_limit(1000),
              (long)fused_limit(100000), (long)fused_limit(1 << 24));
}

int main() {
  table();
  defaults_and_limit();
  return 0;
}
