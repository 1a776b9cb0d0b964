// The cases of tests/test_free_slots_form.py: dm_split_form.h alone, one line per case.
#include <cstdio>
#include <cstring>

#include "dm_split_form.h"

using namespace dm;

static bool same(const PartForm& a, const PartForm& b) {
  return a.split == b.split && a.steady == b.steady && a.skip_rest == b.skip_rest && a.fixed == b.fixed &&
         a.use_keys == b.use_keys && a.sweep == b.sweep && a.rest_grid == b.rest_grid && a.list_grid == b.list_grid &&
         a.fix_live == b.fix_live && a.cycle == b.cycle && a.cyc_live == b.cyc_live && a.masked == b.masked;
}

static void show(const char* name, const PartForm& f) {
  std::printf("%s %d%d%d%d%d%d cycle=%d masked=%d live=%llu cyc=%llu\n", name, f.split, f.steady, f.skip_rest, f.fixed,
              f.use_keys, f.sweep, f.cycle, f.masked, (unsigned long long)f.fix_live, (unsigned long long)f.cyc_live);
}

// a part of 1000 items, verified in row epoch 7, every item with a mask bit, keys in use
static FormInputs base() {
  FormInputs in;
  in.hints = in.dense_split = true;
  in.row_epoch = in.rec_epoch = in.fix_live = 7;
  in.rec_counts = 1000ull << 32;
  in.writeback = in.inplace = true;
  in.n = 1000;
  in.keep_free = true;
  return in;
}

int main() {
  // the bit clear: the new fields change nothing, whatever the arrival count says
  long cases = 0, differ = 0, masked = 0;
  const uint64_t counts[] = {0, 1, 250, 251, 1ull << 32, 250ull << 32, 251ull << 32, (100ull << 32) | 100};
  for (uint64_t rc : counts)
    for (int bits = 0; bits < 1 << 11; ++bits)
      for (int so = 0; so < 3; ++so)
        for (int64_t upd : {0, 10, 300}) {
          FormInputs in;
          in.hints = bits & 1, in.dense_split = bits & 2, in.fixed_ok = bits & 4, in.sweep_ok = bits & 8;
          in.nparts = bits & 16 ? 2 : 1;
          in.recompute = bits & 32, in.writeback = bits & 64, in.inplace = bits & 128;
          in.keep_updates = bits & 256, in.rec_kept = bits & 512, in.cycle_want = bits & 1024;
          in.steady_ok = so;
          in.row_epoch = in.rec_epoch = in.fix_live = in.cyc_live = 7;
          in.rec_counts = rc;
          in.upd_rows = upd;
          in.n = 1000;
          const PartForm a = choose_form(in, true);
          in.rec_arrivals = 123;
          const PartForm b = choose_form(in, true);
          ++cases;
          differ += same(a, b) ? 0 : 1;
          masked += a.masked || b.masked;
        }
  std::printf("bit_clear cases=%ld differ=%ld masked=%ld\n", cases, differ, masked);

  FormInputs in = base();
  show("all_masked_inplace", choose_form(in, true));
  in.sweep_ok = false;
  show("all_masked_sweep_off", choose_form(in, true));
  in = base();
  in.fix_live = 0;
  show("all_masked_keys_stale", choose_form(in, true));
  in = base();
  in.inplace = false, in.cycle_want = true, in.cyc_live = 7;
  show("all_masked_cycle", choose_form(in, true));
  in.cyc_live = 0;
  show("all_masked_cycle_first", choose_form(in, true));
  in = base();
  in.writeback = false;
  show("all_masked_not_writeback", choose_form(in, true));
  in = base();
  in.inplace = false;
  show("all_masked_alternate_unasked", choose_form(in, true));
  in = base();
  in.keep_free = false;
  show("bit_clear_all_masked", choose_form(in, true));
  in.keep_updates = true;
  show("bit_clear_keep_updates", choose_form(in, true));

  // the quarter bound counts arrivals, undense items and kept updates' rows
  in = base();
  in.rec_arrivals = 250;
  show("arrivals_250", choose_form(in, true));
  in.rec_arrivals = 251;
  show("arrivals_251", choose_form(in, true));
  in = base();
  in.rec_counts |= 250;
  show("undense_250", choose_form(in, true));
  in.rec_counts += 1;
  show("undense_251", choose_form(in, true));
  in = base();
  in.rec_arrivals = 100, in.rec_counts |= 100, in.keep_updates = true, in.rec_kept = true, in.upd_rows = 50;
  show("mixed_250", choose_form(in, true));
  in.upd_rows = 51;
  show("mixed_251", choose_form(in, true));
  in = base();
  in.rec_arrivals = 1, in.writeback = false;
  show("arrival_not_writeback", choose_form(in, true));

  // no mask bit in the record: today's kernels
  in = base();
  in.rec_counts = 0;
  show("no_mask_bit", choose_form(in, true));
  in.rec_counts = 5;
  show("no_mask_bit_5_undense", choose_form(in, true));
  in = base();
  in.rec_counts = 0, in.keep_updates = true, in.rec_kept = true, in.upd_rows = 3;
  show("kept_estimate_after_updates", choose_form(in, true));

  // what keeps the steady forms off keeps the masked builds off
  in = base();
  in.recompute = true;
  show("recompute", choose_form(in, true));
  in = base();
  in.nparts = 2;
  show("two_parts", choose_form(in, true));
  in = base();
  in.steady_ok = 0;
  show("steady_off", choose_form(in, true));
  in = base();
  in.steady_ok = 2;
  show("steady_2", choose_form(in, true));
  in = base();
  in.rec_epoch = 6;
  show("not_verified", choose_form(in, true));
  in = base();
  show("not_tried", choose_form(in, false));
  return 0;
}
