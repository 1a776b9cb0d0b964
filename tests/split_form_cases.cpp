// The cases of tests/test_split_form.py: dm_split_form.h alone, one line per case.
//   <case> mixed live=<fix_live>
//   <case> <split><steady><skip_rest><fixed><use_keys><sweep> rest=<grid> list=<grid> live=<fix_live>
#include <cstdio>

#include "dm_split_form.h"

using namespace dm;

static FormInputs base() {  // a part of 1000 items at its fixed point in row epoch 7, keys in use
  FormInputs in;
  in.hints = in.dense_split = true;
  in.row_epoch = in.rec_epoch = in.fix_live = in.sw_epoch = 7;
  in.writeback = in.inplace = true;
  in.n = 1000;
  return in;
}

static void show(const char* name, const FormInputs& in, bool tried = true) {
  const PartForm f = choose_form(in, tried);
  if (!f.split) {
    printf("%s mixed live=%llu\n", name, (unsigned long long)f.fix_live);
    return;
  }
  printf("%s %d%d%d%d%d%d rest=%d list=%d live=%llu\n", name, f.split, f.steady, f.skip_rest, f.fixed, f.use_keys,
         f.sweep, f.rest_grid, f.list_grid, (unsigned long long)f.fix_live);
}

template <typename F>
static void with(const char* name, F&& change, bool tried = true) {
  FormInputs in = base();
  change(in);
  show(name, in, tried);
}

int main() {
  // mixed
  with("no_hints", [](FormInputs& in) { in.hints = false; });
  with("split_bit_clear", [](FormInputs& in) { in.dense_split = false; });
  with("not_tried", [](FormInputs&) {}, false);

  // the back-off: 251 of 1000 items queued is too many, 250 is not
  int skip = 0, wait = 64, tick = 0;
  printf("backoff_tries");
  for (int tries = 0; tries < 9;) {
    ++tick;
    if (try_split(251, 1000, skip, wait)) {
      printf(" %d", tick);
      ++tries;
    }
  }
  printf(" wait=%d skip=%d\n", wait, skip);
  const bool good = try_split(250, 1000, skip, wait);
  printf("backoff_good_equal try=%d wait=%d skip=%d\n", good, wait, skip);
  for (tick = 1; !try_split(251, 1000, skip, wait); ++tick) {
  }
  printf("backoff_after_good next_try=%d wait=%d\n", tick, wait);

  // dense + rest, the rest skipped, steady
  with("not_verified", [](FormInputs& in) { in.rec_epoch = 6; });
  with("verified_some_undense", [](FormInputs& in) { in.rec_counts = 3; });
  with("verified_released_rows_only", [](FormInputs& in) { in.rec_counts = 5ull << 32; });
  with("verified_clean_two_parts", [](FormInputs& in) { in.nparts = 2; });
  with("verified_clean_steady_off", [](FormInputs& in) { in.steady_ok = 0; });
  with("verified_clean_steady_2", [](FormInputs& in) { in.steady_ok = 2; });
  with("verified_clean_recompute", [](FormInputs& in) { in.recompute = true; });

  // FIXED and the sweep
  with("steady_not_writeback", [](FormInputs& in) { in.writeback = false; });
  with("steady_alternate_column", [](FormInputs& in) { in.inplace = false; });
  with("steady_fixed_off", [](FormInputs& in) { in.fixed_ok = false; });
  with("fixed_keys_stale", [](FormInputs& in) { in.fix_live = 6; });
  with("fixed_keys_never", [](FormInputs& in) { in.fix_live = 0; });
  with("fixed_next_tick", [](FormInputs&) {});
  with("fixed_next_tick_sweep_off", [](FormInputs& in) { in.sweep_ok = false; });

  // grids
  for (int q : {0, 16, 17, 512, 513}) {
    char name[32];
    snprintf(name, sizeof name, "rest_grid_%d", q);
    with(name, [q](FormInputs& in) {
      in.n = 100000;
      in.queued = q;
    });
  }
  with("list_grid_stale_record", [](FormInputs& in) {
    in.n = 100000;
    in.sw_epoch = 6;
    in.sw_told = 5;
  });
  for (int told : {0, 8, 1000}) {
    char name[32];
    snprintf(name, sizeof name, "list_grid_told_%d", told);
    with(name, [told](FormInputs& in) {
      in.n = 100000;
      in.sw_told = told;
    });
  }
  with("list_grid_margin_beyond_n", [](FormInputs& in) { in.sw_told = 900; });
  return 0;
}
