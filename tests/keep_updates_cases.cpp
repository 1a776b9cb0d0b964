// The cases of tests/test_keep_updates_rule.py: dm_row_epoch.h and dm_split_form.h alone.
// First one line per writer, dm_keep_keys mode (0-3) and keys in use, from the functions that
// take the mode's bits, in the format of tests/row_epoch_cases.cpp:
//   <writer> mode=<0-3> keys=<0|1> -> defer=<0|1> build=<plain|keys> | ok=<end> nan=<end> rejected=<end> nan+rejected=<end>
// then `legacy_same=<0|1>`: for modes 0 and 1 the rule the header held before dm_keep_keys took
// a bit set (legacy_start, legacy_kept below: a transcription) answers the same;
// then the form's choice with DM_KEEP_UPDATES, in the format of tests/split_form_cases.cpp:
//   <case> <split><steady><skip_rest><fixed><use_keys><sweep> rest=<grid> list=<grid> live=<fix_live>
#include <cstdio>

#include "dm_row_epoch.h"
#include "dm_split_form.h"

using namespace dm;

// dm_row_epoch.h's rule when dm_keep_keys was a boolean, as the header then held it
static RowWriteStart legacy_start(RowWrite w, bool keep_keys, bool keys_in_use) {
  RowWriteStart s;
  s.defer = keep_keys && is_refresh(w);
  s.clear_keys = s.defer && keys_in_use;
  return s;
}
static bool legacy_kept(RowWrite w, bool keep_keys, bool rejected, bool nan) {
  return keep_keys && is_refresh(w) && !rejected && !nan;
}

static FormInputs base() {  // split_form_cases.cpp's: 1000 items at their fixed point in row epoch 7, keys in use
  FormInputs in;
  in.hints = in.dense_split = true;
  in.row_epoch = in.rec_epoch = in.fix_live = in.sw_epoch = 7;
  in.writeback = in.inplace = true;
  in.n = 1000;
  return in;
}

static void show(const char* name, const FormInputs& in) {
  const PartForm f = choose_form(in, true);
  printf("%s %d%d%d%d%d%d rest=%d list=%d live=%llu\n", name, f.split, f.steady, f.skip_rest, f.fixed, f.use_keys,
         f.sweep, f.rest_grid, f.list_grid, (unsigned long long)f.fix_live);
}

template <typename F>
static void with(const char* name, F&& change) {
  FormInputs in = base();
  change(in);
  show(name, in);
}

// a kept update is pending: the record is the host's copy, `rows` written since its count
static void pending(FormInputs& in, uint64_t counts, int64_t rows) {
  in.keep_updates = true;
  in.rec_kept = true;
  in.rec_counts = counts;
  in.upd_rows = rows;
}

int main() {
  static const struct {
    RowWrite w;
    const char* name;
  } writers[] = {{RowWrite::refresh, "refresh"},     {RowWrite::refresh_mask, "refresh_mask"},
                 {RowWrite::load, "load"},           {RowWrite::plan, "plan"},
                 {RowWrite::upsert, "upsert"},       {RowWrite::release, "release"},
                 {RowWrite::apply, "apply"},         {RowWrite::apply_async, "apply_async"},
                 {RowWrite::decide, "decide"},       {RowWrite::clean, "clean"},
                 {RowWrite::relayout, "relayout"},   {RowWrite::config_load, "config_load"},
                 {RowWrite::root_tick, "root_tick"}};
  bool legacy_same = true;
  for (int mode = 0; mode < 4; ++mode)
    for (const auto& wr : writers)
      for (int keys = 0; keys < 2; ++keys) {
        const RowWriteStart s = row_write_start_mode(wr.w, mode, keys != 0);
        printf("%s mode=%d keys=%d -> defer=%d build=%s |", wr.name, mode, keys, s.defer, s.clear_keys ? "keys" : "plain");
        static const char* const outcome[4] = {"ok", "nan", "rejected", "nan+rejected"};
        if (mode < 2) {
          const RowWriteStart l = legacy_start(wr.w, mode != 0, keys != 0);
          legacy_same &= l.defer == s.defer && l.clear_keys == s.clear_keys;
        }
        for (int o = 0; o < 4; ++o) {
          const bool kept = row_write_kept_mode(wr.w, mode, (o & 2) != 0, (o & 1) != 0);
          if (mode < 2) legacy_same &= kept == legacy_kept(wr.w, mode != 0, (o & 2) != 0, (o & 1) != 0);
          printf(" %s=%s", outcome[o], kept ? "kept" : "epoch");
        }
        printf("\n");
      }
  printf("legacy_same=%d\n", legacy_same);

  // the added fields' defaults: what split_form_cases.cpp prints for these
  with("default_fixed_next_tick", [](FormInputs&) {});
  with("default_some_undense", [](FormInputs& in) { in.rec_counts = 3; });
  with("default_released_rows_only", [](FormInputs& in) { in.rec_counts = 5ull << 32; });
  with("default_two_parts", [](FormInputs& in) { in.nparts = 2; });
  // the counts alone do not relax anything without the bit, nor does the bit off the FIXED tick
  with("bit_clear_released_rows", [](FormInputs& in) { in.rec_counts = 5ull << 32; });
  with("bit_set_not_writeback", [](FormInputs& in) {
    in.keep_updates = true;
    in.rec_counts = 5ull << 32;
    in.writeback = false;
  });
  with("bit_set_alternate_column", [](FormInputs& in) {
    in.keep_updates = true;
    in.rec_counts = 5ull << 32;
    in.inplace = false;
  });
  with("bit_set_recompute", [](FormInputs& in) {
    in.keep_updates = true;
    in.rec_counts = 5ull << 32;
    in.recompute = true;
  });
  with("bit_set_steady_off", [](FormInputs& in) {
    in.keep_updates = true;
    in.rec_counts = 5ull << 32;
    in.steady_ok = 0;
  });

  // no update pending: a count with a few released-row items or items not dense keeps the part FIXED
  with("few_released_rows", [](FormInputs& in) {
    in.keep_updates = true;
    in.rec_counts = 5ull << 32;
  });
  with("few_undense", [](FormInputs& in) {
    in.keep_updates = true;
    in.rec_counts = 3;
  });

  // a kept update pending: fix_live and the keys' use survive it ...
  with("pending_one_row", [](FormInputs& in) { pending(in, 0, 1); });
  // ... not with the bit cleared since (the mode switched mid-run): dense + rest, no key kept
  with("pending_bit_cleared", [](FormInputs& in) {
    pending(in, 0, 1);
    in.keep_updates = false;
  });
  // ... and in stream parts the dense kernel does not run alone: dense + rest
  with("pending_two_parts", [](FormInputs& in) {
    pending(in, 0, 1);
    in.nparts = 2;
  });
  with("pending_record_of_older_epoch", [](FormInputs& in) {
    pending(in, 0, 1);
    in.rec_epoch = 6;
  });

  // the quarter bound: n / 4 of 1000 items, from each source and mixed, and one more
  with("quarter_undense_250", [](FormInputs& in) { pending(in, 250, 0); });
  with("quarter_undense_251", [](FormInputs& in) { pending(in, 251, 0); });
  with("quarter_masks_250", [](FormInputs& in) { pending(in, 250ull << 32, 0); });
  with("quarter_masks_251", [](FormInputs& in) { pending(in, 251ull << 32, 0); });
  with("quarter_rows_250", [](FormInputs& in) { pending(in, 0, 250); });
  with("quarter_rows_251", [](FormInputs& in) { pending(in, 0, 251); });
  with("quarter_mixed_250", [](FormInputs& in) { pending(in, 100 | 100ull << 32, 50); });
  with("quarter_mixed_251", [](FormInputs& in) { pending(in, 100 | 100ull << 32, 51); });
  with("quarter_live_record_251", [](FormInputs& in) {
    in.keep_updates = true;
    in.rec_counts = 251ull << 32;
  });

  // a pending update never yields skip_rest, whatever else holds
  int combos = 0, skips = 0;
  for (int bit = 0; bit < 2; ++bit)
    for (int nparts = 1; nparts <= 2; ++nparts)
      for (int steady = 0; steady <= 2; ++steady)
        for (int wb = 0; wb < 2; ++wb)
          for (int inplace = 0; inplace < 2; ++inplace)
            for (int recompute = 0; recompute < 2; ++recompute)
              for (uint64_t counts : {0ull, 3ull, 5ull << 32, 900ull})
                for (int64_t rows : {0, 1, 250, 251, 100000}) {
                  FormInputs in = base();
                  pending(in, counts, rows);
                  in.keep_updates = bit;
                  in.nparts = nparts;
                  in.steady_ok = steady;
                  in.writeback = wb;
                  in.inplace = inplace;
                  in.recompute = recompute;
                  ++combos;
                  skips += choose_form(in, true).skip_rest;
                }
  printf("pending_never_skip_rest combos=%d skip_rest=%d\n", combos, skips);

  // the grid hint: the rows of kept updates are in `refreshed` (dm_tick.cpp), added to the count told
  for (long long rows : {0, 100, 200000})
    for (long long told : {0, 8}) {
      FormInputs in = base();
      pending(in, 0, 1);
      in.n = 100000;
      in.sw_told = told;
      in.refreshed = rows;
      const PartForm f = choose_form(in, true);
      printf("list_grid told=%lld rows=%lld -> %d sweep=%d\n", told, rows, f.list_grid, f.sweep);
    }
  return 0;
}
