// The cases of tests/test_row_epoch.py: dm_row_epoch.h alone, one line per case,
//   <writer> mode=<0|1> keys=<0|1> -> defer=<0|1> build=<plain|keys> | ok=<end> nan=<end> rejected=<end> nan+rejected=<end>
// <end>: how the call ends for that outcome, "epoch" (rows_changed()) or "kept";
// then the sweep's grid hint after kept refreshes (dm_split_form.h FormInputs::refreshed):
//   list_grid told=<count> refreshed=<values> -> <grid> sweep=<0|1>
#include <cstdio>

#include "dm_row_epoch.h"
#include "dm_split_form.h"

using namespace dm;

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
  for (int mode = 0; mode < 2; ++mode)
    for (const auto& wr : writers)
      for (int keys = 0; keys < 2; ++keys) {
        const RowWriteStart s = row_write_start_mode(wr.w, mode, keys != 0);
        printf("%s mode=%d keys=%d -> defer=%d build=%s |", wr.name, mode, keys, s.defer, s.clear_keys ? "keys" : "plain");
        static const char* const outcome[4] = {"ok", "nan", "rejected", "nan+rejected"};
        for (int o = 0; o < 4; ++o)
          printf(" %s=%s", outcome[o], row_write_kept_mode(wr.w, mode, (o & 2) != 0, (o & 1) != 0) ? "kept" : "epoch");
        printf("\n");
      }
  // a part of 100,000 items with keys in use, whose sweep record is of this row epoch
  static const long long told_refreshed[][2] = {{0, 0}, {0, 100}, {8, 100}, {1000, 0}, {1000, 10000}, {0, 200000}};
  for (const auto& tr : told_refreshed) {
    FormInputs in;
    in.hints = in.dense_split = in.writeback = in.inplace = true;
    in.row_epoch = in.rec_epoch = in.fix_live = in.sw_epoch = 7;
    in.n = 100000;
    in.sw_told = tr[0];
    in.refreshed = tr[1];
    const PartForm f = choose_form(in, true);
    printf("list_grid told=%lld refreshed=%lld -> %d sweep=%d\n", tr[0], tr[1], f.list_grid, f.sweep);
  }
  return 0;
}
