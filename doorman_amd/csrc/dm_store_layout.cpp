// dm_store_layout.cpp — a loaded store re-laid out in HBM (dm_store_relayout) and Clean on the
// device (dm_store_clean, dm_read_cleaned).  Neither stages columns: both wait for the batches
// in flight (dm_store_update.cpp async_retire_all), then work on the store's own columns.
#include "dm_ctx.h"

// The store re-laid out in HBM (dm_relayout.hip): fresh columns take every row that
// stays, the kernels flag what the new layout cannot hold, and the fresh columns become
// the store's only when nothing was flagged -- a rejected call leaves the old columns,
// index, sums and plan as they were.  What crosses PCIe: the new seg_off, two flag words
// and, when asked for, the row map.
int dm_store_relayout(dm_ctx* c, int64_t n_resources, const int64_t* new_seg_off, uint32_t flags, int64_t* row_map) {
  DM_ENTER(c);
  if (!c->store_loaded) return c->fail(DM_E_STATE, "no store loaded");
  (void)c->check_device();
  if (c->store_lost)
    return c->fail(DM_E_STATE, "the store is lost (" + c->lost_msg + "): reload it (dm_store_load), a re-layout would carry its rows over");
  // in-flight batches name rows of the old layout: they finish first, and a rejected one's
  // error is returned before anything moves (as dm_config_load)
  if (int ra = async_retire_all(c)) return ra;
  const int64_t R = c->R, N = c->N, Rn = n_resources;
  if (!new_seg_off || (flags & ~DM_RELAYOUT_COMPACT)) return c->fail(DM_E_INVAL, "bad re-layout arguments");
  if (Rn < R) return c->fail(DM_E_INVAL, "a re-layout keeps every resource: n_resources below the store's count");
  if (Rn > INT32_MAX - 1) return c->fail(DM_E_INVAL, "too many resources for one context (max 2^31-2)");
  if (new_seg_off[0] != 0) return c->fail(DM_E_INVAL, "new_seg_off must start at 0");
  for (int64_t r = 0; r < Rn; ++r)
    if (new_seg_off[r + 1] < new_seg_off[r]) return c->fail(DM_E_INVAL, "new_seg_off must be non-decreasing");
  if (Rn != R && (!c->pub_ring.empty() || c->hs_leaf))
    return c->fail(DM_E_STATE, "a publish ring or hierarchy pair is bound to this store (blocks of 1 + R records): "
                               "the number of resources cannot change");
  const int64_t Nn = new_seg_off[Rn];
  const bool compact = flags & DM_RELAYOUT_COMPACT;
  DM_HIP(c, hipStreamSynchronize(c->stream), "sync");
  hipStream_t st = c->stream;
  DBuf<int64_t> n_off, n_exp;
  DBuf<int32_t> n_blk, n_sub;
  DBuf<double> n_wants, n_has;
  DBuf<ResAgg> n_agg;
  DBuf<uint8_t> n_expl;
  // (a failure waits for what the stream still holds before the fresh columns go with the return)
#define RL_HIP(expr, what)                 \
  do {                                     \
    const hipError_t _e = (expr);          \
    if (_e != hipSuccess) {                \
      (void)hipStreamSynchronize(st);      \
      return c->hip_fail(_e, what);        \
    }                                      \
  } while (0)
  RL_HIP(upload(n_off, new_seg_off, (size_t)Rn + 1, st), "upload seg_off");
  RL_HIP(n_blk.ensure((size_t)((Nn >> kRowBlkShift) + 2)), "alloc row index");
  RL_HIP(n_wants.ensure((size_t)Nn), "alloc wants");
  RL_HIP(n_has.ensure((size_t)Nn), "alloc has");
  RL_HIP(n_sub.ensure((size_t)Nn), "alloc subclients");
  RL_HIP(n_exp.ensure((size_t)Nn), "alloc expiry");
  RL_HIP(n_agg.ensure((size_t)Rn), "alloc running sums");
  RL_HIP(n_expl.ensure((size_t)std::max<int64_t>(Rn, 1)), "alloc explicit flags");
  RL_HIP(hipMemsetAsync(n_expl.p, 1, n_expl.n, st), "explicit flags");  // every row leaves with an expiry of its own
  RL_HIP(c->rl_flags.ensure(1), "re-layout flags");
  RL_HIP(c->rl_bad.ensure(1), "re-layout flags");
  const int64_t nb = (N + kRlBlkRows - 1) / kRlBlkRows;
  if (compact) {
    RL_HIP(c->rl_blk_pre.ensure((size_t)nb + 1), "block prefix");
    RL_HIP(c->rl_seg_local.ensure((size_t)std::max<int64_t>(R, 1)), "resource bases");
  }
  if (row_map && N > 0) RL_HIP(c->rl_map.ensure((size_t)N), "row map");
  RelayoutArgs a{};
  a.N = N;
  a.R = R;
  a.ix = c->row_index();
  a.wants = c->wants.p;
  a.has = c->has.p;
  a.sub = c->sub.p;
  a.expiry = c->expiry.p;
  a.agg = c->agg.p;
  a.Nn = Nn;
  a.Rn = Rn;
  a.new_off = n_off.p;
  a.n_wants = n_wants.p;
  a.n_has = n_has.p;
  a.n_sub = n_sub.p;
  a.n_expiry = n_exp.p;
  a.blk_pre = compact ? c->rl_blk_pre.p : nullptr;
  a.seg_local = compact ? c->rl_seg_local.p : nullptr;
  a.row_map = row_map && N > 0 ? c->rl_map.p : nullptr;
  a.flags = c->rl_flags.p;
  a.bad = c->rl_bad.p;
  RL_HIP(launch_relayout(a, n_blk.p, n_agg.p, compact, st), "re-layout");
  uint32_t f = 0;
  unsigned long long bad = 0;
  RL_HIP(hipMemcpyAsync(&f, c->rl_flags.p, sizeof f, hipMemcpyDeviceToHost, st), "re-layout flags");
  RL_HIP(hipMemcpyAsync(&bad, c->rl_bad.p, sizeof bad, hipMemcpyDeviceToHost, st), "re-layout flags");
  RL_HIP(hipStreamSynchronize(st), "re-layout");
  if (f & kRlReject) {
    char buf[160];
    if (f & kRlInternal) {
      snprintf(buf, sizeof buf, "re-layout: inconsistent ranks at resource %llu", bad);
      return c->fail(DM_E_INTERNAL, buf);
    }
    if (f & kRlDrop)
      snprintf(buf, sizeof buf, "resource %llu: the new segment would drop a row that is not released", bad);
    else
      snprintf(buf, sizeof buf, "resource %llu: more live rows than its new segment holds", bad);
    return c->fail(DM_E_RANGE, buf);
  }
  if (row_map && N > 0) {
    RL_HIP(hipMemcpyAsync(row_map, c->rl_map.p, (size_t)N * sizeof(int64_t), hipMemcpyDeviceToHost, st), "row map");
    RL_HIP(hipStreamSynchronize(st), "row map");
  }
#undef RL_HIP
  // the fresh table becomes the store; the old one is freed when the call returns
  std::swap(c->seg_off, n_off);
  std::swap(c->blk_seg, n_blk);
  std::swap(c->wants, n_wants);
  std::swap(c->has, n_has);
  std::swap(c->sub, n_sub);
  std::swap(c->expiry, n_exp);
  std::swap(c->agg, n_agg);
  std::swap(c->expl, n_expl);
  if (Nn != N) {  // the alternate columns and lease outputs follow N at the next tick that needs them
    c->out_gets.release();
    c->out_expiry.release();
  }
  c->R = Rn;
  c->N = Nn;
  c->h_seg_off.assign(new_seg_off, new_seg_off + Rn + 1);
  c->seg_uniform = uniform_rows(new_seg_off, Rn);
  // maybe_general / all_sub_one are carried: no live row was added.  One case the rows
  // themselves decide (kRlGeneral): a resource of the small tiles, which the load's scan
  // never looked at, now in a bin that hands heterogeneous rows to k_general.
  if (f & kRlGeneral) c->maybe_general = true;
  build_plan(c);
  if (int rc = upload_plan(c)) return rc;  // (with R unchanged: bin 4's shape by the kept kinds, update_bin4_shape)
  DM_HIP(c, hipStreamSynchronize(st), "re-layout");
  c->expl_rows = true;
  c->rows_changed();
  c->have_result = false;
  c->hints_set = false;
  c->cl_valid = false;  // the last clean's list named rows of the old layout
  if (Rn != R) c->cfg_loaded = false;  // the caller loads a configuration for the new count
  return DM_OK;
}

// Clean (store.go:169-181) on the device (dm_clean.hip): a count pass, the 16-B result to
// the host (which sizes the list from it), then the apply pass.  What crosses PCIe: that
// result, and 8 B per listed row when dm_read_cleaned asks for them.
int dm_store_clean(dm_ctx* c, int64_t now_ns, uint32_t flags, dm_clean_result* out) {
  DM_ENTER(c);
  DM_STORE_OK(c);
  if (flags & ~DM_CLEAN_PEEK) return c->fail(DM_E_INVAL, "unknown clean flags");
  if (!c->store_loaded) return c->fail(DM_E_STATE, "no store loaded");
  // in-flight batches change which rows are live: they finish first, and a rejected one's
  // error is returned before anything is cleaned (as dm_config_load)
  if (int ra = async_retire_all(c)) return ra;
  const bool peek = flags & DM_CLEAN_PEEK;
  hipStream_t st = c->stream;
  const int64_t nb = (c->N + kRlBlkRows - 1) / kRlBlkRows;
  c->cl_valid = false;
  c->cl_n = 0;
  int64_t res[2] = {0, DM_NO_EXPIRY};
  CleanArgs a{};
  if (nb > 0) {
    DM_HIP(c, c->cl_blk_pre.ensure((size_t)nb + 2), "clean block prefix");
    DM_HIP(c, c->cl_blk_min.ensure((size_t)nb), "clean block minima");
    a.N = c->N;
    a.ix = c->row_index();
    a.has = c->has.p;
    a.wants = c->wants.p;
    a.sub = c->sub.p;
    a.expiry = c->expiry.p;
    a.agg = c->agg.p;
    a.expl = c->expl.p;
    a.now = now_ns;
    a.blk_pre = c->cl_blk_pre.p;
    a.blk_min = c->cl_blk_min.p;
    DM_HIP(c, c->timed(KC_RELEASE, st, [&] { return launch_clean_count(a, st); }), "clean count");
    DM_HIP(c, hipMemcpyAsync(res, c->cl_blk_pre.p + nb, sizeof res, hipMemcpyDeviceToHost, st), "clean result");
    if (int rs = c->synced("clean")) return rs;
  }
  const int64_t total = res[0];
  if (total < 0 || total > c->N) return c->fail(DM_E_INTERNAL, "clean: inconsistent count of lapsed rows");
  if (total > 0) {
    DM_HIP(c, c->cl_list.ensure((size_t)total), "clean list");
    a.list = c->cl_list.p;
    a.list_n = total;
    if (!peek) c->rows_changed();
    DM_HIP(c, c->timed(KC_RELEASE, st, [&] { return launch_clean_apply(a, c->dense_upd(), peek, st); }),
           "clean apply");
    if (!peek) c->have_result = false;
    if (int rs = c->synced("clean")) return rs;
  }
  c->cl_valid = true;
  c->cl_n = total;
  if (out) {
    out->released = total;
    out->next_expiry_ns = res[1];
  }
  return DM_OK;
}

int dm_read_cleaned(dm_ctx* c, int64_t off, int64_t n, int64_t* rows) {
  DM_ENTER(c);
  if (!c->cl_valid) return c->fail(DM_E_STATE, "no dm_store_clean list (none yet, or the store was loaded or re-laid out since)");
  if (int rc = check_range(c, off, n, c->cl_n)) return rc;
  if (n > 0 && !rows) return c->fail(DM_E_INVAL, "null rows");
  DM_HIP(c, download(rows, (const int64_t*)c->cl_list.p, off, n, c->stream), "read cleaned rows");
  DM_HIP(c, hipStreamSynchronize(c->stream), "read cleaned rows");
  return DM_OK;
}
