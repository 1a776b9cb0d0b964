// dm_store_update.cpp — the calls that write rows of a loaded store from columns the caller
// gives, in host memory (staged) or device memory (read in place): the single updates (upsert,
// wants refreshes, release), the dense wants refresh, and a round's batch (dm_store_apply,
// synchronous and asynchronous) with its retirement.
#include "dm_ctx.h"

// An update's columns are staged in an UpdateStage (dm_update_stage.h: set 0 for every call
// that waits before it returns), validated on the device and applied on the context stream;
// what the flags its kernels leave mean is dm_update_outcome.h's to say.  Two copy schedules:
//   - a single call's columns cross PCIe in chunks on the copy stream while the context
//     stream validates the chunks already there (k_check_rows: no O(n) host pass, so pinned
//     buffers from dm_host_alloc go at full DMA rate);
//   - a batch's parts cross back to back, each validated and applied once it has landed.
// Neither copy waits for the context stream: the call (or, for an asynchronous batch, the
// set's retirement) waits for its kernels before the staging is used again, so the copies
// overlap whatever still runs there (e.g. an asynchronous tick), and each validation is
// ordered after that work and its copy.
struct StageCol {
  void* dst;
  const void* src;
  size_t elem;
};
static constexpr int64_t kStageChunk = 1 << 22;  // rows per copy/validate step of a single call

// Where a part's kernels read its columns: one parameter of row_part and mask_kernels, made from
// a call's `device` argument by the builders below, so that the host calls and their device
// twins (dm_store_*_device) are one sequence of launches.
//   - staged (the host calls): set S's columns, which the copy stream fills; the context
//     stream waits for each copy's event before the kernels that read it.
//   - in place (the device twins): the caller's own device columns, read on the context
//     stream where they lie.  No copy, no event, no column of S allocated: of S only the flags
//     words, their mirror and the masked refresh's blk / wpre scratch are used.  The caller
//     has ordered the columns' producer before the call, so every value is there: a single
//     call's rows are one step, a refresh's values one chunk.
struct UpdSrc {
  bool in_place = false;
  const uint64_t* mask = nullptr;  // a masked refresh: the mask and its packed values
  const double* mwants = nullptr;
  const int64_t *rows = nullptr, *rel = nullptr;  // row parts: an upsert's or refresh's rows, a release's
  const double *has = nullptr, *wants = nullptr;  // (has, exp: nullptr for narrow arrivals)
  const void* sub = nullptr;                      // int64, or int32 for narrow arrivals
  const int64_t* exp = nullptr;
};
// The staged source of set S: a single call's columns (b == nullptr: every column it copies is
// there), or batch b's, whose arrivals may be narrow.
static UpdSrc staged(const UpdateStage& S, const dm_store_batch* b) {
  UpdSrc u;
  u.mask = S.mask.p, u.mwants = S.mwants.p;
  u.rows = S.rows.p, u.rel = b ? S.rel.p : S.rows.p;
  u.has = !b || b->upsert_has ? S.has.p : nullptr;
  u.wants = S.wants.p, u.sub = S.sub.p;
  u.exp = !b || b->upsert_expiry_ns ? S.exp.p : nullptr;
  return u;
}
// The in-place source of batch b, every pointer the caller's.
static UpdSrc in_place(const dm_store_batch* b) {
  UpdSrc u;
  u.in_place = true;
  u.mask = b->wants_mask, u.mwants = b->wants;
  u.rows = b->upsert_rows, u.rel = b->release_rows;
  u.has = b->upsert_has, u.wants = b->upsert_wants;
  u.sub = b->upsert_subclients32 ? (const void*)b->upsert_subclients32 : b->upsert_subclients;
  u.exp = b->upsert_expiry_ns;
  return u;
}
// The in-place source of a single call that names rows (a release's rows too are `rows`, as in
// staged()), and of a single masked refresh.
static UpdSrc in_place(const int64_t* rows, const double* has, const double* wants, const int64_t* sub,
                       const int64_t* exp) {
  UpdSrc u;
  u.in_place = true;
  u.rows = u.rel = rows;
  u.has = has, u.wants = wants, u.sub = sub, u.exp = exp;
  return u;
}
static UpdSrc in_place(const uint64_t* mask, const double* mwants) {
  UpdSrc u;
  u.in_place = true;
  u.mask = mask, u.mwants = mwants;
  return u;
}

// How a call that dm_keep_keys may keep ends (dm_row_epoch.h): a wants refresh, and with
// DM_KEEP_UPDATES a release, an upsert or a synchronous batch.  Where the mode does not cover
// the call (an asynchronous batch never is) it starts a row epoch before it launches, as every
// writer does; where it does, once its flags are back -- kept (dm_ctx::refresh_kept,
// update_kept), or rows_changed() on every other way out of the call (a rejection, a NaN, a
// failure on the way).  Every one of these ends tells the large chain that rows were written.
namespace {
struct WriteEnd {
  dm_ctx* c;
  RowWrite w;
  RowWriteStart start;
  KeyClear kc;
  bool ended = false;
  WriteEnd(dm_ctx* ctx, RowWrite kind)
      : c(ctx), w(kind), start(row_write_start_mode(kind, ctx->keep_mode, ctx->keys_in_use())), kc(ctx->key_clear()) {
    if (!start.defer) end(true, false, 0);
  }
  ~WriteEnd() { end(true, false, 0); }
  const KeyClear* keys() const { return start.clear_keys ? &kc : nullptr; }  // the launchers' build
  void end(bool rejected, bool nan, int64_t n) {
    if (ended) return;
    ended = true;
    if (!row_write_kept_mode(w, c->keep_mode, rejected, nan))
      c->rows_changed();
    else if (is_refresh(w))
      c->refresh_kept(n);
    else
      c->update_kept(w, n);
  }
};

}  // namespace

// Host columns' rows [off, off + m) onto the copy stream (a column without a source: none).
static int copy_cols(dm_ctx* c, const StageCol* cols, int ncols, int64_t off, int64_t m) {
  for (const StageCol* k = cols; k < cols + ncols; ++k)
    if (k->src && m > 0)
      DM_HIP(c, hipMemcpyAsync((char*)k->dst + off * k->elem, (const char*)k->src + off * k->elem, (size_t)m * k->elem,
                               hipMemcpyHostToDevice, c->cpy),
             "stage update");
  return DM_OK;
}

// A part that names rows (an upsert, a row refresh, a release; alone or in a batch), its
// columns at src (staged in S, or the caller's in place): the device sequence on the context
// stream.  Its rows in range and unique (a bitmap over the table, O(n + N/64)) once they have landed, the rejection of the part
// before carried into its word, the apply kernel (which finds each row's resource, and returns
// at once from a rejected word), the bitmap cleared again.  cols: a single call's host columns,
// copied here chunk by chunk; b: a batch, whose part is already on its way and whose arrivals
// may be narrow (subclients of 4 B, no has: 0, no expiry: now + the resource's lease length).
static int row_part(dm_ctx* c, UpdateStage& S, const UpdSrc& src, const WriteEnd& we, UpdPart part, int64_t n,
                    const StageCol* cols, int ncols, const dm_store_batch* b) {
  hipStream_t st = c->stream;
  const int word = flags_word(part);
  uint32_t* F = S.flag(word);
  const int64_t* rows = writes_wants(part) ? src.rows : src.rel;
  const double* wants = writes_wants(part) ? src.wants : nullptr;
  const bool sub32 = b && b->upsert_subclients32;
  const int64_t* sub = writes_subclients(part) && !sub32 ? (const int64_t*)src.sub : nullptr;
  const int32_t* s32 = writes_subclients(part) && sub32 ? (const int32_t*)src.sub : nullptr;
  const int64_t step = b || src.in_place ? n : kStageChunk;
  int k = 0;
  for (int64_t off = 0; off < n; off += step, ++k) {
    const int64_t m = std::min(step, n - off);
    if (!src.in_place) {
      hipEvent_t ev = S.ev_bat[b ? word : k & 1];
      if (!b) {
        if (int rc = copy_cols(c, cols, ncols, off, m)) return rc;
        DM_HIP(c, hipEventRecord(ev, c->cpy), "stage update");
      }
      DM_HIP(c, hipStreamWaitEvent(st, ev, 0), "stage update");
    }
    DM_HIP(c, launch_check_rows(m, rows + off, c->N, c->row_bits.bits.p, wants ? wants + off : nullptr,
                                sub ? sub + off : nullptr, s32 ? s32 + off : nullptr, F, st),
           "check rows");
  }
  if (b) DM_HIP(c, launch_carry_reject(F - 1, F, st), "carry");
  const StoreCols sc = c->store_cols();
  if (!wants)
    DM_HIP(c, launch_release(n, rows, sc, F, c->dense_upd(), we.keys(), st), "release");
  else if (!writes_subclients(part))
    DM_HIP(c, launch_update_wants(n, rows, wants, sc, F, we.keys(), st), "update wants");
  else
    DM_HIP(c, launch_upsert(n, rows, src.has, wants, sub, s32, src.exp, b ? b->upsert_now_ns : 0, sc, F, c->dense_upd(),
                            we.keys(), st),
           "upsert");
  DM_HIP(c, launch_clear_rows(n, rows, c->N, c->row_bits.bits.p, st), "clear rows");
  return DM_OK;
}

// A masked refresh's copies (copy stream) and kernels (context stream).  nchunk 0, the single
// call: mask and values land behind one event, and one launch counts, scans and applies.
// Else, a batch: the count and scan run once the mask is there, and the n packed values cross
// in nchunk chunks, each applied as soon as it has landed (the apply of one chunk overlaps the
// next one's copy: C4 3.2 -> ~3.0 ms per step).
static int mask_copies(dm_ctx* c, UpdateStage& S, int64_t nwords, const uint64_t* mask, int64_t n, const double* wants,
                       int nchunk) {
  const StageCol cm{S.mask.p, mask, 8}, cv{S.mwants.p, wants, 8};
  if (int rc = copy_cols(c, &cm, 1, 0, nwords)) return rc;
  if (!nchunk)
    if (int rc = copy_cols(c, &cv, 1, 0, n)) return rc;
  DM_HIP(c, hipEventRecord(S.ev_bat[0], c->cpy), "stage update");
  for (int k = 0; k < nchunk; ++k) {
    if (int rc = copy_cols(c, &cv, 1, n * k / nchunk, n * (k + 1) / nchunk - n * k / nchunk)) return rc;
    DM_HIP(c, hipEventRecord(S.ev_wchunk[k], c->cpy), "stage update");
  }
  return DM_OK;
}

// (In place: mask and values are there, so nchunk is 0 and no event is waited for.)
static int mask_kernels(dm_ctx* c, UpdateStage& S, const UpdSrc& src, int64_t first_row, int64_t nwords, int64_t n,
                        uint32_t* flags, int nchunk, const KeyClear* kc) {
  hipStream_t st = c->stream;
  auto launch = [&](int phase, int64_t v0, int64_t v1) {
    return launch_update_wants_mask(nwords, src.mask, first_row, c->N, n, src.mwants, S.blk.p, S.wpre.p, c->store_cols(),
                                    flags, phase, v0, v1, kc, st);
  };
  if (!src.in_place) DM_HIP(c, hipStreamWaitEvent(st, S.ev_bat[0], 0), "stage update");
  DM_HIP(c, launch(nchunk ? 0 : 2, 0, INT64_MAX), "masked update");
  for (int k = 0; k < nchunk; ++k) {
    const int64_t v0 = n * k / nchunk, v1 = n * (k + 1) / nchunk;
    DM_HIP(c, hipStreamWaitEvent(st, S.ev_wchunk[k], 0), "stage update");
    if (v1 > v0) DM_HIP(c, launch(1, v0, v1), "masked update");
  }
  return DM_OK;
}

// A single call's end: its flags word back and the wait (the call is synchronous on return, so
// the caller may free its buffers and set 0 is idle again), then what the word says.  tail (a
// round's Assign, upsert_round below): what else the call's one wait covers is enqueued before
// the flags' copy, and its results are taken as soon as the wait is over, whatever the word says.
static int single_end(dm_ctx* c, UpdateStage& S, UpdPart part, WriteEnd& we, int64_t n, const UpsertTail* tail = nullptr) {
  if (tail)
    if (int rc = tail->enqueue()) return rc;
  DM_HIP(c, S.fetch_flags(1, c->stream), "update flags");
  if (int rs = c->synced("update")) return rs;
  if (tail) tail->landed();
  const uint32_t f = S.h_flags.p[0];
  const UpdOutcome o = update_outcome(part, f, false);
  if (o.code != DM_OK) return c->fail(o.code, o.msg);
  update_values(part, f, c->maybe_general, c->all_sub_one);
  we.end(false, f & kUpdNaN, n);
  c->have_result = false;
  return DM_OK;
}


// ---- the parts' argument rules, stated once for the single calls and batch_args ----

static bool block_aligned(int64_t first_row) { return first_row >= 0 && !(first_row & 63); }

// A masked refresh's scalars.  The single call checks them all; as a batch's part, a refresh
// without mask words is absent, and only packed values it may still bring are looked at.
static int mask_args(dm_ctx* c, int64_t first_row, int64_t nwords, const uint64_t* mask, int64_t n, const double* wants,
                     bool batch_part) {
  if ((!batch_part || nwords > 0) &&
      (!block_aligned(first_row) || nwords < 0 || n < 0 || (nwords > 0 && !mask) || (n > 0 && !wants)))
    return c->fail(DM_E_INVAL, "bad masked update (first_row must be a multiple of 64)");
  if (nwords == 0 && n > 0) return c->fail(DM_E_INVAL, "packed values without a mask");
  if (nwords > 0 && first_row + 64 * (nwords - 1) >= c->N) return c->fail(DM_E_RANGE, "mask words past the store's end");
  return DM_OK;
}
static int release_args(dm_ctx* c, int64_t n, const int64_t* rows) {
  return n < 0 || (n > 0 && !rows) ? c->fail(DM_E_INVAL, "bad release") : DM_OK;
}
// (narrow: a batch's arrivals, which may come without has and expiry; sub: of either width)
static int upsert_args(dm_ctx* c, int64_t n, const int64_t* rows, const double* has, const double* wants, const void* sub,
                       const int64_t* exp, bool narrow) {
  const bool missing = !rows || !wants || !sub || (!narrow && (!has || !exp));
  return n < 0 || (n > 0 && missing) ? c->fail(DM_E_INVAL, "bad upsert") : DM_OK;
}

// ---- the single calls, each one body for host columns and device columns ----
// The steps of every body: the entry, the argument checks, nothing to do; (device) the pointer
// checks; the call's WriteEnd; (host) set 0's columns and what is copied into them; the kernels
// from staged(S) or from the caller's columns in place; single_end.

// Every update call's entry (a batch's too).
static int update_enter(dm_ctx* c) {
  DM_ENTER(c);
  DM_STORE_OK(c);
  return c->store_loaded ? DM_OK : c->fail(DM_E_STATE, "no store loaded");
}

// A single call that names n > 0 rows, from its pointer checks on (a column the call does not
// take: nullptr, which every step passes over; stage: the staging's name in a failure).  tail:
// the columns are the context's own device buffers (no pointer check), and the call ends as
// single_end says.
static int single_rows(dm_ctx* c, bool device, UpdPart part, RowWrite kind, const char* stage, int64_t n,
                       const int64_t* rows, const double* has, const double* wants, const int64_t* sub, const int64_t* exp,
                       const UpsertTail* tail = nullptr) {
  if (device && !tail) {
    DM_DEVICE_PTR(c, rows, n * 8, "rows");
    DM_DEVICE_PTR(c, has, n * 8, "has");
    DM_DEVICE_PTR(c, wants, n * 8, "wants");
    DM_DEVICE_PTR(c, sub, n * 8, "subclients");
    DM_DEVICE_PTR(c, exp, n * 8, "expiry_ns");
  }
  if (part == UpdPart::upsert) c->expl_rows = true;  // (kept or not: the rows take explicit expiries)
  WriteEnd we(c, kind);  // (a refresh: a NaN wants ends a resource's dense state)
  UpdateStage& S = c->stage[0];
  if (!device)
    DM_HIP(c, !wants ? S.rows.ensure((size_t)n) : !sub ? S.ensure_each(n, S.rows, S.wants) : S.ensure_upsert(n), stage);
  const StageCol cols[] = {{S.rows.p, rows, 8}, {S.wants.p, wants, 8}, {S.sub.p, sub, 8}, {S.has.p, has, 8}, {S.exp.p, exp, 8}};
  const UpdSrc src = device ? in_place(rows, has, wants, sub, exp) : staged(S, nullptr);
  DM_HIP(c, c->row_bits.ensure(c->N, c->stream), "row bitmap");
  DM_HIP(c, S.reset_flags(1, c->stream), "update flags");
  if (int rc = row_part(c, S, src, we, part, n, cols, 5, nullptr)) return rc;
  return single_end(c, S, part, we, n, tail);
}

// A round's Assign (dm_decide_assign, dm_decide.cpp): dm_store_upsert_device's body from
// single_rows on, for a caller that has entered (DM_ENTER, ready) and whose n > 0 rows, unique
// by its selection, lie in the round's own compact columns, written by kernels already on the
// context stream.
int dm::upsert_round(dm_ctx* c, int64_t n, const int64_t* rows, const double* has, const double* wants,
                     const int64_t* sub, const int64_t* exp, const UpsertTail& tail) {
  return single_rows(c, true, UpdPart::upsert, RowWrite::upsert, "stage upsert", n, rows, has, wants, sub, exp, &tail);
}

static int upsert(dm_ctx* c, bool device, int64_t n, const int64_t* rows, const double* has, const double* wants,
                  const int64_t* sub, const int64_t* exp) {
  if (int rc = update_enter(c)) return rc;
  if (int rc = upsert_args(c, n, rows, has, wants, sub, exp, false)) return rc;
  if (n == 0) return DM_OK;
  return single_rows(c, device, UpdPart::upsert, RowWrite::upsert, "stage upsert", n, rows, has, wants, sub, exp);
}

static int update_wants(dm_ctx* c, bool device, int64_t n, const int64_t* rows, const double* wants) {
  if (int rc = update_enter(c)) return rc;
  if (n < 0 || (n > 0 && (!rows || !wants))) return c->fail(DM_E_INVAL, "bad update");
  if (n == 0) return DM_OK;
  return single_rows(c, device, UpdPart::refresh, RowWrite::refresh, "stage refresh", n, rows, nullptr, wants, nullptr, nullptr);
}


// The same narrow Assign with the rows as a bit mask (one bit per row of
// [first_row, first_row + 64 nwords)) and the values packed in row order: at
// more than ~3% of the rows updated the mask is smaller than 8-B row indices.
static int update_wants_mask(dm_ctx* c, bool device, int64_t first_row, int64_t nwords, const uint64_t* mask, int64_t n,
                             const double* wants) {
  if (int rc = update_enter(c)) return rc;
  if (int rc = mask_args(c, first_row, nwords, mask, n, wants, false)) return rc;
  if (nwords == 0) return DM_OK;
  if (device) {
    DM_DEVICE_PTR(c, mask, nwords * 8, "mask");
    if (n > 0) DM_DEVICE_PTR(c, wants, n * 8, "wants");
  }
  WriteEnd re(c, RowWrite::refresh_mask);  // a NaN wants ends a resource's dense state
  UpdateStage& S = c->stage[0];
  DM_HIP(c, device ? S.ensure_scan(nwords) : S.ensure_mask(nwords, n), device ? "mask scratch" : "stage mask");
  DM_HIP(c, S.reset_flags(1, c->stream), "update flags");
  if (!device)
    if (int rc = mask_copies(c, S, nwords, mask, n, wants, 0)) return rc;
  const UpdSrc src = device ? in_place(mask, wants) : staged(S, nullptr);
  if (int rc = mask_kernels(c, S, src, first_row, nwords, n, S.flag(0), 0, re.keys())) return rc;
  return single_end(c, S, UpdPart::refresh_mask, re, n);
}

static int release(dm_ctx* c, bool device, int64_t n, const int64_t* rows) {
  if (int rc = update_enter(c)) return rc;
  if (int rc = release_args(c, n, rows)) return rc;
  if (n == 0) return DM_OK;
  return single_rows(c, device, UpdPart::release, RowWrite::release, "stage rows", n, rows, nullptr, nullptr, nullptr, nullptr);
}

int dm_store_upsert(dm_ctx* c, int64_t n, const int64_t* rows, const double* has, const double* wants,
                    const int64_t* sub, const int64_t* exp) {
  return upsert(c, false, n, rows, has, wants, sub, exp);
}
int dm_store_upsert_device(dm_ctx* c, int64_t n, const int64_t* rows, const double* has, const double* wants,
                           const int64_t* sub, const int64_t* exp) {
  return upsert(c, true, n, rows, has, wants, sub, exp);
}
int dm_store_update_wants(dm_ctx* c, int64_t n, const int64_t* rows, const double* wants) {
  return update_wants(c, false, n, rows, wants);
}
int dm_store_update_wants_device(dm_ctx* c, int64_t n, const int64_t* rows, const double* wants) {
  return update_wants(c, true, n, rows, wants);
}
int dm_store_update_wants_mask(dm_ctx* c, int64_t first_row, int64_t nwords, const uint64_t* mask, int64_t n,
                               const double* wants) {
  return update_wants_mask(c, false, first_row, nwords, mask, n, wants);
}
int dm_store_update_wants_mask_device(dm_ctx* c, int64_t first_row, int64_t nwords, const uint64_t* mask, int64_t n,
                                      const double* wants) {
  return update_wants_mask(c, true, first_row, nwords, mask, n, wants);
}
int dm_store_release(dm_ctx* c, int64_t n, const int64_t* rows) { return release(c, false, n, rows); }
int dm_store_release_device(dm_ctx* c, int64_t n, const int64_t* rows) { return release(c, true, n, rows); }

// A wants refresh from a dense device column: wants[i] is the new wants of row first_row + i.
// One kernel (k_refresh_dense, dm_update.hip) finds the rows that are not released and whose
// bits differ from the stored wants, and applies exactly those as dm_store_update_wants_mask
// would for that mask: no mask, no packed values, no count or scan pass.  It ends as a masked
// refresh does (RowWrite::refresh_mask, UpdPart::refresh_mask for its flags word: only kUpdNaN
// can be set, the range was checked here).  Over PCIe: the flags word and the 8-B count.
int dm_store_refresh_wants_device(dm_ctx* c, int64_t first_row, int64_t n, const double* wants, int64_t* n_changed) {
  if (int rc = update_enter(c)) return rc;
  if (!block_aligned(first_row) || n < 0 || (n > 0 && !wants))
    return c->fail(DM_E_INVAL, "bad dense refresh (first_row must be a multiple of 64)");
  if (first_row > c->N || n > c->N - first_row) return c->fail(DM_E_RANGE, "rows past the store's end");
  if (n_changed) *n_changed = 0;
  if (n == 0) return DM_OK;
  DM_DEVICE_PTR(c, wants, n * 8, "wants");
  WriteEnd re(c, RowWrite::refresh_mask);  // a changed NaN wants ends a resource's dense state
  UpdateStage& S = c->stage[0];
  DM_HIP(c, S.reset_flags(kFlagWords, c->stream), "update flags");
  DM_HIP(c, launch_refresh_dense(n, first_row, wants, c->store_cols(), S.flag(0), S.count(), re.keys(), c->stream),
         "dense refresh");
  DM_HIP(c, S.fetch_flags(kFlagWords, c->stream), "update flags");
  if (int rs = c->synced("update")) return rs;
  const uint32_t f = S.h_flags.p[0];
  int64_t changed = 0;
  memcpy(&changed, S.h_flags.p + kCountWord, sizeof changed);
  update_values(UpdPart::refresh_mask, f, c->maybe_general, c->all_sub_one);
  re.end(false, f & kUpdNaN, changed);
  c->have_result = false;
  if (n_changed) *n_changed = changed;
  return DM_OK;
}

// One round of updates: every part's columns cross PCIe back to back on the copy
// stream; each part is validated and applied on the context stream as soon as its
// columns have landed (overlapping the later parts' copies), in the order refresh,
// departures, arrivals.  A part whose validation fails is not applied, nor is any
// later part (k_carry_reject); earlier parts stay applied.
static int batch_args(dm_ctx* c, const dm_store_batch* b) {
  if (!b) return c->fail(DM_E_INVAL, "null batch");
  const int64_t nw = b->wants_nwords, nm = b->wants_n, nr = b->release_n, nu = b->upsert_n;
  if (nw < 0 || nm < 0 || nr < 0 || nu < 0) return c->fail(DM_E_INVAL, "negative batch sizes");
  if (int rc = mask_args(c, b->wants_first_row, nw, b->wants_mask, nm, b->wants, true)) return rc;
  if (int rc = release_args(c, nr, b->release_rows)) return rc;
  // narrow arrivals: subclients as int32, has NULL (= 0), expiry NULL (= now + lease length)
  const void* sub = b->upsert_subclients32 ? (const void*)b->upsert_subclients32 : b->upsert_subclients;
  if (int rc = upsert_args(c, nu, b->upsert_rows, b->upsert_has, b->upsert_wants, sub, b->upsert_expiry_ns, true)) return rc;
  if (nu > 0 && !b->upsert_expiry_ns && !c->cfg_loaded)
    return c->fail(DM_E_STATE, "arrivals without expiries take the resource's lease length: load a configuration");
  if (nu > 0 && !b->upsert_expiry_ns && b->upsert_now_ns <= 0)  // an unset clock would insert lapsed leases
    return c->fail(DM_E_INVAL, "arrivals without expiries need upsert_now_ns (> 0): their expiry is now + lease length");
  return DM_OK;
}

// A device batch's columns (the struct itself is host memory): every pointer a part reads
// passes check_device_ptr with the part's bytes before any kernel is given it.
static int batch_device_ptrs(dm_ctx* c, const dm_store_batch* b) {
  const int64_t nw = b->wants_nwords, nm = b->wants_n, nr = b->release_n, nu = b->upsert_n;
  if (nw > 0) DM_DEVICE_PTR(c, b->wants_mask, nw * 8, "wants_mask");
  if (nw > 0 && nm > 0) DM_DEVICE_PTR(c, b->wants, nm * 8, "wants");
  if (nr > 0) DM_DEVICE_PTR(c, b->release_rows, nr * 8, "release_rows");
  if (nu > 0) {
    DM_DEVICE_PTR(c, b->upsert_rows, nu * 8, "upsert_rows");
    DM_DEVICE_PTR(c, b->upsert_has, nu * 8, "upsert_has");
    DM_DEVICE_PTR(c, b->upsert_wants, nu * 8, "upsert_wants");
    if (b->upsert_subclients32)
      DM_DEVICE_PTR(c, b->upsert_subclients32, nu * 4, "upsert_subclients32");
    else
      DM_DEVICE_PTR(c, b->upsert_subclients, nu * 8, "upsert_subclients");
    DM_DEVICE_PTR(c, b->upsert_expiry_ns, nu * 8, "upsert_expiry_ns");
  }
  return DM_OK;
}

// The batch's copies (copy stream), its three parts' kernels (context stream) and the
// flags' copy back into S.h_flags; nothing waits for them here.  we: the call's end (its
// key-clearing builds, and the row epoch it has started or will decide on).  device: the batch's
// columns are device memory, read in place (no copies); else they are staged in S, and the
// kernels' source is taken from S once its columns are allocated (ensure_* may move them).
static int apply_enqueue(dm_ctx* c, const dm_store_batch* b, UpdateStage& S, bool device, const WriteEnd& we) {
  const int64_t nw = b->wants_nwords, nm = b->wants_n, nr = b->release_n, nu = b->upsert_n;
  const bool sub32 = b->upsert_subclients32 != nullptr;
  if (nu > 0) c->expl_rows = true;  // arrivals take explicit expiries
  S.nu = nu;
  hipStream_t st = c->stream;
  DM_HIP(c, c->row_bits.ensure(c->N, st), "row bitmap");
  DM_HIP(c, S.reset_flags(3, st), "batch flags");
  // the refresh's packed values cross in up to kWChunks chunks of >= 2^21 values, so
  // that the synchronous call's apply overlaps its own copies; an asynchronous batch's
  // apply overlaps the next batch's copies anyway, and one copy costs less than four
  // (C4 2.95 -> 2.91 ms per step, alternated: tools/archive/gpu_r6_c4chunk.sh)
  const int nchunk = device                          ? 0
                     : we.w == RowWrite::apply_async ? 1
                                                     : (int)std::max<int64_t>(1, std::min<int64_t>(kWChunks, nm >> 21));
  // copies, back to back
  if (nw > 0 && device) DM_HIP(c, S.ensure_scan(nw), "mask scratch");
  if (nw > 0 && !device) {
    DM_HIP(c, S.ensure_mask(nw, nm), "stage mask");
    if (int rc = mask_copies(c, S, nw, b->wants_mask, nm, b->wants, nchunk)) return rc;
  }
  if (nr > 0 && !device) {
    DM_HIP(c, S.rel.ensure((size_t)nr), "stage release rows");
    const StageCol col{S.rel.p, b->release_rows, 8};
    if (int rc = copy_cols(c, &col, 1, 0, nr)) return rc;
    DM_HIP(c, hipEventRecord(S.ev_bat[1], c->cpy), "stage update");
  }
  if (nu > 0 && !device) {
    DM_HIP(c, S.ensure_upsert(nu), "stage upsert");
    const StageCol cols[] = {{S.rows.p, b->upsert_rows, 8},
                             {S.wants.p, b->upsert_wants, 8},
                             {S.sub.p, sub32 ? (const void*)b->upsert_subclients32 : b->upsert_subclients, sub32 ? 4u : 8u},
                             {S.has.p, b->upsert_has, 8},
                             {S.exp.p, b->upsert_expiry_ns, 8}};
    if (int rc = copy_cols(c, cols, 5, 0, nu)) return rc;
    DM_HIP(c, hipEventRecord(S.ev_bat[2], c->cpy), "stage update");
  }
  const UpdSrc src = device ? in_place(b) : staged(S, b);
  // part 1: wants refresh (validated by its count/scan passes over the mask)
  if (nw > 0)
    if (int rc = mask_kernels(c, S, src, b->wants_first_row, nw, nm, S.flag(0), nchunk, we.keys())) return rc;
  // part 2: departures
  if (nr > 0) {
    if (int rc = row_part(c, S, src, we, UpdPart::batch_release, nr, nullptr, 0, b)) return rc;
  } else {
    DM_HIP(c, launch_carry_reject(S.flag(0), S.flag(1), st), "carry");
  }
  // part 3: arrivals / full refreshes
  if (nu > 0)
    if (int rc = row_part(c, S, src, we, UpdPart::batch_upsert, nu, nullptr, 0, b)) return rc;
  DM_HIP(c, S.fetch_flags(3, st), "batch flags");
  c->have_result = false;
  return DM_OK;
}

// A landed batch's flags (dm_update_outcome.h batch_outcome; `late` marks an asynchronous
// batch reported by a later call).
static int apply_check(dm_ctx* c, const UpdateStage& S, bool late) {
  const UpdOutcome o = batch_outcome(S.h_flags.p, S.nu > 0, late, c->maybe_general, c->all_sub_one);
  return o.code != DM_OK ? c->fail(o.code, o.msg) : DM_OK;
}

// The synchronous batch, host (dm_store_apply) or device columns (dm_store_apply_device).
static int apply_sync(dm_ctx* c, const dm_store_batch* b, bool device) {
  if (int rc = update_enter(c)) return rc;
  if (int rc = batch_args(c, b)) return rc;
  if (device)
    if (int rc = batch_device_ptrs(c, b)) return rc;
  if (b->wants_nwords == 0 && b->release_n == 0 && b->upsert_n == 0) return DM_OK;
  UpdateStage& S = c->stage[0];
  WriteEnd we(c, RowWrite::apply);
  if (int rc = apply_enqueue(c, b, S, device, we)) return rc;
  if (int rs = c->synced("batch")) return rs;
  if (int rc = apply_check(c, S, false)) return rc;  // (a rejected part: a row epoch, ~WriteEnd)
  we.end(false, (S.h_flags.p[0] | S.h_flags.p[2]) & kUpdNaN, b->wants_n + b->release_n + b->upsert_n);
  return DM_OK;
}

int dm_store_apply(dm_ctx* c, const dm_store_batch* b) { return apply_sync(c, b, false); }
int dm_store_apply_device(dm_ctx* c, const dm_store_batch* b) { return apply_sync(c, b, true); }

// Retire asynchronous set S: wait for its batch, then its flags.
static int async_retire(dm_ctx* c, UpdateStage& S) {
  if (!S.pending) return DM_OK;
  const hipError_t e = hipEventSynchronize(S.ev_done);
  S.pending = false;
  if (e != hipSuccess) return c->fail(DM_E_HIP, std::string("asynchronous batch: ") + hipGetErrorString(e));
  return apply_check(c, S, true);
}

// The asynchronous batch, host or device columns: one sequence and the same sets for both.
static int apply_async(dm_ctx* c, const dm_store_batch* b, bool device) {
  if (int rc = update_enter(c)) return rc;
  if (int rc = batch_args(c, b)) return rc;
  if (device)
    if (int rc = batch_device_ptrs(c, b)) return rc;
  if (b->wants_nwords == 0 && b->release_n == 0 && b->upsert_n == 0) return DM_OK;
  UpdateStage& S = c->stage[1 + (int)(c->async_seq % kAsyncSets)];
  // the set's previous batch (kAsyncSets batches back) first: its flags, and its
  // staging free for these copies (this wait is what keeps the host kAsyncSets
  // batches ahead of the device at most)
  if (int rc = async_retire(c, S)) return rc;
  S.may_general = b->wants_nwords > 0 || b->upsert_n > 0;
  // (wants refreshes too start a row epoch: a NaN wants ends a resource's dense state, and
  // the batch's flags are read two batches later)
  WriteEnd we(c, RowWrite::apply_async);
  if (int rc = apply_enqueue(c, b, S, device, we)) return rc;
  DM_HIP(c, hipEventRecord(S.ev_done, c->stream), "batch done");
  S.pending = true;
  c->async_seq += 1;
  return DM_OK;
}

int dm_store_apply_async(dm_ctx* c, const dm_store_batch* b) { return apply_async(c, b, false); }
int dm_store_apply_device_async(dm_ctx* c, const dm_store_batch* b) { return apply_async(c, b, true); }

// Every set is retired (the flags of sets after a rejected one still count); the first
// failure and its message are returned.
int dm::async_retire_all(dm_ctx* c) {
  int first = DM_OK;
  std::string msg;
  for (int64_t k = c->async_seq - kAsyncSets; k < c->async_seq; ++k) {  // oldest first
    if (k < 0) continue;
    const int rc = async_retire(c, c->stage[1 + (int)(k % kAsyncSets)]);
    if (rc && first == DM_OK) {
      first = rc;
      msg = c->err;
    }
  }
  if (first != DM_OK) c->err = msg;
  return first;
}

// Asynchronous store batches still in flight finish before the store is replaced.  Their
// outcome is dropped with the store they updated: a rejected batch's error is lost here
// on purpose, and the load's own scan sets maybe_general / all_sub_one anew.
void dm::async_drain(dm_ctx* c) {
  for (int i = 1; i <= kAsyncSets; ++i)
    if (c->stage[i].pending) {
      (void)hipEventSynchronize(c->stage[i].ev_done);
      c->stage[i].pending = false;
    }
}

int dm_store_apply_wait(dm_ctx* c) {
  DM_ENTER(c);
  return async_retire_all(c);
}
