// dm_store_update.cpp — the calls that change a loaded store: staged updates (upsert,
// wants refreshes, release), a round's batch (dm_store_apply, synchronous and
// asynchronous), the re-layout and Clean on the device.
#include "dm_ctx.h"

// Rows of one upsert/release call: in range and unique (a bitmap over the table,
// O(n + N/64)); the resource of each row is found on the device.
// The call's columns cross PCIe in chunks on an auxiliary stream while the
// context stream validates the chunks already there (k_check_rows: no O(n) host
// pass, so pinned buffers from dm_host_alloc go at full DMA rate).  The apply
// kernel then runs on the context stream; finish_update() maps the flags.
struct StageCol {
  void* dst;
  const void* src;
  size_t elem;
};
static constexpr int64_t kStageChunk = 1 << 22;  // rows per copy/validate step

// The update calls' flags word, cleared on the context stream (the first call allocates it
// and its pinned host mirror).
static int reset_upd_flags(dm_ctx* c) {
  if (!c->upd_flags.p) {
    DM_HIP(c, c->upd_flags.ensure(1), "update flags");
    DM_HIP(c, c->h_flags.alloc(1, hipHostMallocDefault), "update flags");
  }
  DM_HIP(c, hipMemsetAsync(c->upd_flags.p, 0, sizeof(uint32_t), c->stream), "update flags");
  return DM_OK;
}

static int staged_check(dm_ctx* c, int64_t n, const StageCol* cols, int ncols, bool check_wants, bool check_sub) {
  if (!c->row_bits.p || c->row_bits.n < (size_t)(c->N / 32 + 1)) {
    DM_HIP(c, c->row_bits.ensure((size_t)(c->N / 32 + 1)), "row bitmap");
    DM_HIP(c, hipMemsetAsync(c->row_bits.p, 0, c->row_bits.n * sizeof(uint32_t), c->stream), "row bitmap");
  }
  if (int rc = reset_upd_flags(c)) return rc;
  // Every call that reads the staging buffers (updates, dm_read_leases_rows) waits
  // for its kernels before it returns, so the copies need not wait for the context
  // stream: they overlap whatever is still running there (e.g. an asynchronous
  // tick), and each chunk's validation is ordered after that work and its copy.
  hipStream_t cp = c->cpy;
  int k = 0;
  for (int64_t off = 0; off < n; off += kStageChunk, ++k) {
    const int64_t m = std::min(kStageChunk, n - off);
    for (int j = 0; j < ncols; ++j)
      DM_HIP(c,
             hipMemcpyAsync((char*)cols[j].dst + off * cols[j].elem, (const char*)cols[j].src + off * cols[j].elem,
                            (size_t)m * cols[j].elem, hipMemcpyHostToDevice, cp),
             "stage update");
    hipEvent_t ev = c->ev_stage[k & 1];
    DM_HIP(c, hipEventRecord(ev, cp), "stage update");
    DM_HIP(c, hipStreamWaitEvent(c->stream, ev, 0), "stage update");
    DM_HIP(c, launch_check_rows(m, c->st_rows.p + off, c->N, c->row_bits.p, check_wants ? c->st_wants.p + off : nullptr,
                                check_sub ? c->st_sub.p + off : nullptr, nullptr, c->upd_flags.p, c->stream),
           "check rows");
  }
  return DM_OK;
}

// After the apply kernel: clear the bitmap, fetch the flags, wait (the call is
// synchronous on return, so the caller may free its buffers), map errors.
static int finish_update(dm_ctx* c, int64_t n, uint32_t* flags_out) {
  DM_HIP(c, launch_clear_rows(n, c->st_rows.p, c->N, c->row_bits.p, c->stream), "clear rows");
  DM_HIP(c, hipMemcpyAsync(c->h_flags.p, c->upd_flags.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream),
         "update flags");
  if (int rs = c->synced("update")) return rs;
  const uint32_t f = *c->h_flags.p;
  *flags_out = f;
  if (f & kUpdRange) return c->fail(DM_E_RANGE, "row out of range");
  if (f & kUpdDup) return c->fail(DM_E_INVAL, "rows must be unique within one call");
  if (f & kUpdSub) return c->fail(DM_E_INVAL, "subclients must be in [0, 2^31-2]");
  return DM_OK;
}

// How a call that dm_keep_keys may keep ends (dm_row_epoch.h): a wants refresh, and with
// DM_KEEP_UPDATES a release, an upsert or a synchronous batch.  Where the mode does not cover
// the call it starts a row epoch before it launches, as every writer does; where it does,
// once its flags are back -- kept (dm_ctx::refresh_kept, update_kept), or rows_changed() on
// every other way out of the call (a rejection, a NaN, a failure on the way).
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

int dm_store_upsert(dm_ctx* c, int64_t n, const int64_t* rows, const double* has, const double* wants,
                    const int64_t* sub, const int64_t* exp) {
  DM_ENTER(c);
  DM_STORE_OK(c);
  if (!c->store_loaded) return c->fail(DM_E_STATE, "no store loaded");
  if (n < 0 || (n > 0 && (!rows || !has || !wants || !sub || !exp))) return c->fail(DM_E_INVAL, "bad upsert");
  if (n == 0) return DM_OK;
  c->expl_rows = true;  // (kept or not: the rows take explicit expiries)
  WriteEnd we(c, RowWrite::upsert);
  DM_HIP(c, c->st_rows.ensure((size_t)n), "stage rows");
  DM_HIP(c, c->st_has.ensure((size_t)n), "stage has");
  DM_HIP(c, c->st_wants.ensure((size_t)n), "stage wants");
  DM_HIP(c, c->st_sub.ensure((size_t)n), "stage sub");
  DM_HIP(c, c->st_exp.ensure((size_t)n), "stage expiry");
  const StageCol cols[] = {{c->st_rows.p, rows, 8}, {c->st_wants.p, wants, 8}, {c->st_sub.p, sub, 8},
                           {c->st_has.p, has, 8}, {c->st_exp.p, exp, 8}};
  int rc = staged_check(c, n, cols, 5, true, true);
  if (rc) return rc;
  DM_HIP(c, launch_upsert(n, c->st_rows.p, c->st_has.p, c->st_wants.p, c->st_sub.p, nullptr, c->st_exp.p, c->cfg.p, 0,
                          c->row_index(), c->has.p, c->wants.p, c->sub.p, c->expiry.p, c->agg.p, c->expl.p,
                          c->upd_flags.p, c->dense_upd(), c->stream, we.keys()),
         "upsert");
  uint32_t f = 0;
  rc = finish_update(c, n, &f);
  if (rc) return rc;
  we.end(false, f & kUpdNaN, n);
  // an upsert can make a resource's subclients heterogeneous: stay conservative
  if ((f & (kUpdNaN | kUpdNotOne)) || !c->all_sub_one) c->maybe_general = true;
  if (f & kUpdNotOne) c->all_sub_one = false;
  c->have_result = false;
  return DM_OK;
}

int dm_store_update_wants(dm_ctx* c, int64_t n, const int64_t* rows, const double* wants) {
  DM_ENTER(c);
  DM_STORE_OK(c);
  if (!c->store_loaded) return c->fail(DM_E_STATE, "no store loaded");
  if (n < 0 || (n > 0 && (!rows || !wants))) return c->fail(DM_E_INVAL, "bad update");
  if (n == 0) return DM_OK;
  WriteEnd re(c, RowWrite::refresh);  // a NaN wants ends a resource's dense state
  DM_HIP(c, c->st_rows.ensure((size_t)n), "stage rows");
  DM_HIP(c, c->st_wants.ensure((size_t)n), "stage wants");
  const StageCol cols[] = {{c->st_rows.p, rows, 8}, {c->st_wants.p, wants, 8}};
  int rc = staged_check(c, n, cols, 2, true, false);
  if (rc) return rc;
  DM_HIP(c, launch_update_wants(n, c->st_rows.p, c->st_wants.p, c->row_index(), c->sub.p, c->wants.p, c->agg.p,
                                c->upd_flags.p, re.keys(), c->stream),
         "update wants");
  uint32_t f = 0;
  rc = finish_update(c, n, &f);
  if (rc) return rc;
  re.end(false, f & kUpdNaN, n);
  if (f & kUpdNaN) c->maybe_general = true;
  c->have_result = false;
  return DM_OK;
}

// The same narrow Assign with the rows as a bit mask (one bit per row of
// [first_row, first_row + 64 nwords)) and the values packed in row order: at
// more than ~3% of the rows updated the mask is smaller than 8-B row indices.
int dm_store_update_wants_mask(dm_ctx* c, int64_t first_row, int64_t nwords, const uint64_t* mask, int64_t n,
                               const double* wants) {
  DM_ENTER(c);
  DM_STORE_OK(c);
  if (!c->store_loaded) return c->fail(DM_E_STATE, "no store loaded");
  if (first_row < 0 || (first_row & 63) || nwords < 0 || n < 0 || (nwords > 0 && !mask) || (n > 0 && !wants))
    return c->fail(DM_E_INVAL, "bad masked update (first_row must be a multiple of 64)");
  if (nwords == 0) return n == 0 ? DM_OK : c->fail(DM_E_INVAL, "packed values without a mask");
  if (first_row + 64 * (nwords - 1) >= c->N) return c->fail(DM_E_RANGE, "mask words past the store's end");
  WriteEnd re(c, RowWrite::refresh_mask);  // a NaN wants ends a resource's dense state
  const int64_t nb = (nwords + 255) / 256;
  DM_HIP(c, c->st_mask.ensure((size_t)nwords), "stage mask");
  DM_HIP(c, c->st_wants.ensure((size_t)std::max<int64_t>(n, 1)), "stage wants");
  DM_HIP(c, c->st_blk.ensure((size_t)nb), "stage block sums");
  DM_HIP(c, c->st_wpre.ensure((size_t)nwords), "stage word offsets");
  if (int rc = reset_upd_flags(c)) return rc;
  // the copies overlap whatever still runs on the context's streams (staged_check)
  DM_HIP(c, hipMemcpyAsync(c->st_mask.p, mask, (size_t)nwords * 8, hipMemcpyHostToDevice, c->cpy), "stage mask");
  if (n > 0)
    DM_HIP(c, hipMemcpyAsync(c->st_wants.p, wants, (size_t)n * 8, hipMemcpyHostToDevice, c->cpy), "stage wants");
  DM_HIP(c, hipEventRecord(c->ev_stage[0], c->cpy), "stage update");
  DM_HIP(c, hipStreamWaitEvent(c->stream, c->ev_stage[0], 0), "stage update");
  DM_HIP(c, launch_update_wants_mask(nwords, c->st_mask.p, first_row, c->N, n, c->st_wants.p, c->st_blk.p,
                                     c->st_wpre.p, c->row_index(), c->sub.p, c->wants.p, c->agg.p, c->upd_flags.p,
                                     c->stream, 2, 0, INT64_MAX, re.keys()),
         "masked update");
  DM_HIP(c, hipMemcpyAsync(c->h_flags.p, c->upd_flags.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream),
         "update flags");
  if (int rs = c->synced("update")) return rs;
  const uint32_t f = *c->h_flags.p;
  if (f & kUpdRange) return c->fail(DM_E_RANGE, "mask bit past the store's end");
  if (f & kUpdCount) return c->fail(DM_E_INVAL, "packed values must match the mask's set bits");
  re.end(false, f & kUpdNaN, n);
  if (f & kUpdNaN) c->maybe_general = true;
  c->have_result = false;
  return DM_OK;
}

int dm_store_release(dm_ctx* c, int64_t n, const int64_t* rows) {
  DM_ENTER(c);
  DM_STORE_OK(c);
  if (!c->store_loaded) return c->fail(DM_E_STATE, "no store loaded");
  if (n < 0 || (n > 0 && !rows)) return c->fail(DM_E_INVAL, "bad release");
  if (n == 0) return DM_OK;
  WriteEnd we(c, RowWrite::release);
  DM_HIP(c, c->st_rows.ensure((size_t)n), "stage rows");
  const StageCol cols[] = {{c->st_rows.p, rows, 8}};
  int rc = staged_check(c, n, cols, 1, false, false);
  if (rc) return rc;
  DM_HIP(c, launch_release(n, c->st_rows.p, c->row_index(), c->has.p, c->wants.p, c->sub.p, c->expiry.p,
                           c->agg.p, c->expl.p, c->upd_flags.p, c->dense_upd(), c->stream, we.keys()),
         "release");
  uint32_t f = 0;
  rc = finish_update(c, n, &f);
  if (rc) return rc;
  we.end(false, false, n);
  c->have_result = false;
  return DM_OK;
}

// One round of updates: every part's columns cross PCIe back to back on the copy
// stream; each part is validated and applied on the context stream as soon as its
// columns have landed (overlapping the later parts' copies), in the order refresh,
// departures, arrivals.  A part whose validation fails is not applied, nor is any
// later part (k_carry_reject); earlier parts stay applied.
static int batch_args(dm_ctx* c, const dm_store_batch* b) {
  if (!c->store_loaded) return c->fail(DM_E_STATE, "no store loaded");
  if (!b) return c->fail(DM_E_INVAL, "null batch");
  const int64_t nw = b->wants_nwords, nm = b->wants_n, nr = b->release_n, nu = b->upsert_n;
  if (nw < 0 || nm < 0 || nr < 0 || nu < 0) return c->fail(DM_E_INVAL, "negative batch sizes");
  if (nw == 0 && nm > 0) return c->fail(DM_E_INVAL, "packed values without a mask");
  if (nw > 0) {
    const int64_t fr = b->wants_first_row;
    if (fr < 0 || (fr & 63) || !b->wants_mask || (nm > 0 && !b->wants))
      return c->fail(DM_E_INVAL, "bad masked update (first_row must be a multiple of 64)");
    if (fr + 64 * (nw - 1) >= c->N) return c->fail(DM_E_RANGE, "mask words past the store's end");
  }
  if (nr > 0 && !b->release_rows) return c->fail(DM_E_INVAL, "bad release");
  // narrow arrivals: subclients as int32, has NULL (= 0), expiry NULL (= now + lease length)
  const bool sub32 = b->upsert_subclients32 != nullptr;
  if (nu > 0 && (!b->upsert_rows || !b->upsert_wants || (!b->upsert_subclients && !sub32)))
    return c->fail(DM_E_INVAL, "bad upsert");
  if (nu > 0 && !b->upsert_expiry_ns && !c->cfg_loaded)
    return c->fail(DM_E_STATE, "arrivals without expiries take the resource's lease length: load a configuration");
  if (nu > 0 && !b->upsert_expiry_ns && b->upsert_now_ns <= 0)  // an unset clock would insert lapsed leases
    return c->fail(DM_E_INVAL, "arrivals without expiries need upsert_now_ns (> 0): their expiry is now + lease length");
  return DM_OK;
}

// The batch's copies (copy stream), its three parts' kernels (context stream) and the
// flags' copy back into S.h_flags; nothing waits for them here.  we: the synchronous call's
// end (its key-clearing builds, and the row epoch it has started or will decide on); null:
// an asynchronous batch, which starts a row epoch here.
static int apply_enqueue(dm_ctx* c, const dm_store_batch* b, dm_ctx::ApplySet& S, const WriteEnd* we) {
  const int64_t nw = b->wants_nwords, nm = b->wants_n, nr = b->release_n, nu = b->upsert_n;
  const bool sub32 = b->upsert_subclients32 != nullptr;
  if (nu > 0) c->expl_rows = true;  // arrivals take explicit expiries
  if (nu > 0 || nr > 0) c->chain.rows_written();  // subclients words written, rows released
  if (!we) c->rows_changed();  // (wants refreshes too: a NaN wants ends a resource's dense state)
  const KeyClear* kc = we ? we->keys() : nullptr;
  S.nu = nu;
  hipStream_t st = c->stream, cp = c->cpy;
  if (!S.flags.p) {
    DM_HIP(c, S.flags.ensure(3), "batch flags");
    DM_HIP(c, S.h_flags.alloc(3, hipHostMallocDefault), "batch flags");
  }
  if (!c->row_bits.p || c->row_bits.n < (size_t)(c->N / 32 + 1)) {
    DM_HIP(c, c->row_bits.ensure((size_t)(c->N / 32 + 1)), "row bitmap");
    DM_HIP(c, hipMemsetAsync(c->row_bits.p, 0, c->row_bits.n * sizeof(uint32_t), st), "row bitmap");
  }
  DM_HIP(c, hipMemsetAsync(S.flags.p, 0, 3 * sizeof(uint32_t), st), "batch flags");
  uint32_t* F = S.flags.p;
  // the refresh's packed values cross in up to kWChunks chunks of >= 2^21 values, so
  // that the synchronous call's apply overlaps its own copies; an asynchronous batch's
  // apply overlaps the next batch's copies anyway, and one copy costs less than four
  // (C4 2.95 -> 2.91 ms per step, alternated: tools/archive/gpu_r6_c4chunk.sh)
  const bool sync_set = &S == &c->aset[0];
  const int nchunk = nw == 0 ? 0 : !sync_set ? 1 : (int)std::max<int64_t>(1, std::min<int64_t>(dm_ctx::kWChunks, nm >> 21));
  // copies, back to back
  if (nw > 0) {
    DM_HIP(c, S.mask.ensure((size_t)nw), "stage mask");
    DM_HIP(c, S.mwants.ensure((size_t)std::max<int64_t>(nm, 1)), "stage wants");
    DM_HIP(c, S.blk.ensure((size_t)((nw + 255) / 256)), "stage block sums");
    DM_HIP(c, S.wpre.ensure((size_t)nw), "stage word offsets");
    DM_HIP(c, hipMemcpyAsync(S.mask.p, b->wants_mask, (size_t)nw * 8, hipMemcpyHostToDevice, cp), "stage mask");
    DM_HIP(c, hipEventRecord(S.ev_bat[0], cp), "stage");
    // the packed values in chunks, each applied as soon as it has landed (the apply
    // of one chunk overlaps the next one's copy): C4 3.2 -> ~3.0 ms per step
    for (int k = 0; k < nchunk; ++k) {
      const int64_t v0 = nm * k / nchunk, v1 = nm * (k + 1) / nchunk;
      if (v1 > v0)
        DM_HIP(c, hipMemcpyAsync(S.mwants.p + v0, b->wants + v0, (size_t)(v1 - v0) * 8, hipMemcpyHostToDevice, cp),
               "stage wants");
      DM_HIP(c, hipEventRecord(S.ev_wchunk[k], cp), "stage");
    }
  }
  if (nr > 0) {
    DM_HIP(c, S.rel.ensure((size_t)nr), "stage release rows");
    DM_HIP(c, hipMemcpyAsync(S.rel.p, b->release_rows, (size_t)nr * 8, hipMemcpyHostToDevice, cp), "stage rows");
    DM_HIP(c, hipEventRecord(S.ev_bat[1], cp), "stage");
  }
  if (nu > 0) {
    DM_HIP(c, S.rows.ensure((size_t)nu), "stage rows");
    DM_HIP(c, S.has.ensure((size_t)nu), "stage has");
    DM_HIP(c, S.wants.ensure((size_t)nu), "stage wants");
    DM_HIP(c, S.sub.ensure((size_t)nu), "stage sub");
    DM_HIP(c, S.exp.ensure((size_t)nu), "stage expiry");
    const StageCol cols[] = {{S.rows.p, b->upsert_rows, 8},
                             {S.wants.p, b->upsert_wants, 8},
                             {S.sub.p, sub32 ? (const void*)b->upsert_subclients32 : b->upsert_subclients, sub32 ? 4u : 8u},
                             {S.has.p, b->upsert_has, 8},
                             {S.exp.p, b->upsert_expiry_ns, 8}};
    for (const auto& col : cols)
      if (col.src)
        DM_HIP(c, hipMemcpyAsync(col.dst, col.src, (size_t)nu * col.elem, hipMemcpyHostToDevice, cp), "stage upsert");
    DM_HIP(c, hipEventRecord(S.ev_bat[2], cp), "stage");
  }
  // part 1: wants refresh (validated by its count/scan passes over the mask, then
  // applied chunk by chunk as the values land)
  if (nw > 0) {
    DM_HIP(c, hipStreamWaitEvent(st, S.ev_bat[0], 0), "stage");
    DM_HIP(c, launch_update_wants_mask(nw, S.mask.p, b->wants_first_row, c->N, nm, S.mwants.p, S.blk.p, S.wpre.p,
                                       c->row_index(), c->sub.p, c->wants.p, c->agg.p, F + 0, st, 0, 0, 0),
           "masked update");
    for (int k = 0; k < nchunk; ++k) {
      const int64_t v0 = nm * k / nchunk, v1 = nm * (k + 1) / nchunk;
      DM_HIP(c, hipStreamWaitEvent(st, S.ev_wchunk[k], 0), "stage");
      if (v1 > v0)
        DM_HIP(c, launch_update_wants_mask(nw, S.mask.p, b->wants_first_row, c->N, nm, S.mwants.p, S.blk.p, S.wpre.p,
                                           c->row_index(), c->sub.p, c->wants.p, c->agg.p, F + 0, st, 1, v0, v1, kc),
               "masked update");
    }
  }
  // part 2: departures
  if (nr > 0) {
    DM_HIP(c, hipStreamWaitEvent(st, S.ev_bat[1], 0), "stage");
    DM_HIP(c, launch_check_rows(nr, S.rel.p, c->N, c->row_bits.p, nullptr, nullptr, nullptr, F + 1, st), "check rows");
    DM_HIP(c, launch_carry_reject(F + 0, F + 1, st), "carry");
    DM_HIP(c, launch_release(nr, S.rel.p, c->row_index(), c->has.p, c->wants.p, c->sub.p, c->expiry.p, c->agg.p,
                             c->expl.p, F + 1, c->dense_upd(), st, kc),
           "release");
    DM_HIP(c, launch_clear_rows(nr, S.rel.p, c->N, c->row_bits.p, st), "clear rows");
  } else {
    DM_HIP(c, launch_carry_reject(F + 0, F + 1, st), "carry");
  }
  // part 3: arrivals / full refreshes
  if (nu > 0) {
    DM_HIP(c, hipStreamWaitEvent(st, S.ev_bat[2], 0), "stage");
    const int64_t* s64 = sub32 ? nullptr : S.sub.p;
    const int32_t* s32 = sub32 ? (const int32_t*)S.sub.p : nullptr;
    DM_HIP(c, launch_check_rows(nu, S.rows.p, c->N, c->row_bits.p, S.wants.p, s64, s32, F + 2, st), "check rows");
    DM_HIP(c, launch_carry_reject(F + 1, F + 2, st), "carry");
    DM_HIP(c, launch_upsert(nu, S.rows.p, b->upsert_has ? S.has.p : nullptr, S.wants.p, s64, s32,
                            b->upsert_expiry_ns ? S.exp.p : nullptr, c->cfg.p, b->upsert_now_ns, c->row_index(),
                            c->has.p, c->wants.p, c->sub.p, c->expiry.p, c->agg.p, c->expl.p, F + 2, c->dense_upd(), st,
                            kc),
           "upsert");
    DM_HIP(c, launch_clear_rows(nu, S.rows.p, c->N, c->row_bits.p, st), "clear rows");
  }
  DM_HIP(c, hipMemcpyAsync(S.h_flags.p, F, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "batch flags");
  c->have_result = false;
  return DM_OK;
}

// A landed batch's flags: the first rejected part fails the call (its message names the
// part; `late` marks an asynchronous batch reported by a later call), NaN wants or
// other subclient counts make the store maybe-general.
static int apply_check(dm_ctx* c, const dm_ctx::ApplySet& S, bool late) {
  const uint32_t f0 = S.h_flags.p[0], f1 = S.h_flags.p[1], f2 = S.h_flags.p[2];
  auto reject = [&](uint32_t f, const char* part) -> int {
    const std::string p = std::string(late ? "an earlier asynchronous batch's " : "") + part;
    if (f & kUpdRange) return c->fail(DM_E_RANGE, p + ": row out of range");
    if (f & kUpdCount) return c->fail(DM_E_INVAL, p + ": packed values must match the mask's set bits");
    if (f & kUpdDup) return c->fail(DM_E_INVAL, p + ": rows must be unique within one part");
    return c->fail(DM_E_INVAL, p + ": subclients must be in [0, 2^31-2]");
  };
  if (f0 & kUpdReject) return reject(f0, "wants refresh");
  if (f0 & kUpdNaN) c->maybe_general = true;
  if (f1 & kUpdReject) return reject(f1, "release");
  if (f2 & kUpdReject) return reject(f2, "upsert");
  if (S.nu > 0) {
    if ((f2 & (kUpdNaN | kUpdNotOne)) || !c->all_sub_one) c->maybe_general = true;
    if (f2 & kUpdNotOne) c->all_sub_one = false;
  }
  return DM_OK;
}

int dm_store_apply(dm_ctx* c, const dm_store_batch* b) {
  DM_ENTER(c);
  DM_STORE_OK(c);
  if (int rc = batch_args(c, b)) return rc;
  if (b->wants_nwords == 0 && b->release_n == 0 && b->upsert_n == 0) return DM_OK;
  dm_ctx::ApplySet& S = c->aset[0];
  WriteEnd we(c, RowWrite::apply);
  if (int rc = apply_enqueue(c, b, S, &we)) return rc;
  if (int rs = c->synced("batch")) return rs;
  if (int rc = apply_check(c, S, false)) return rc;  // (a rejected part: a row epoch, ~WriteEnd)
  we.end(false, (S.h_flags.p[0] | S.h_flags.p[2]) & kUpdNaN, b->wants_n + b->release_n + b->upsert_n);
  return DM_OK;
}

// Retire asynchronous set S: wait for its batch, then its flags.
static int async_retire(dm_ctx* c, dm_ctx::ApplySet& S) {
  if (!S.pending) return DM_OK;
  const hipError_t e = hipEventSynchronize(S.ev_done);
  S.pending = false;
  if (e != hipSuccess) return c->fail(DM_E_HIP, std::string("asynchronous batch: ") + hipGetErrorString(e));
  return apply_check(c, S, true);
}

int dm_store_apply_async(dm_ctx* c, const dm_store_batch* b) {
  DM_ENTER(c);
  DM_STORE_OK(c);
  if (int rc = batch_args(c, b)) return rc;
  if (b->wants_nwords == 0 && b->release_n == 0 && b->upsert_n == 0) return DM_OK;
  dm_ctx::ApplySet& S = c->aset[1 + (int)(c->async_seq % dm_ctx::kAsyncSets)];
  // the set's previous batch (kAsyncSets batches back) first: its flags, and its
  // staging free for these copies (this wait is what keeps the host kAsyncSets
  // batches ahead of the device at most)
  if (int rc = async_retire(c, S)) return rc;
  S.may_general = b->wants_nwords > 0 || b->upsert_n > 0;
  if (int rc = apply_enqueue(c, b, S, nullptr)) return rc;
  DM_HIP(c, hipEventRecord(S.ev_done, c->stream), "batch done");
  S.pending = true;
  c->async_seq += 1;
  return DM_OK;
}

// Every set is retired (the flags of sets after a rejected one still count); the first
// failure and its message are returned.
int dm::async_retire_all(dm_ctx* c) {
  int first = DM_OK;
  std::string msg;
  for (int64_t k = c->async_seq - dm_ctx::kAsyncSets; k < c->async_seq; ++k) {  // oldest first
    if (k < 0) continue;
    const int rc = async_retire(c, c->aset[1 + (int)(k % dm_ctx::kAsyncSets)]);
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
  for (int i = 1; i <= dm_ctx::kAsyncSets; ++i)
    if (c->aset[i].pending) {
      (void)hipEventSynchronize(c->aset[i].ev_done);
      c->aset[i].pending = false;
    }
}

int dm_store_apply_wait(dm_ctx* c) {
  DM_ENTER(c);
  return async_retire_all(c);
}

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
