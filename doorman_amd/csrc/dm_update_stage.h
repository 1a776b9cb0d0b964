// dm_update_stage.h — the device staging of the calls that change or read a loaded store:
// the one owner of the columns a call copies in, its flags words and their pinned mirror, and
// the events that order its copies before its kernels (dm_store_update.cpp, and the three
// reads of dm_store.cpp that resolve rows on the device).
// Part of dm_ctx.h, which includes it below the buffer types it uses.
#pragma once

namespace dm {

constexpr int kWChunks = 4;    // dm_store_apply: the refresh values' copy chunks
constexpr int kAsyncSets = 2;  // asynchronous batches in flight at most
// A set's flags words: one per part of a batch (words 0-2), and behind them the 8-B count of
// rows a dense refresh wrote (dm_store_refresh_wants_device; words kCountWord and the next,
// 8-B aligned), which only that call clears and fetches.
constexpr int kFlagWords = 6, kCountWord = 4;

// One set of staging.  A context has 1 + kAsyncSets (dm_ctx::stage):
//   - set 0 serves every call that is synchronous on return: the single updates, the
//     synchronous dm_store_apply, and dm_read_leases, dm_read_leases_rows and dm_read_store.
//     Each of them waits for the work it put on the set before it returns, and the calls of
//     one context do not overlap, so set 0 is idle whenever a call begins: one allocation
//     serves them all, grown by whichever call needs most.
//   - sets 1..kAsyncSets serve dm_store_apply_async: batch k uses set 1 + k % kAsyncSets and
//     is retired (waited for, its flags read) before batch k + kAsyncSets reuses the set.
// The columns are raw: a call ensures the ones its part needs and no others.
struct UpdateStage {
  // rows .. wants: a row part (upsert, row refresh, single release) and the reads' outputs; sub
  // also holds a batch's narrow int32 subclients.  rel: a batch's departures.  A masked refresh:
  // the mask, its packed values (mwants), the count pass' block sums (blk) and word offsets (wpre).
  DBuf<int64_t> rows, sub, exp, rel, blk;
  DBuf<double> has, wants, mwants;
  DBuf<uint64_t> mask;
  DBuf<int32_t> wpre;
  DBuf<uint32_t> flags;          // one flags word per part (a single call: word 0)
  HBuf<uint32_t> h_flags;        // their pinned host mirror
  // copies landed: a batch's parts ([0] also the single masked refresh; [k & 1] the single row
  // calls' chunk k), the refresh values' chunks; the asynchronous batch's last kernel and flags copy
  Event ev_bat[3], ev_wchunk[kWChunks], ev_done;
  bool pending = false;      // (asynchronous sets) enqueued, not yet retired
  bool may_general = false;  // its refresh or arrivals may bring NaN wants / other subclient counts
  int64_t nu = 0;            // its arrivals

  hipError_t create_events() {
    hipError_t e = ev_done.create(hipEventDisableTiming);
    for (Event& ev : ev_bat) e = e == hipSuccess ? ev.create(hipEventDisableTiming) : e;
    for (Event& ev : ev_wchunk) e = e == hipSuccess ? ev.create(hipEventDisableTiming) : e;
    return e;
  }
  template <typename... B>
  static hipError_t ensure_each(int64_t n, B&... b) {
    hipError_t e = hipSuccess;
    ((e = e == hipSuccess ? b.ensure((size_t)n) : e), ...);
    return e;
  }
  hipError_t ensure_upsert(int64_t n) { return ensure_each(n, rows, wants, has, sub, exp); }
  hipError_t ensure_mask(int64_t nwords, int64_t n_values) {
    hipError_t e = ensure_each(nwords, mask, wpre);
    if (e == hipSuccess) e = blk.ensure((size_t)((nwords + 255) / 256));
    return e == hipSuccess ? mwants.ensure((size_t)std::max<int64_t>(n_values, 1)) : e;
  }
  // A masked refresh of device columns: the count pass' scratch alone, no column.
  hipError_t ensure_scan(int64_t nwords) {
    const hipError_t e = wpre.ensure((size_t)nwords);
    return e == hipSuccess ? blk.ensure((size_t)((nwords + 255) / 256)) : e;
  }
  // The first `words` flags words cleared on stream st (the first call allocates them and
  // the mirror); flag(k): the device address of part k's word.
  hipError_t reset_flags(int words, hipStream_t st) {
    hipError_t e = hipSuccess;
    if (!flags.p) {
      e = flags.ensure(kFlagWords);
      if (e == hipSuccess) e = h_flags.alloc(kFlagWords, hipHostMallocDefault);
    }
    return e == hipSuccess ? hipMemsetAsync(flags.p, 0, words * sizeof(uint32_t), st) : e;
  }
  uint32_t* flag(int k) const { return flags.p + k; }
  unsigned long long* count() const { return reinterpret_cast<unsigned long long*>(flags.p + kCountWord); }
  hipError_t fetch_flags(int words, hipStream_t st) {
    return hipMemcpyAsync(h_flags.p, flags.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
  }
};
static_assert(!std::is_copy_constructible<UpdateStage>::value, "a staging set owns its buffers and events");

// The row bitmap of the uniqueness check, one bit per row of the store, shared by every set:
// the parts that name rows run one after the other on the context stream.  All-zero between
// parts: k_check_rows sets the bits of a part's rows and k_clear_rows, launched behind the
// part's apply kernel whether it was rejected or not, clears exactly those.  So it is cleared
// here only when it is allocated: for the first part, and when the store has grown.
struct RowBitmap {
  DBuf<uint32_t> bits;
  hipError_t ensure(int64_t N, hipStream_t st) {
    const size_t words = (size_t)(N / 32 + 1);
    if (bits.p && bits.n >= words) return hipSuccess;
    const hipError_t e = bits.ensure(words);
    return e == hipSuccess ? hipMemsetAsync(bits.p, 0, bits.n * sizeof(uint32_t), st) : e;
  }
};

}  // namespace dm
