// dm_update.hip — the store-update kernels: validation, upsert, release, wants updates
// (by row list and by mask), and the lease read-back gathers.
#include <hip/hip_runtime.h>

#include "dm_kernel_util.h"
#include "dm_launch.h"
#include "dm_update_util.h"

namespace dm {

// --------------------------------------------------------------------------
// store maintenance
// --------------------------------------------------------------------------
// Assign on existing rows (store.go:153-167): running sums += new - old.
// Rows of one call may hit the same resource, so the deltas reach the sums
// through atomics — one per run of a resource within a wave (wave_seg_add,
// dm_update_util.h, with seg_of_row and the dense-state helpers).

// Validation of one store-update call on the device (no O(n) host pass): rows in
// range and unique within the call (a row bitmap, all-zero between calls), and
// the value flags the planner needs.  The apply kernels run only if no error bit
// is set, so a rejected call leaves the store untouched.
__global__ void k_check_rows(int64_t n, const int64_t* __restrict__ rows, int64_t N, uint32_t* bitmap,
                             const double* __restrict__ wants, const int64_t* __restrict__ sub,
                             const int32_t* __restrict__ sub32, uint32_t* flags) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t f = 0;
  if (i < n) {
    const int64_t r = rows[i];
    if (r < 0 || r >= N) {
      f |= kUpdRange;
    } else {
      const uint32_t bit = 1u << (r & 31);
      if (atomicOr(&bitmap[r >> 5], bit) & bit) f |= kUpdDup;
    }
    if (wants && __builtin_isnan(wants[i])) f |= kUpdNaN;
    if (sub || sub32) {
      const int64_t v = sub32 ? (int64_t)sub32[i] : sub[i];
      if (v < 0 || v > kSubMax) f |= kUpdSub;
      if (v != 1) f |= kUpdNotOne;
    }
  }
  // one atomic per wave and flag value
  const uint32_t lo = __builtin_amdgcn_readfirstlane(f);
  if (__all(f == lo)) {
    if ((threadIdx.x & 63) == 0 && lo) atomicOr(flags, lo);
  } else if (f) {
    atomicOr(flags, f);
  }
}

// Return the bitmap words of this call's rows to zero.
__global__ void k_clear_rows(int64_t n, const int64_t* __restrict__ rows, int64_t N, uint32_t* bitmap) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t r = rows[i];
  if (r >= 0 && r < N) bitmap[r >> 5] = 0u;
}

// Narrow arrivals (dm_store_batch): has == nullptr -> 0; sub32 instead of sub;
// expiry == nullptr -> the resource's now + lease length (the Assign's expiry,
// store.go:161).
// Two builds of one body each (dm_update_upsert.inc, dm_update_release.inc), as the refresh
// kernels below, whose comment has the rule, the clearing store and its stream order.  The
// key-clearing builds (k_upsert_keys, k_release_keys) run only under dm_keep_keys'
// DM_KEEP_UPDATES while some part has keys in use (dm_row_epoch.h); they store an invalid key
// for every workgroup-bin resource of which the call writes a row.  The tick kernels would
// not trust such a resource's key anyway (the stale hint, the mask bit: group_segment STEADY,
// k_sweep); cleared here, a valid key keeps meaning what dm_device.h FixKey says.
__global__ void k_upsert(int64_t n, const int64_t* __restrict__ rows, const double* __restrict__ has,
                         const double* __restrict__ wants, const int64_t* __restrict__ sub,
                         const int32_t* __restrict__ sub32, const int64_t* __restrict__ expiry,
                         const ResCfg* __restrict__ cfg, int64_t now, RowIndex ix, double* s_has, double* s_wants,
                         int32_t* s_sub, int64_t* s_exp, ResAgg* agg, uint8_t* expl, const uint32_t* flags,
                         DenseUpd du) {
  constexpr bool kKeys = false;
  const KeyClear kc{};
#include "dm_update_upsert.inc"
}

__global__ void k_upsert_keys(int64_t n, const int64_t* __restrict__ rows, const double* __restrict__ has,
                              const double* __restrict__ wants, const int64_t* __restrict__ sub,
                              const int32_t* __restrict__ sub32, const int64_t* __restrict__ expiry,
                              const ResCfg* __restrict__ cfg, int64_t now, RowIndex ix, double* s_has,
                              double* s_wants, int32_t* s_sub, int64_t* s_exp, ResAgg* agg, uint8_t* expl,
                              const uint32_t* flags, DenseUpd du, KeyClear kc) {
  constexpr bool kKeys = true;
#include "dm_update_upsert.inc"
}

__global__ void k_release(int64_t n, const int64_t* __restrict__ rows, RowIndex ix, double* s_has, double* s_wants,
                          int32_t* s_sub, int64_t* s_exp, ResAgg* agg, uint8_t* expl, const uint32_t* flags,
                          DenseUpd du) {
  constexpr bool kKeys = false;
  const KeyClear kc{};
#include "dm_update_release.inc"
}

__global__ void k_release_keys(int64_t n, const int64_t* __restrict__ rows, RowIndex ix, double* s_has,
                               double* s_wants, int32_t* s_sub, int64_t* s_exp, ResAgg* agg, uint8_t* expl,
                               const uint32_t* flags, DenseUpd du, KeyClear kc) {
  constexpr bool kKeys = true;
#include "dm_update_release.inc"
}

// Narrow Assign for a refresh that only changes wants (store.go:157):
// sumWants += new - old.  Rows are unique within one call.
// A released row is a free slot, not a client: a refresh of it changes nothing (a
// returning client is an arrival, dm_store_upsert).  Written into it, the wants would
// be subtracted from the resource's running sum by every later tick's Clean.
//
// Two builds of one body each (dm_update_wants.inc, dm_mask_apply.inc: the including
// kernel sets kKeys).  The plain one is every launch's unless dm_keep_keys is on and some
// part has fixed-point keys in use (dm_row_epoch.h); then the key-clearing build
// (k_update_wants_keys, k_mask_apply_keys) also stores an invalid key for every
// workgroup-bin resource in which a row changed.
// A row is changed when it is not released and its new wants differ from the stored wants
// as 64-bit patterns: -0.0 against +0.0 is a change, a client re-sending its stored value
// is none (its delta is x - x = +0.0, which leaves the bits of every sum but -0.0, and the
// sweep's write_fixed writes the sums it read either way, as the full path would).  The
// stores to the wants column and the atomics on sum_wants are the plain build's.
// Order: the key stores are on the context stream behind the call's wants stores.  The
// call entered through DM_ENTER (dm_ctx.h), which joined every class stream's tick work
// into the context stream (StreamOrder::join), so they follow the last tick's own key
// stores; and it marked the context stream as holding work (main_has_work), so the next
// tick's StreamOrder::fork makes every class stream wait for them, exactly as for the
// wants its row loads need (a tick on the context stream alone is behind them anyway).
__global__ void k_update_wants(int64_t n, const int64_t* __restrict__ rows, const double* __restrict__ wants,
                               RowIndex ix, const int32_t* __restrict__ s_sub, double* s_wants, ResAgg* agg,
                               const uint32_t* flags) {
  constexpr bool kKeys = false;
  const KeyClear kc{};
#include "dm_update_wants.inc"
}

__global__ void k_update_wants_keys(int64_t n, const int64_t* __restrict__ rows, const double* __restrict__ wants,
                                    RowIndex ix, const int32_t* __restrict__ s_sub, double* s_wants, ResAgg* agg,
                                    const uint32_t* flags, KeyClear kc) {
  constexpr bool kKeys = true;
#include "dm_update_wants.inc"
}

// ---- wants updates as a row mask + packed values (dm_store_update_wants_mask) ----
// Bit j of word w is row first_row + 64 w + j; the set rows take the packed values
// in ascending row order.  At 10% of the rows updated this moves 1.25 B of mask
// per update over PCIe instead of an 8-B row index (C4: 116 instead of 200 MB).
struct OpAddI64 {
  __device__ long long operator()(long long a, long long b) const { return a + b; }
};
// Pass 1: popcount per 256-word block (+ rows past the store's end), and every
// word's exclusive offset within its block.
__global__ __launch_bounds__(256) void k_mask_count(int64_t nwords, const uint64_t* __restrict__ mask,
                                                    int64_t first_row, int64_t N, int64_t* block_sums,
                                                    int32_t* word_pre, uint32_t* flags) {
  __shared__ int part[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t m = w < nwords ? mask[w] : 0ull;
  const int64_t row0 = first_row + 64 * w;
  if (m && row0 + 63 >= N) {  // bits of rows >= N
    const int64_t keep = N - row0;  // < 64
    const uint64_t ok = keep <= 0 ? 0ull : ((1ull << keep) - 1ull);
    if (m & ~ok) atomicOr(flags, kUpdRange);
  }
  const int c = __popcll(m);
  int incl = c;
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  int pre = incl - c;
  for (int i = 0; i < wave; ++i) pre += part[i];
  if (w < nwords) word_pre[w] = pre;
  if (threadIdx.x == 0) block_sums[blockIdx.x] = (int64_t)part[0] + part[1] + part[2] + part[3];
}

// Pass 2 (one workgroup): exclusive scan of the block sums in place; the total
// must equal the number of packed values.
__global__ __launch_bounds__(1024) void k_mask_scan(int64_t nblocks, int64_t* block_sums, int64_t n_values,
                                                    uint32_t* flags) {
  __shared__ int64_t tot[1024];
  const int t = threadIdx.x;
  const int64_t per = (nblocks + 1023) / 1024;
  const int64_t b0 = t * per < nblocks ? t * per : nblocks;
  const int64_t b1 = b0 + per < nblocks ? b0 + per : nblocks;
  int64_t s = 0;
  for (int64_t b = b0; b < b1; ++b) s += block_sums[b];
  tot[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {  // inclusive Hillis-Steele scan of the 1024 partials
    const int64_t v = t >= o ? tot[t - o] : 0;
    __syncthreads();
    tot[t] += v;
    __syncthreads();
  }
  int64_t run = tot[t] - s;
  for (int64_t b = b0; b < b1; ++b) {
    const int64_t v = block_sums[b];
    block_sums[b] = run;
    run += v;
  }
  if (t == 1023 && tot[1023] != n_values) atomicOr(flags, kUpdCount);
}

// Pass 3: one lane per row; a wave takes kMaskWords consecutive mask words (64
// rows each).  Lane q first fetches word q, its first value's offset and the
// resource of its first row (all words in parallel); then every row's loads of
// every word are issued before any is consumed (coalesced: per word the wave reads
// its packed values and 512 B of the wants column).  A resource's deltas stay in
// per-lane registers while consecutive words lie inside it and leave with one
// reduction + atomic when the resource changes; a word that spans resources adds
// its runs directly (wave_seg_add).
// The key-clearing build (k_update_wants has the rule; the body: dm_mask_apply.inc) keeps
// "a row of this lane's changed" beside `acc` and clears a resource's key where its deltas
// are flushed, by the lane that adds them, when some lane's did; a word that spans
// resources clears per run (wave_seg_add<true>).  The compare sits inside the branch that
// holds the row's values: 94 VGPRs against the plain build's 88, no scratch.
constexpr int kMaskWords = 16;
__global__ __launch_bounds__(256) void k_mask_apply(int64_t nwords, const uint64_t* __restrict__ mask,
                                                    int64_t first_row, const int64_t* __restrict__ block_offs,
                                                    const int32_t* __restrict__ word_pre,
                                                    const double* __restrict__ wants, RowIndex ix,
                                                    const int32_t* __restrict__ s_sub, double* s_wants, ResAgg* agg,
                                                    uint32_t* flags, int64_t vlo, int64_t vhi) {
  constexpr bool kKeys = false;
  const KeyClear kc{};
#include "dm_mask_apply.inc"
}

__global__ __launch_bounds__(256) void k_mask_apply_keys(int64_t nwords, const uint64_t* __restrict__ mask,
                                                         int64_t first_row, const int64_t* __restrict__ block_offs,
                                                         const int32_t* __restrict__ word_pre,
                                                         const double* __restrict__ wants, RowIndex ix,
                                                         const int32_t* __restrict__ s_sub, double* s_wants,
                                                         ResAgg* agg, uint32_t* flags, int64_t vlo, int64_t vhi,
                                                         KeyClear kc) {
  constexpr bool kKeys = true;
#include "dm_mask_apply.inc"
}

// ---- a wants refresh from a dense column (dm_store_refresh_wants_device) ----
// wants[i] is the new wants of row first_row + i (first_row a multiple of 64, checked with
// the range on the host; n any value).  The kernel acts as k_mask_apply would for the mask of
// the rows that are not released and whose new value differs from the stored one as 64-bit
// patterns, without that mask ever existing: k_mask_apply's shape (one lane per row,
// kMaskWords 64-row runs a wave, four waves a workgroup), every new and stored value loaded
// before the first use, and a run's changed mask is the wave's ballot -- so no count pass, no
// scan and no packed-value index.  The subclients word is loaded only by the lanes whose bits
// differ (the released test: the released mark, or an explicit row whose expiry is DM_RELEASED,
// which a load leaves until the first tick marks it); a run whose ballot is empty does nothing
// more; unchanged rows are not stored.  Deltas leave as k_mask_apply's do (`cur` / `acc`, wave_seg_add for a run
// that spans resources), so a resource none of whose rows changed sees no atomic and, in the
// key-clearing build, no key store: every flush there follows a changed row, and clears.
// kUpdNaN (a changed value that is NaN) and the count of rows written are reduced per wave
// and per workgroup: one atomic per workgroup on each word at most.
// About 16 B per row read, 8 B more per differing row, 8 B per changed row written.
__global__ __launch_bounds__(256) void k_refresh_dense(int64_t n, int64_t first_row,
                                                       const double* __restrict__ wants, RowIndex ix,
                                                       const int32_t* __restrict__ s_sub,
                                                       const int64_t* __restrict__ s_exp, double* s_wants,
                                                       ResAgg* agg, uint32_t* flags, unsigned long long* count) {
  constexpr bool kKeys = false;
  const KeyClear kc{};
#include "dm_refresh_dense.inc"
}

__global__ __launch_bounds__(256) void k_refresh_dense_keys(int64_t n, int64_t first_row,
                                                            const double* __restrict__ wants, RowIndex ix,
                                                            const int32_t* __restrict__ s_sub,
                                                            const int64_t* __restrict__ s_exp, double* s_wants,
                                                            ResAgg* agg, uint32_t* flags, unsigned long long* count,
                                                            KeyClear kc) {
  constexpr bool kKeys = true;
#include "dm_refresh_dense.inc"
}

// dm_store_apply: a part is applied only if no earlier part was rejected.
__global__ void k_carry_reject(const uint32_t* __restrict__ from, uint32_t* to) { *to |= *from & kUpdReject; }

// gets / expiry of scattered rows (dm_read_leases_rows)
// Rows as the store holds them (dm_device.h encoding), for the host: the expiry of
// row r (a follower's is its resource's follow_exp) and its subclients value.
// rows == nullptr: rows off .. off+n-1.
__global__ void k_resolve_rows(int64_t n, const int64_t* __restrict__ rows, int64_t off, const int32_t* __restrict__ sub,
                               const int64_t* __restrict__ expiry, RowIndex ix, const ResAgg* __restrict__ agg,
                               int64_t* out_exp, int64_t* out_sub) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t r = rows ? rows[i] : off + i;
  const int32_t raw = sub[r];
  int64_t e;
  if (sub_released(raw))
    e = kReleased;
  else if (raw < 0)
    e = expiry[r];
  else
    e = agg[seg_of_row(ix, r)].follow_exp;
  if (out_exp) out_exp[i] = e;
  if (out_sub) out_sub[i] = sub_value(raw);
}

__global__ void k_gather_leases(int64_t n, const int64_t* __restrict__ rows, const double* __restrict__ gets,
                                const int64_t* __restrict__ expiry, double* out_gets, int64_t* out_exp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t r = rows[i];
  out_gets[i] = gets[r];
  if (expiry) out_exp[i] = expiry[r];  // else resolved by k_resolve_rows
}

// --------------------------------------------------------------------------
// host-side launchers (called by dm_store.cpp and dm_store_update.cpp)
// --------------------------------------------------------------------------
hipError_t launch_upsert(int64_t n, const int64_t* rows, const double* has, const double* wants, const int64_t* sub,
                         const int32_t* sub32, const int64_t* expiry, int64_t now, const StoreCols& s,
                         const uint32_t* flags, const DenseUpd& du, const KeyClear* kc, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const unsigned grid = (unsigned)((n + 255) / 256);
  if (kc)
    k_upsert_keys<<<grid, 256, 0, st>>>(n, rows, has, wants, sub, sub32, expiry, s.cfg, now, s.ix, s.has, s.wants, s.sub,
                                        s.expiry, s.agg, s.expl, flags, du, *kc);
  else
    k_upsert<<<grid, 256, 0, st>>>(n, rows, has, wants, sub, sub32, expiry, s.cfg, now, s.ix, s.has, s.wants, s.sub,
                                   s.expiry, s.agg, s.expl, flags, du);
  return hipGetLastError();
}

hipError_t launch_release(int64_t n, const int64_t* rows, const StoreCols& s, const uint32_t* flags,
                          const DenseUpd& du, const KeyClear* kc, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const unsigned grid = (unsigned)((n + 255) / 256);
  if (kc)
    k_release_keys<<<grid, 256, 0, st>>>(n, rows, s.ix, s.has, s.wants, s.sub, s.expiry, s.agg, s.expl, flags, du, *kc);
  else
    k_release<<<grid, 256, 0, st>>>(n, rows, s.ix, s.has, s.wants, s.sub, s.expiry, s.agg, s.expl, flags, du);
  return hipGetLastError();
}

hipError_t launch_update_wants(int64_t n, const int64_t* rows, const double* wants, const StoreCols& s,
                               const uint32_t* flags, const KeyClear* kc, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const unsigned grid = (unsigned)((n + 255) / 256);
  if (kc)
    k_update_wants_keys<<<grid, 256, 0, st>>>(n, rows, wants, s.ix, s.sub, s.wants, s.agg, flags, *kc);
  else
    k_update_wants<<<grid, 256, 0, st>>>(n, rows, wants, s.ix, s.sub, s.wants, s.agg, flags);
  return hipGetLastError();
}

hipError_t launch_resolve_rows(int64_t n, const int64_t* rows, int64_t off, const int32_t* sub, const int64_t* expiry,
                               const RowIndex& ix, const ResAgg* agg, int64_t* out_exp, int64_t* out_sub,
                               hipStream_t st) {
  if (n <= 0) return hipSuccess;
  k_resolve_rows<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(n, rows, off, sub, expiry, ix, agg, out_exp, out_sub);
  return hipGetLastError();
}

hipError_t launch_gather_leases(int64_t n, const int64_t* rows, const double* gets, const int64_t* expiry,
                               double* out_gets, int64_t* out_exp, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  k_gather_leases<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(n, rows, gets, expiry, out_gets, out_exp);
  return hipGetLastError();
}

hipError_t launch_check_rows(int64_t n, const int64_t* rows, int64_t N, uint32_t* bitmap, const double* wants,
                             const int64_t* sub, const int32_t* sub32, uint32_t* flags, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  k_check_rows<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(n, rows, N, bitmap, wants, sub, sub32, flags);
  return hipGetLastError();
}

hipError_t launch_clear_rows(int64_t n, const int64_t* rows, int64_t N, uint32_t* bitmap, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  k_clear_rows<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(n, rows, N, bitmap);
  return hipGetLastError();
}

hipError_t launch_update_wants_mask(int64_t nwords, const uint64_t* mask, int64_t first_row, int64_t N,
                                    int64_t n_values, const double* wants, int64_t* block_sums, int32_t* word_pre,
                                    const StoreCols& s, uint32_t* flags, int phase, int64_t vlo, int64_t vhi,
                                    const KeyClear* kc, hipStream_t st) {
  if (nwords <= 0) return hipSuccess;
  const int64_t nb = (nwords + 255) / 256;
  if (phase != 1) {  // the mask's counts and value offsets (the mask alone)
    k_mask_count<<<(unsigned)nb, 256, 0, st>>>(nwords, mask, first_row, N, block_sums, word_pre, flags);
    k_mask_scan<<<1, 1024, 0, st>>>(nb, block_sums, n_values, flags);
  }
  if (phase != 0) {  // the rows whose values [vlo, vhi) have landed
    const int64_t waves = (nwords + kMaskWords - 1) / kMaskWords;
    const unsigned grid = (unsigned)((waves + 3) / 4);
    if (kc)
      k_mask_apply_keys<<<grid, 256, 0, st>>>(nwords, mask, first_row, block_sums, word_pre, wants, s.ix, s.sub, s.wants,
                                              s.agg, flags, vlo, vhi, *kc);
    else
      k_mask_apply<<<grid, 256, 0, st>>>(nwords, mask, first_row, block_sums, word_pre, wants, s.ix, s.sub, s.wants, s.agg,
                                         flags, vlo, vhi);
  }
  return hipGetLastError();
}

hipError_t launch_refresh_dense(int64_t n, int64_t first_row, const double* wants, const StoreCols& s, uint32_t* flags,
                                unsigned long long* count, const KeyClear* kc, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int64_t waves = (((n + 63) >> 6) + kMaskWords - 1) / kMaskWords;
  const unsigned grid = (unsigned)((waves + 3) / 4);
  if (kc)
    k_refresh_dense_keys<<<grid, 256, 0, st>>>(n, first_row, wants, s.ix, s.sub, s.expiry, s.wants, s.agg, flags, count,
                                               *kc);
  else
    k_refresh_dense<<<grid, 256, 0, st>>>(n, first_row, wants, s.ix, s.sub, s.expiry, s.wants, s.agg, flags, count);
  return hipGetLastError();
}

hipError_t launch_carry_reject(const uint32_t* from, uint32_t* to, hipStream_t st) {
  k_carry_reject<<<1, 1, 0, st>>>(from, to);
  return hipGetLastError();
}

}  // namespace dm
