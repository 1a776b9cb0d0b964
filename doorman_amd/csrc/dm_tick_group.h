// dm_tick_group.h — what the units of the resource-per-group kernels share: group_segment (the
// body of every workgroup-bin and sub-wave kernel) with the device functions it uses, and the
// host-side list of the workgroup bins' shapes.  dm_tick_steady.h states the split form's
// dense-side kernels over it; dm_tick_group.hip holds the other kernels and the launchers;
// dm_tick_masked.hip instantiates the masked builds (dm_keep_keys' DM_KEEP_FREE_SLOTS) in a unit,
// and so a code object, of their own: dm_tick_group.hip's device code does not depend on them.
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <type_traits>

#include "dm_kernel_util.h"
#include "dm_launch.h"
#include "dm_update_util.h"

namespace dm {

// --------------------------------------------------------------------------
// Resource-per-group kernel: G threads (a wave or a 256-thread workgroup) own
// one resource of up to G*R rows; rows live in VGPRs across all passes.
// --------------------------------------------------------------------------
// MODE (the 128/256/512-thread bins): kMixed = one kernel for every item (hint or
// not), kDenseOnly = items whose hint is set (k_block_dense: no subclients column at
// all; a stale hint queues the item for k_block_rest and returns), kRest = queued
// items (k_block_rest: the column is read, the hint rewritten).
enum { kMixed = 0, kDenseOnly = 1, kRest = 2 };
// Gets stores: non-temporal for the workgroup bins and the large chain (long contiguous
// spans: whole lines); plain for the sub-wave groups, whose spans are short and
// unaligned, so that L2 merges the partial sectors two groups write at a resource
// boundary (C2 112.2-112.5 -> 109.6-111.1 us, three interleaved rounds; the chain's
// stores plain: no change; profiles/r05_ab/c2_gets_stores.txt; the chain's maps take
// put_live's default, map_row in dm_tick_large.h)
template <int G> constexpr bool kGroupNT = G >= 128;

// One live row's gets in the skipping map of group_segment: the resource's algorithm on
// the row's wants / has / subclients and the passes' sums, the same decisions as the
// plain loop's (which keeps its inline form: every build without the skip is then the
// code it was, register for register).
__device__ __forceinline__ double row_gets(const Res& rs, bool ps, double C, double eq, const Clean& cl,
                                           const AggB& b, const FsU& fu, double w, double h, int s) {
  if (rs.learning) return h;             // Learn (algorithm.go:297-302)
  if (rs.kind == 0) return w;            // NoAlgorithm
  if (rs.kind == 1) return minF(C, w);   // Static
  if (ps) {
    const double epc = eq * (double)s;         // :233
    const double unused = C - cl.sum_has + h;  // :239
    return (cl.sum_wants <= C || w <= epc) ? minF(w, unused)                               // :245
                                           : minF(epc + (w - epc) * (b.x / b.y), unused);  // :283
  }
  return fs_uniform_row(w, h, C, cl.sum_has, fu);
}

// Thread 0: the item's fixed-point key (dm_device.h FixKey) after this tick.  Stored only
// when it differs from the one loaded, unless the launch does not use the keys: then
// whatever the array holds is overwritten.
__device__ __forceinline__ void put_key(FixKey* key, const FixKey& fk, int use_keys, bool fix, double C, int kind) {
  const FixKey nk{fix ? (uint64_t)__double_as_longlong(C) : 0ull, fix ? kind : 0, fix ? 1 : 0};
  if (!use_keys || nk.cbits != fk.cbits || nk.kind != fk.kind || nk.valid != fk.valid) *key = nk;
}

// The builds of group_segment, a set of flags: group_segment<G, R, kDenseOnly, kFixed | kList>.
// A flag's value includes the flags it implies (has_build asks for all of its bits).  Kernels
// that differ only in their build are one template over these flags (dm_tick_steady.h); what
// guards each build's code is tools/isa_diff.py, against the parent's, kernel for kernel.
//   kSkip    unchanged runs of gets are not stored (a writeback tick in place)
//   kSteady  Clean's result is known; an item it is not known for goes to the rest queue
//   kFixed   the steady, skipping build that keeps a fixed-point key per item (FixKey)
//   kList    the caller is a loop over a worklist (k_block_list, k_block_fused)
//   kCycle   the fixed-point list build on the alternate column (CycAux)
//   kMasked  a steady build that also takes items with released rows (DM_KEEP_FREE_SLOTS)
using Build = unsigned;
constexpr Build kSkip = 1u, kSteady = 2u, kFixed = 4u | kSkip | kSteady, kList = 8u, kCycle = 16u | kFixed | kList,
                kMasked = 32u | kSteady;
constexpr bool has_build(Build b, Build f) { return (b & f) == f; }

// The steady `rest` test: an item a steady build does not decide (k_block_rest does).  A stale
// hint, a released-row or arrival bit, lapsed followers, recompute mode.  MASKED: the
// released-row bit alone does not send the item there, but an item with no live row does
// (under these conditions the running count is exact and every live row counts at least 1):
// the plain path's empty-range arithmetic stays in one place.  (group_segment keeps the one
// written-out copy of this test, which must equal this function: called there, the unmasked
// steady builds' code moves.  key_holds is called there too.)
template <bool MASKED>
__device__ __forceinline__ bool steady_rest(const DevParams& p, const Res& rs, int hw, int hint) {
  return dense_subclients(rs) != hint || (hw >> 8 & (MASKED ? 2 : 3)) != 0 || p.now > rs.follow_exp || p.recompute ||
         (MASKED && rs.agg_count == 0);
}
// The key against the record: its tick computed with this capacity and kind, outside learning.
__device__ __forceinline__ bool key_holds(const FixKey& fk, const Res& rs) {
  return fk.cbits == (uint64_t)__double_as_longlong(rs.C) && fk.kind == rs.kind && !rs.learning;
}

// What a fixed-point build and the sweep's lanes do with an item whose key holds: the record
// as the full path would write it (follow_exp moves, the exchange's block is published, the
// state byte stays), the sums it read and a delta of +0.0.
__device__ __forceinline__ void write_fixed(const DevParams& p, int seg, const Res& rs, int hint) {
  write_resource(p, seg, rs, Clean{rs.agg_count, rs.agg_has, rs.agg_wants}, 0.0, hint);
}
// The cycle form's step for an item whose key holds (CycAux; axp: the item's entry in memory,
// ax: its copy).  State 2: the item reproduces its state of two ticks ago, which its destination
// column still holds -- write_fixed's record with sum_has := prev_has, and prev_has becomes the
// sum just read, a store only where they differ; true: done.  State 1: the back-off goes on
// (carry), or has run out and the row kernel probes.
__device__ __forceinline__ bool cycle_step(const DevParams& p, int seg, const Res& rs, int hint, int state, CycAux* axp,
                                           CycAux& ax, int& probe, int& carry) {
  if (state == 2) {
    write_resource(p, seg, rs, Clean{rs.agg_count, __longlong_as_double((long long)ax.prev_has), rs.agg_wants}, 0.0,
                   hint);
    const uint64_t was = (uint64_t)__double_as_longlong(rs.agg_has);
    if (ax.prev_has != was) axp->prev_has = was;
    return true;
  }
  if (ax.skip > 0) {
    ax.skip -= 1;
    axp->skip = ax.skip;
    carry = 1;
  } else {
    probe = carry = 1;
  }
  return false;
}

// One lane's item in a sweep (k_sweep, step 1 of k_block_fused): the tests a kFixed build makes
// before its rows -- a zero hint word, the `rest` test, the key against the record -- and, where
// all pass, the item's whole tick.  state: the key's, as the launch trusts it (0: not at all).
// done: nothing is left to do; else the item is listed, for k_block_rest's body if to_rest.
// SPLIT (k_block_fused, which runs both bodies) classifies an item without a trusted key too;
// else it is listed with no record loaded, and the row kernel's own test hands it on.
struct LaneClass { bool done, to_rest; int probe, carry; };
template <bool CYCLE, bool MASKED, bool SPLIT>
__device__ __forceinline__ LaneClass sweep_lane(const DevParams& p, const WorkItem& wi, const FixKey& fk, int state,
                                                CycAux* axp, CycAux& ax) {
  LaneClass c{false, false, 0, 0};
  const int hw = wi.n >> 16;
  if (hw == 0) {
    c.to_rest = true;
  } else if (SPLIT || state != 0) {
    const Res rs = load_res(p, wi.seg);
    const int hint = hw & 0xFF;
    if (steady_rest<MASKED>(p, rs, hw, hint)) {
      c.to_rest = true;
    } else if (state != 0 && key_holds(fk, rs)) {
      if constexpr (CYCLE) {
        c.done = cycle_step(p, wi.seg, rs, hint, state, axp, ax, c.probe, c.carry);
      } else {
        write_fixed(p, wi.seg, rs, hint);
        c.done = true;
      }
    }
  }
  return c;
}

// One thread (`one`) tells the host a worklist's {count, row epoch} (host-mapped: the next
// launches' grid size, a hint) when either differs from the last told (told[0], told[1]), or
// `always`.  The count's high half: the host's stamp of the launch (the cycle form; else 0).
__device__ __forceinline__ void tell_count(bool one, int32_t* told, int count, unsigned long long* host_count,
                                           unsigned long long epoch, unsigned stamp, bool always) {
  if (one && (always || told[0] != count || told[1] != (int32_t)epoch)) {
    __hip_atomic_store(host_count, (unsigned long long)(unsigned)count | (unsigned long long)stamp << 32,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(host_count + 1, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    told[0] = count;
    told[1] = (int32_t)epoch;
  }
}
// One thread hands item qidx to the rest queue: its key cleared first (KEY), at most one
// entry per item and tick (a guarded tick's count may grow past qcap), and the guard set
// where the launch has one.  (The count's slot is qcnt + par, added here and not by the
// caller: ahead of the key's store the addition moves the kFixed build's code.)
template <bool KEY>
__device__ __forceinline__ void hand_off(FixKey* key, const FixKey& fk, int use_keys, int32_t* queue, int32_t* qcnt,
                                         int par, int32_t qidx, int qcap, int32_t* guard) {
  if constexpr (KEY) put_key(key, fk, use_keys, false, 0.0, 0);  // before the hand-off
  const int q = atomicAdd(qcnt + par, 1);
  if (q < qcap) queue[q] = qidx;
  if (guard) __hip_atomic_store(guard, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// kList: the caller is a loop over items (k_block_list).  Behind an earlier item's
// stores the compiler loads the record with vector loads, a register per dword and lane
// through every pass (128 x 8: 88 VGPRs against 65); the record is moved back to SGPRs.
// kCycle (k_block_list's and k_block_fused's cycle builds): kFixed | kList on the alternate
// column, p.out_gets != p.has (dm_device.h CycAux has the key's states and the proof).  probe: the item's key is
// in state 1 under this capacity and kind (the sweep saw to it, SweepEntry::pad: no dependent
// load): the destination rows are loaded with the others and the SKIP ballot compares against
// them -- skipping an equal run is always correct, only the key's conclusion rests on what
// the destination held.  Without it every run is stored.  carry: the back-off goes on.
// kMasked (dm_tick_masked.hip's builds, launched for a part under DM_KEEP_FREE_SLOTS:
// dm_split_form.h): a steady build that also takes an item whose hint word carries the
// released-row bit, with no arrival bit and at least one live row.  With no arrival, lapse or
// recompute Clean releases nothing there either: the masked rows hold zeros, the live rows are
// valid & ~mask, all with the hint's subclient count, and the running sums are the ones read --
// the steady argument with one more register.  A masked row takes the map's not-live path: a
// gets of +0.0 against the +0.0 it holds, and put_released with kSubReleased, which stores
// nothing more in a writeback tick.
template <int G, int R, int MODE = kMixed, Build BUILD = 0u>
__device__ __forceinline__ void group_segment(const DevParams& p, const WorkItem wi, WorkItem* item, int t,
                                              Lds<G>& lds, int32_t* general_list, int32_t* general_count,
                                              int32_t* queue = nullptr, int32_t* qcount = nullptr,
                                              int32_t qidx = 0, int32_t* guard = nullptr, int qcap = 0,
                                              FixKey* key = nullptr, const FixKey fk = FixKey{0, 0, 0},
                                              int use_keys = 0, CycAux* aux = nullptr,
                                              const CycAux ax = CycAux{0, 0, 0}, int probe = 0, int carry = 0) {
  // the dense state (below): every workgroup kernel tracks it and writes the hints;
  // only the 128-thread mixed kernel and the dense-only kernels load by the hint
  constexpr bool kDense = G >= 128 || (G == 64 && R >= 16);  // (64 x 16: kBin4Wave)
  constexpr bool kHintLoad = (G == 128 && MODE == kMixed) || MODE == kDenseOnly;
  constexpr bool SKIP = has_build(BUILD, kSkip), STEADY = has_build(BUILD, kSteady), FIXED = has_build(BUILD, kFixed),
                 LIST = has_build(BUILD, kList), CYCLE = has_build(BUILD, kCycle), MASKED = has_build(BUILD, kMasked);
  static_assert(!STEADY || MODE == kDenseOnly, "kSteady: a dense-only build");
  static_assert(!FIXED || (SKIP && STEADY), "kFixed: a steady build that skips unchanged stores");
  static_assert(!CYCLE || (FIXED && LIST), "kCycle: a list build of the fixed-point build");
  static_assert(!MASKED || STEADY, "kMasked: a steady build");
  const int seg = wi.seg;
  const int64_t lo = wi.lo;
  const int n = kDense ? wi.n & 0xFFFF : wi.n;
  // wave-uniform bases + 32-bit per-lane offsets: one VGPR addresses every column
  const double* __restrict__ wb = p.wants + lo;
  const double* __restrict__ hb = p.has + lo;
  const int32_t* __restrict__ sb = p.sub + lo;
  const int64_t* __restrict__ eb = p.expiry + lo;
  // the rows stay in VGPRs for every pass: 6 registers per row
  double w[R], h[R];
  int s[R];   // subclients in [0, kSubMax]
  int sr[R];  // the raw subclients words: where each row's expiry lives (dm_device.h)
  unsigned valid = 0, live = 0;
  unsigned relm = 0;  // rows a dense resource's mask says are released (bit k: row k*G + t)
  unsigned relb = 0;  // rows whose subclients word marks them released
  // Every load is issued before any is consumed: lanes past the segment end
  // re-read row n-1 (same cache line, n >= 1 in every bin) instead of branching
  // around the load, which made the compiler wait on each row's expiry before
  // issuing the next row (R serial memory latencies per workgroup).
  // A dense resource (every row a live follower with the same subclients s0, the
  // state its last writeback tick left: dm_device.h) is not read from the
  // subclients column: 24 B per lease instead of 28.  The work item carries the
  // state as a hint (no dependent load before the rows); the resource's own byte,
  // loaded with its record, confirms it, and a stale hint (an upsert or release
  // since that tick) reads the column after all.  The 128-thread mixed kernel
  // (257-1024 rows) loads by the hint; the 256/512-thread mixed kernels (1025-4096
  // rows) only track the state and write the hints (the extra branch costs
  // registers they do not have: spills at 5 waves per SIMD, C2 +3.5 %), and their
  // dense-only kernels skip the column.
  // A dense resource may also hold released rows (C2: loaded leases that had lapsed):
  // its hint word carries "has released rows" (bit 8) and the tick that set it wrote
  // which rows they are, one mask entry of R bits per lane (RelMask), read here in
  // place of the column: 1-2 B per lane instead of 4 B per row.
  const int hw = kDense ? wi.n >> 16 : 0;  // hint word: s0 in bits 0-7, released rows in bit 8, arrivals in bit 9
  const int hint = (kHintLoad) ? hw & 0xFF : 0;
  using MaskT = typename RelMask<R>::T;
  MaskT* const mrow = reinterpret_cast<MaskT*>(p.rmask + rel_mask_offset(lo));
  // rows upserted since the dense state was set (dm_device.h mask_pos): the high nibble
  // of the released-row entry for R <= 4, else G entries after the released-row ones
  constexpr unsigned kRowBits = R >= 32 ? ~0u : (1u << R) - 1u;
  const bool arrivals = !STEADY && kDense && ((hw >> 9) & 1);
  bool by_hint = MODE == kDenseOnly;  // the rows' states come from the hint and the masks, not the column
  // kFixed (k_block_dense's build for a steady part ticking in place, dm_tick.cpp): an item
  // whose key is valid, in a launch that uses the keys, issues no row load before its
  // record has confirmed or refuted the key (below); every other item loads first, as ever.
  const bool keyed = FIXED && use_keys && fk.valid;
  if (FIXED && keyed) {
    // (the loads follow the record on a mismatch)
  } else if (MODE != kDenseOnly && !hint) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int i = k * G + t;
      const unsigned u = (unsigned)(i < n ? i : n - 1);
      // plain loads: non-temporal loads measured 3-4% slower (tools/ab.py, C1 and C3)
      w[k] = *col_at(wb, u);
      h[k] = *col_at(hb, u);
      sr[k] = *col_at(sb, u);
    }
  } else {
    // (MASKED: with the rows, no dependent load -- the address comes from wi.lo alone)
    if ((!STEADY || MASKED) && (hw >> 8 & 1)) relm = (unsigned)mrow[t] & kRowBits;
    by_hint = true;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int i = k * G + t;
      const unsigned u = (unsigned)(i < n ? i : n - 1);
      w[k] = *col_at(wb, u);
      h[k] = *col_at(hb, u);
      sr[k] = hint;  // uniform: the mask's rows are taken out below (one register, not R)
    }
  }
  // CYCLE: the destination rows of a probing item, in flight with the others (16 more
  // registers for R = 8 while they wait; profiles/cycle_isa.md has each build's count)
  [[maybe_unused]] double d[CYCLE ? R : 1];
  if constexpr (CYCLE) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int i = k * G + t;
      const unsigned u = (unsigned)(i < n ? i : n - 1);
      d[k] = probe ? *col_at((const double*)p.out_gets + lo, u) : 0.0;
    }
  }
  const Res rs = LIST ? uniform(load_res(p, seg)) : load_res(p, seg);
  // arrivals outlive the followers (at or after follow_exp): only a tick past follow_exp
  // needs their own expiries, from the columns
  const bool arr_lapse = arrivals && p.now > rs.follow_exp;
  if constexpr (MODE == kDenseOnly) {
    // STEADY (k_block_dense's steady builds, launched when the host knows of no released
    // row, arrival or recompute in the part: dm_tick.cpp): an item with a released-row
    // or arrival bit after all, or whose followers have lapsed (lease lengths change on
    // the device, so only the kernel can tell), goes to k_block_rest like a stale hint.
    // What is left has a known Clean (below), with no row examined.
    const bool stale = dense_subclients(rs) != hint;
    // (steady_rest<MASKED>, written out and equal to it: behind the call the compiler orders
    // the test's terms differently and the unmasked steady builds' code moves)
    const bool rest = STEADY ? stale || (hw >> 8 & (MASKED ? 2 : 3)) != 0 || p.now > rs.follow_exp || p.recompute ||
                                   (MASKED && rs.agg_count == 0)
                             : stale || arr_lapse;
    if (rest) {  // stale hint: k_block_rest reads the column
      if (t == 0) hand_off<FIXED>(key, fk, use_keys, queue, qcount, 0, qidx, qcap, guard);
      return;
    }
    if constexpr (FIXED) {
      if (keyed) {
        // The key's tick computed with this capacity and kind, outside learning mode, from
        // the rows, running sums and state that are still there (FixKey): this tick would
        // store no gets, reduce a delta of +0.0 and write the sums it read.  It writes the
        // record as the full path would and is done.
        if (key_holds(fk, rs)) {
          if (t == 0) write_fixed(p, seg, rs, hint);
          return;
        }
        if (MASKED && (hw >> 8 & 1)) relm = (unsigned)mrow[t] & kRowBits;
#pragma unroll
        for (int k = 0; k < R; ++k) {  // refuted (the capacity or kind moved): one memory latency later than usual
          const int i = k * G + t;
          const unsigned u = (unsigned)(i < n ? i : n - 1);
          w[k] = *col_at(wb, u);
          h[k] = *col_at(hb, u);
          sr[k] = hint;
        }
      }
    }
  } else if (kHintLoad && hint && (dense_subclients(rs) != hint || arr_lapse)) {
    relm = 0;  // the column says which rows are released now
    by_hint = false;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int i = k * G + t;
      sr[k] = *col_at(sb, (unsigned)(i < n ? i : n - 1));
    }
  }
  // Followers expire with their resource; only a resource whose rows may carry an
  // explicit expiry (loaded / upserted by the host, none after a writeback tick)
  // reads the 8-B expiry column.  The test is the resource's flag, not the rows'
  // subclients words, which would make every wave wait for its loads to decide.
  int64_t e[R];
  if constexpr (STEADY) {  // every row a live follower of hint subclients: no expiry, no released row
#pragma unroll
    for (int k = 0; k < R; ++k) {
      valid |= ((k * G + t < n) ? 1u : 0u) << k;
      s[k] = hint;
    }
    live = MASKED ? valid & ~relm : valid;  // (MASKED: the mask's rows are released and hold zeros)
  } else {
#pragma unroll
    for (int k = 0; k < R; ++k) e[k] = rs.follow_exp;
    if (MODE != kDenseOnly && (any_explicit(rs) || arr_lapse)) {  // a dense resource: only its lapsing arrivals
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int i = k * G + t;
        const int64_t x = *col_at(eb, (unsigned)(i < n ? i : n - 1));
        if (sub_explicit(sr[k])) e[k] = x;
      }
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {  // rows past the end stay out of valid/live, so every pass skips them
      const unsigned vk = (k * G + t < n) ? 1u : 0u;
      valid |= vk << k;
      if (sub_released(sr[k])) e[k] = kReleased;
      live |= (vk & (p.now > e[k] ? 0u : 1u)) << k;  // store.go:174 when.After(expiry)
      relb |= (sub_released(sr[k]) ? 1u : 0u) << k;
      s[k] = sub_value(sr[k]);
    }
    live &= ~relm;
  }

  // ---- pass A: Clean ----
  // STEADY: Clean releases nothing (exact zeros: nothing is ever added) and every row is
  // live with hint subclients, so the loop, its reduction and its barrier are left out.
  // Only "any NaN wants" depends on the rows: FairShare (the one user) counts them with
  // pass B's reduction, in bits 48 and up of AggB::i (the sum itself stays below 2^43).
  AggA a = zeroA();
  if constexpr (STEADY) {
    a.smin = a.smax = hint;
    a.nlive = n;
  } else {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if (!(valid >> k & 1)) continue;
      const bool lv = live >> k & 1;
      const int sk = (relm >> k & 1) ? 0 : s[k];  // a released row counts nothing (its wants and has are 0)
      if (!lv) {
        a.cnt += sk;
        a.h += h[k];
        a.w += w[k];
      }
      if (p.recompute) {
        a.all.cnt += sk;
        a.all.h += h[k];
        a.all.w += w[k];
      }
      if (lv) {
        a.smin = s[k] < a.smin ? s[k] : a.smin;
        a.smax = s[k] > a.smax ? s[k] : a.smax;
        a.nan |= __builtin_isnan(w[k]) ? 1 : 0;
        a.nlive += 1;
      }
    }
  }
  if constexpr (!STEADY) {
    const AggR all_part = a.all;
    bool fast_a = false;
    if constexpr (G <= 64) {
      // Sub-wave and wave groups are VALU-bound on their reductions.  In the steady
      // state pass A's totals are known wave-wide without one: no row of the wave is
      // released by this Clean (rows already marked released hold zeros), its live
      // rows share one subclient count u, no wants is NaN.  Then every group's Clean
      // sums are exact zeros and its live range is [u, u] (empty: no live row).
      if (!p.recompute) {
        const uint64_t lv = __ballot(live != 0);
        const int u = __builtin_amdgcn_readlane(a.smin, lv ? (int)__builtin_ctzll(lv) : 0);
        const bool ok = (valid & ~live & ~relb) == 0 && a.cnt == 0 && __double_as_longlong(a.h) == 0 &&
                        __double_as_longlong(a.w) == 0 && !a.nan && (live == 0 || (a.smin == u && a.smax == u));
        if (__all(ok)) {
          fast_a = true;
          const int base = (int)(threadIdx.x & 63) & ~(G - 1);
          uint64_t gmask = ~0ull;
          if constexpr (G < 64) gmask = ((1ull << G) - 1) << base;
          const bool any_live = (lv & gmask) != 0;
          a.smin = any_live ? u : INT32_MAX;
          a.smax = any_live ? u : INT32_MIN;
        }
      }
    }
    if (!fast_a) a = group_reduce<G, AggA, OpA, false>(a, OpA(), lds.a);
    if (p.recompute) a.all = group_reduce<G, AggR, OpR, false>(all_part, OpR(), lds.r);
  }
  // (STEADY: the running sums as they are; never in recompute mode)
  const Clean cl = STEADY ? Clean{rs.agg_count, rs.agg_has, rs.agg_wants} : clean_from(p, rs, a);
  const double C = rs.C;
  const double eq = C / (double)cl.count;  // algorithm.go:123,229 equalShare
  const bool ps = !rs.learning && rs.kind == 2;
  const bool fs = !rs.learning && rs.kind == 3;
  const bool fs_uniform = fs && a.smin >= a.smax && !a.nan;  // no live rows counts as uniform
  constexpr long long kNanOne = 1ll << 48;  // STEADY: a NaN wants in AggB::i
  if (!STEADY && fs && !fs_uniform) {
    // heterogeneous subclients (GetServerCapacity, server.go:850-879) or NaN wants:
    // one round-2 threshold per distinct subclient count.  Rare (the hierarchy's
    // root level), so the whole resource goes to k_general, untouched here.
    if (t == 0) {
      general_list[atomicAdd(general_count, 1)] = seg;
      if (p.writeback && (wi.n >> 16)) item->n = n;  // k_general's writeback clears the byte
    }
    return;
  }

  // ---- pass B: ProportionalShare extraCapacity/extraNeed, FairShare round 1 ----
  AggB b{0.0, 0.0, 0};
  if (ps || fs) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if (!(live >> k & 1)) continue;
      if (ps) {
        const double e = eq * (double)s[k];  // :273
        if (w[k] < e)
          b.x += e - w[k];  // :275
        else
          b.y += w[k] - e;  // :277
      } else {
        const double d = (double)s[k] * eq;  // :160
        if (w[k] < d)
          b.x += d - w[k];  // :164
        else if (w[k] > d)
          b.i += s[k];  // :168
        if constexpr (STEADY) b.i += __builtin_isnan(w[k]) ? kNanOne : 0;  // (adds to neither sum above)
      }
    }
    b = group_reduce<G, AggB, OpB, false>(b, OpB(), lds.b);
    if constexpr (STEADY) {
      if (b.i >= kNanOne) {  // FairShare with a NaN wants: k_general, as above (nothing is stored yet)
        if (t == 0) {
          if constexpr (FIXED) put_key(key, fk, use_keys, false, 0.0, 0);  // before the hand-off
          general_list[atomicAdd(general_count, 1)] = seg;
          if (p.writeback && (wi.n >> 16)) item->n = n;
        }
        return;
      }
    }
  }

  // ---- pass C (uniform subclients): FairShare round 2 at the resource's one threshold ----
  AggC cu{0.0, 0};
  FsU fu{0.0, 0.0, 0.0, 0.0, 0.0};
  if (fs_uniform) {
    fu = make_fsu(eq, a.smin, b.x, b.i, cu);
    const double Tu = fu.T;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if (!(live >> k & 1)) continue;
      if (!(w[k] > (double)s[k] * eq)) continue;  // j in wantExtraClients (:165-169)
      if (w[k] < Tu)
        cu.ee += Tu - w[k];  // :197-198
      else if (w[k] > Tu)
        cu.sgt += s[k];  // :199-200
    }
    cu = group_reduce<G, AggC, OpC, false>(cu, OpC(), lds.c);
    fu = make_fsu(eq, a.smin, b.x, b.i, cu);
    if constexpr (G >= 64) fu = uniform(fu);  // one resource per wave or workgroup: SGPRs
  }

  // ---- map: decide and write every lease (store.go:153-167 Assign) ----
  // SKIP (k_block_dense's second build, launched for a writeback tick in place: out_gets
  // is the column h[] was loaded from) leaves out the gets store of a wave's 64-row run
  // (512 B) when no row of the run changes: on a resource at its fixed point (no wants
  // change, arrival, departure or capacity change since the last tick) the value is bit
  // for bit the has just loaded, a third of the tick's bytes.  Bits, not values (-0.0,
  // NaN payloads); a row Clean releases stores +0.0.  The ballot runs among the run's
  // valid rows (lanes past n do not vote), so the store's branch is wave-uniform: whole
  // runs, no partial lines.  The comparison reuses h[k] (live for delta) and leaves a
  // scalar mask.  Every other store (subclients, wants of released rows, masks, the
  // resource) stays.  Never on a non-writeback tick or on the alternate column, which
  // holds the tick before last: those run the build without it, the loop as it always was.
  SumD delta{0.0};
  bool stored = false;  // FIXED: some run of this wave's gets is stored (wave-uniform)
#pragma unroll
  for (int k = 0; k < R; ++k) {
    if (!(valid >> k & 1)) continue;
    const unsigned u = (unsigned)(k * G + t);
    if constexpr (SKIP) {
      const bool lv = live >> k & 1;
      const double g = lv ? row_gets(rs, ps, C, eq, cl, b, fu, w[k], h[k], s[k]) : 0.0;
      bool st;
      if constexpr (CYCLE)
        st = !probe || __ballot(__double_as_longlong(g) != __double_as_longlong(d[k])) != 0;
      else
        st = __ballot(__double_as_longlong(g) != __double_as_longlong(h[k])) != 0;
      if constexpr (FIXED) stored |= st;
      if (!lv) {  // released by Clean: no lease
        put_released<kGroupNT<G>>(p, lo, u, (relm >> k & 1) ? (int)kSubReleased : sr[k], st);
        continue;
      }
      put_live<kGroupNT<G>>(p, lo, u, g, rs, sr[k], st);
      delta.v += g - h[k];
      continue;
    }
    if (!(live >> k & 1)) {  // released by Clean: no lease
      put_released<kGroupNT<G>>(p, lo, u, (relm >> k & 1) ? (int)kSubReleased : sr[k]);
      continue;
    }
    double g;
    if (rs.learning) {
      g = h[k];  // Learn (algorithm.go:297-302)
    } else if (rs.kind == 0) {
      g = w[k];  // NoAlgorithm
    } else if (rs.kind == 1) {
      g = minF(C, w[k]);  // Static
    } else if (ps) {
      const double epc = eq * (double)s[k];         // :233
      const double unused = C - cl.sum_has + h[k];  // :239
      g = (cl.sum_wants <= C || w[k] <= epc) ? minF(w[k], unused)            // :245
                                             : minF(epc + (w[k] - epc) * (b.x / b.y), unused);  // :283
    } else {
      g = fs_uniform_row(w[k], h[k], C, cl.sum_has, fu);
    }
    put_live<kGroupNT<G>>(p, lo, u, g, rs, sr[k]);
    delta.v += g - h[k];
  }
  // (uniform) the live arrivals of a dense resource decided by the hint become followers:
  // their explicit subclients words are rewritten (the arrival mask is loaded only here,
  // so a store without arrivals carries no register for it)
  unsigned arrm = 0;
  if (arrivals && by_hint) {
    arrm = R <= 4 ? ((unsigned)mrow[t] >> 4) & kRowBits : (unsigned)mrow[G + t];
    if (p.writeback) {
#pragma unroll
      for (int k = 0; k < R; ++k)
        if ((arrm & live) >> k & 1) *col_at(p.out_sub + lo, (unsigned)(k * G + t)) = hint;
    }
  }

  // After a writeback tick every live row follows the resource and every other row
  // is released: live rows with one subclient count s0 (1..254) make the resource
  // dense.  Released rows among them go into its mask (written by the tick that sets
  // the state; a dense tick leaves the state as it found it or, when the followers
  // lapse together, ends it).
  // A resource with no live row left (its followers lapsed together) stays dense,
  // every row in its mask, so that a dense tick always leaves a dense resource dense
  // (the host's skip of the rest kernel rests on it: dm_tick.cpp).
  const int nlive = a.nlive;
  const int s_keep = (hw & 0xFF) ? (hw & 0xFF) : 1;
  const int dn = !(kDense && p.writeback) ? 0
                 : nlive == 0              ? s_keep
                 : (a.smin == a.smax && a.smin >= 1 && a.smin <= 254) ? a.smin : 0;
  const int hw_next = dn ? (dn | (nlive < n ? 1 << 8 : 0)) : 0;
  if constexpr (FIXED) {
    // the delta's reduction in group_reduce's order, each wave's "stored a run" beside its
    // partial behind the same barrier; then the key: the item is at its fixed point when
    // no wave stored a run, the delta is +0.0 as bits and the sums written are the sums
    // read (count and sum_wants are, in a steady build), outside learning mode
    delta = wave_reduce_g<(G < 64 ? G : 64)>(delta, OpSumD());
    int any = stored ? 1 : 0;
    if constexpr (G > 64) {
      if ((t & 63) == 0) lds.dn[t >> 6] = SumDN{delta.v, any, 0};
      __syncthreads();
      SumDN r = lds.dn[0];
#pragma unroll 3
      for (int i = 1; i < G / 64; ++i) {
        const SumDN x = lds.dn[i];
        r = SumDN{r.v + x.v, r.n | x.n, 0};
      }
      delta.v = r.v;
      any = r.n;
    }
    if constexpr (CYCLE) {
      // the key after a cycle-form tick: state 2 when the probe stored no run and the sum
      // written is the one from before the last tick; else state 1 (every row of the item
      // is in the column written or was equal there).  Both sums of a valid key must
      // survive the sweep's `+ 0.0` (write_resource): never -0.0 or a signalling NaN.
      if (t == 0) {
        write_resource(p, seg, rs, cl, delta.v, hint);
        const uint64_t was = (uint64_t)__double_as_longlong(rs.agg_has);
        const uint64_t now_has = (uint64_t)__double_as_longlong(cl.sum_has + delta.v);
        const bool stable = (uint64_t)__double_as_longlong(__longlong_as_double((long long)now_has) + 0.0) == now_has &&
                            (uint64_t)__double_as_longlong(rs.agg_has + 0.0) == was;
        const bool ok = probe && !any && now_has == ax.prev_has && stable && !rs.learning;
        int wait = 0, skip = 0;
        if (!ok && probe) {
          wait = ax.wait < 1 ? 1 : (2 * ax.wait > kCycleProbeWaitMax ? kCycleProbeWaitMax : 2 * ax.wait);
          skip = wait;
        } else if (!ok && carry) {
          wait = ax.wait;
          skip = ax.skip;
        }
        const bool rec = !rs.learning;
        *key = FixKey{rec ? (uint64_t)__double_as_longlong(C) : 0ull, rec ? rs.kind : 0, rec ? (ok ? 2 : 1) : 0};
        *aux = CycAux{was, wait, skip};
      }
      return;
    }
    if (t == 0) {
      write_resource(p, seg, rs, cl, delta.v, hint);
      const bool fix = !any && __double_as_longlong(delta.v) == 0 &&
                       __double_as_longlong(cl.sum_has + delta.v) == __double_as_longlong(rs.agg_has) && !rs.learning;
      put_key(key, fk, use_keys, fix, C, rs.kind);
    }
    return;
  }
  delta = group_reduce<G, SumD, OpSumD, false>(delta, OpSumD(), lds.d);
  if constexpr (STEADY) {  // the state stays as it is: dn == hint, hw_next == hw, no mask to write
    if (t == 0) write_resource(p, seg, rs, cl, delta.v, hint);
    return;
  }
  // A dense tick changes the mask only by a lapse; a writeback tick that changes the
  // state word writes it whole (a later release ORs its row in, so it must be valid
  // whenever the hint is set) and clears the arrivals it turned into followers.
  if (kDense && (MODE == kDenseOnly ? nlive == 0 || (p.writeback && hw != hw_next)
                                    : (hw_next >> 8) != 0 || (p.writeback && hw != hw_next))) {
    // (R <= 4: a non-writeback tick keeps the arrivals' nibble)
    mrow[t] = (MaskT)((valid & ~live) | (R <= 4 && !p.writeback ? arrm << 4 : 0u));
    if (R > 4 && arrivals && p.writeback) mrow[G + t] = 0;
  }
  if (t == 0) {
    write_resource(p, seg, rs, cl, delta.v, dn);
    if (p.writeback && hw != hw_next) item->n = n | hw_next << 16;
  }
}

// The workgroup bins' shapes, G threads x R rows per thread: the one list behind every
// per-bin launcher.  Calls f(integral_constant<int, G>, integral_constant<int, R>);
// false: no such bin.
template <int G, int R, typename F>
bool as_bin_shape(F& f) {
  f(std::integral_constant<int, G>{}, std::integral_constant<int, R>{});
  return true;
}
template <typename F>
bool with_bin_shape(int bin, F&& f) {
  switch (bin) {
    case 3: return as_bin_shape<128, 4>(f);
    case 4: return as_bin_shape<128, 8>(f);
    case kBin4Wave: return as_bin_shape<64, 16>(f);
    case 5: return as_bin_shape<256, 8>(f);
    case 6: return as_bin_shape<256, 16>(f);
    case kBin6Wide: return as_bin_shape<512, 8>(f);
    default: return false;
  }
}
// f(bool_constant<B>) for a runtime b
template <typename F>
void with_bool(bool b, F&& f) {
  if (b)
    f(std::true_type{});
  else
    f(std::false_type{});
}

}  // namespace dm
