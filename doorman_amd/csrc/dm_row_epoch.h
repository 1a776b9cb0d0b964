// dm_row_epoch.h — which calls that write rows start a row epoch (dm_ctx::rows_changed),
// and which update-kernel build a wants refresh launches.  Plain C++17, no HIP: the rule is
// tested on the CPU (tests/test_row_epoch.py).
//
// Two counters (dm_ctx.h): the write epoch moves with every call that writes a row, the row
// epoch only with rows_changed().  Within one row epoch the fixed-point keys of a part stay
// in use, its density verification stays valid and a large store's writeback ticks stay in
// place (dm_split_form.h, dm_tick.cpp Tick::outputs); the write epoch is what the large
// chain's light redo asks (no row written since the last speculative tick).
//
// Every writer ends as rows_changed() except one: with dm_keep_keys on, a wants refresh
// (dm_store_update_wants, dm_store_update_wants_mask) that was neither rejected nor carried
// a NaN is *kept*.  Such a refresh writes wants and adds to sum_wants, nothing else: no
// subclients word, expiry, state byte, mask or work item.  So
//   - no dense resource stops being dense, and none gains a released row or an arrival: the
//     part's density record (SplitSlot::rec) says what it said, and a dense kernel that ran
//     alone (PartForm::skip_rest, the form of a bin in stream parts) still cannot queue an
//     item -- the guard stays for the impossible;
//   - a resource's key is wrong only where a row's wants bits moved, and there the refresh
//     kernel's key-clearing build has stored an invalid key (dm_update.hip), which the sweep
//     and the FIXED builds read as "load the rows".
// A NaN wants can end a resource's dense state (FairShare then needs k_general), so such a
// call starts an epoch as it always did; so does a rejected one, which wrote nothing, and
// every call the refresh's flags are not read in (the batches: the asynchronous one learns
// of a NaN two batches later).
//
// dm_keep_keys' argument is a bit set.  Any non-zero value keeps refreshes, as above
// (kKeepRefresh is the value 1).  kKeepUpdates (2) also keeps dm_store_release,
// dm_store_upsert and the synchronous dm_store_apply, when no part was rejected and none was
// flagged NaN.  Such a call does write subclients words, state bytes, masks and work items,
// and what makes that safe is on the device: every tick kernel that may trust a key or skip a
// pass tests the item first (a hint stale against the state byte, a released-row or arrival
// bit, no hint word: the item's key is cleared and it goes to k_block_rest), and the update
// kernels leave exactly those marks.  Two things follow on the host (dm_split_form.h): the
// steady, FIXED and sweep forms are always followed by the rest launch, so for them the
// density record is a cost estimate and may be a little out of date; the dense kernel that
// runs alone (skip_rest) takes the record as a proof, and a kept update withdraws it until a
// count taken after a later writeback tick (dm_ctx::update_kept, check_dense).  The
// key-clearing builds of the update kernels (k_release_keys, k_upsert_keys) clear the key of
// every workgroup-bin resource of which they write a row: redundant for correctness, it keeps
// FixKey's stated meaning and dm_store_stats' count of valid keys exact right after the call.
// kUpdNotOne does not end the mode: maybe_general / all_sub_one are set as ever and the
// resource's state byte is 1 by then.  Every other writer starts an epoch under either bit.
#pragma once
#include <cstdint>

namespace dm {

enum class RowWrite {
  refresh,       // dm_store_update_wants
  refresh_mask,  // dm_store_update_wants_mask
  load,          // dm_store_load
  plan,          // a new plan (upload_plan)
  upsert,
  release,
  apply,         // dm_store_apply
  apply_async,   // dm_store_apply_async
  decide,
  clean,
  relayout,
  config_load,
  root_tick,     // dm_hier_root_tick
};

constexpr bool is_refresh(RowWrite w) { return w == RowWrite::refresh || w == RowWrite::refresh_mask; }

// Before the launch.  defer: the call decides how it ends once its flags are back
// (row_write_kept_mode); otherwise it calls rows_changed() at once, as every writer did.
// clear_keys: launch the key-clearing build of the refresh kernel.  Only where keys are in
// use (some part's fix_live is the row epoch): keys out of use are rewritten by the next
// FIXED launch before any is read, so every other launch runs the plain kernels.
struct RowWriteStart {
  bool defer = false;
  bool clear_keys = false;
};

// dm_keep_keys' bit set (above).
// kKeepFreeSlots (4) keeps no call: it selects forms alone (dm_split_form.h FormInputs::keep_free,
// PartForm::masked).  A dense workgroup-bin item that holds released rows, with no arrival bit
// and a live row, then runs in the steady, FIXED, sweep and cycle forms' masked builds and keeps
// a key; with the bit clear such an item goes through k_block_rest every tick.
constexpr int kKeepRefresh = 1, kKeepUpdates = 2, kKeepFreeSlots = 4;
constexpr bool is_update(RowWrite w) {
  return w == RowWrite::release || w == RowWrite::upsert || w == RowWrite::apply;
}
constexpr bool mode_keeps(RowWrite w, int mode) {
  return (mode != 0 && is_refresh(w)) || ((mode & kKeepUpdates) && is_update(w));
}
inline RowWriteStart row_write_start_mode(RowWrite w, int mode, bool keys_in_use) {
  RowWriteStart s;
  s.defer = mode_keeps(w, mode);
  s.clear_keys = s.defer && keys_in_use;
  return s;
}

// After the flags are back.  rejected: the call failed or its validation refused it (the
// apply kernel did not run); nan: kUpdNaN.  true: kept (dm_ctx::refresh_kept, update_kept);
// false: rows_changed().
inline bool row_write_kept_mode(RowWrite w, int mode, bool rejected, bool nan) {
  return mode_keeps(w, mode) && !rejected && !nan;
}

}  // namespace dm
