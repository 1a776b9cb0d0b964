// dm_update_outcome.h — what a store update's flags word means: the bits its kernels set
// (dm_update.hip), the error code and message a rejected call returns, and what the value
// bits do to the context's maybe_general / all_sub_one.  Plain C++17, no HIP: the rule is
// tested on the CPU (tests/test_update_outcome.py).  dm_device.h includes it for the bits.
//
// One flags word per single call, three per batch (dm_store_apply: wants refresh, release,
// upsert, in that order).  The bits a word can hold:
//   row upsert      Range, Dup, Sub, NaN, NotOne
//   row refresh     Range, Dup, NaN
//   release         Range, Dup
//   masked refresh  Range, Count, NaN
//   a batch's word  its part's, and the reject bits of the word before (k_carry_reject)
// A word with a reject bit fails the call, and its apply kernel has written nothing.  Which
// bit names the failure: Range, then Count, Dup, Sub.  The messages are what callers match
// on; three wordings depend on who asks, and are meant:
//   - a single masked refresh names rows by mask bits ("mask bit past the store's end"); a
//     row call and every part of a batch say "row out of range";
//   - rows are unique "within one call", or "within one part" of a batch (two parts of one
//     batch may name the same row);
//   - a batch's message starts with its part, and a batch reported by a later call (`late`)
//     with "an earlier asynchronous batch's ".
// Outside the sets above (a Count on an upsert, say) the rule does whatever the one priority
// order gives: no kernel can set such a word.
#pragma once
#include <cstdint>
#include <cstdio>

#include "../../include/doorman_hip.h"

namespace dm {

constexpr uint32_t kUpdRange = 1u;   // row outside [0, N)
constexpr uint32_t kUpdDup = 2u;     // row twice in one call
constexpr uint32_t kUpdSub = 4u;     // subclients outside [0, kSubMax]
constexpr uint32_t kUpdNaN = 8u;     // NaN wants (FairShare then needs k_general)
constexpr uint32_t kUpdNotOne = 16u; // subclients != 1 (may make a resource heterogeneous)
constexpr uint32_t kUpdCount = 32u;  // packed values != set bits of the row mask
constexpr uint32_t kUpdReject = kUpdRange | kUpdDup | kUpdSub | kUpdCount;

enum class UpdPart {
  upsert,        // dm_store_upsert
  refresh,       // dm_store_update_wants
  release,       // dm_store_release
  refresh_mask,  // dm_store_update_wants_mask
  batch_refresh, // a batch's three words, in their order
  batch_release,
  batch_upsert,
};
constexpr bool in_batch(UpdPart p) { return p >= UpdPart::batch_refresh; }
constexpr int flags_word(UpdPart p) { return in_batch(p) ? (int)p - (int)UpdPart::batch_refresh : 0; }
constexpr bool writes_subclients(UpdPart p) { return p == UpdPart::upsert || p == UpdPart::batch_upsert; }
constexpr bool writes_wants(UpdPart p) { return p != UpdPart::release && p != UpdPart::batch_release; }

struct UpdOutcome {
  int code = DM_OK;
  char msg[112] = "";
};

// One word's error code and message (DM_OK and "" for a word without a reject bit).
inline UpdOutcome update_outcome(UpdPart p, uint32_t f, bool late) {
  UpdOutcome o;
  if (!(f & kUpdReject)) return o;
  const char* text = f & kUpdRange   ? (p == UpdPart::refresh_mask ? "mask bit past the store's end" : "row out of range")
                     : f & kUpdCount ? "packed values must match the mask's set bits"
                     : f & kUpdDup   ? (in_batch(p) ? "rows must be unique within one part" : "rows must be unique within one call")
                                     : "subclients must be in [0, 2^31-2]";
  const char* part = p == UpdPart::batch_refresh ? "wants refresh: " : p == UpdPart::batch_release ? "release: " : "upsert: ";
  o.code = f & kUpdRange ? DM_E_RANGE : DM_E_INVAL;
  snprintf(o.msg, sizeof o.msg, "%s%s%s", late ? "an earlier asynchronous batch's " : "", in_batch(p) ? part : "", text);
  return o;
}

// An accepted word's value bits: a NaN wants, or subclients other than one among rows that
// may share a resource with ones, can make a resource need k_general (stay conservative).
inline void update_values(UpdPart p, uint32_t f, bool& maybe_general, bool& all_sub_one) {
  if (writes_wants(p) && (f & kUpdNaN)) maybe_general = true;
  if (!writes_subclients(p)) return;
  if ((f & kUpdNotOne) || !all_sub_one) maybe_general = true;
  if (f & kUpdNotOne) all_sub_one = false;
}

// A landed batch's three words.  The first rejected part fails the call: a later word carries
// that part's reject bits, so the words are asked in order.  The parts before it were applied
// and their values count; the upsert's count when the batch had arrivals (`arrivals`).
inline UpdOutcome batch_outcome(const uint32_t f[3], bool arrivals, bool late, bool& maybe_general, bool& all_sub_one) {
  static constexpr UpdPart parts[3] = {UpdPart::batch_refresh, UpdPart::batch_release, UpdPart::batch_upsert};
  for (int k = 0; k < 3; ++k) {
    const UpdOutcome o = update_outcome(parts[k], f[k], late);
    if (o.code != DM_OK) return o;
    if (k < 2 || arrivals) update_values(parts[k], f[k], maybe_general, all_sub_one);
  }
  return UpdOutcome{};
}

}  // namespace dm
