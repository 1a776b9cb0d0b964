// The cases of tests/test_update_outcome.py: dm_update_outcome.h alone, against a
// transcription of the three places that mapped a store update's flags before the header
// existed (dm_store_update.cpp: finish_update with the single calls' tails, the tail of
// dm_store_update_wants_mask, and apply_check).
// First line: `cases <n> disagreements <n> (single <cases> batch <cases>)`: every flags word
// its call's kernels can set (for a batch: every triple of such words, with the reject bits a
// word carries from the one before), both prior values of maybe_general and all_sub_one, and
// for a batch arrivals or none and late or not; a case disagrees when the code, the message or
// either resulting boolean differs.  Then one line per named case:
//   <case> code=<code> general=<0|1> sub_one=<0|1> "<message>"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dm_update_outcome.h"

using namespace dm;

struct Result {
  int code = DM_OK;
  std::string msg;
  bool general = false, sub_one = true;
  bool operator==(const Result& o) const {
    return code == o.code && msg == o.msg && general == o.general && sub_one == o.sub_one;
  }
};

// ---- the earlier code, transcribed (c->fail(code, msg) returns the code and keeps the message) ----
static int old_finish_update(uint32_t f, Result& r) {
  auto fail = [&](int code, const char* msg) { r.msg = msg; return code; };
  if (f & kUpdRange) return fail(DM_E_RANGE, "row out of range");
  if (f & kUpdDup) return fail(DM_E_INVAL, "rows must be unique within one call");
  if (f & kUpdSub) return fail(DM_E_INVAL, "subclients must be in [0, 2^31-2]");
  return DM_OK;
}
static Result old_single(UpdPart p, uint32_t f, bool general, bool sub_one) {
  Result r;
  r.general = general, r.sub_one = sub_one;
  if (p == UpdPart::refresh_mask) {  // the tail of dm_store_update_wants_mask
    if (f & kUpdRange) return r.code = DM_E_RANGE, r.msg = "mask bit past the store's end", r;
    if (f & kUpdCount) return r.code = DM_E_INVAL, r.msg = "packed values must match the mask's set bits", r;
    if (f & kUpdNaN) r.general = true;
    return r;
  }
  r.code = old_finish_update(f, r);
  if (r.code) return r;
  if (p == UpdPart::upsert) {  // dm_store_upsert
    if ((f & (kUpdNaN | kUpdNotOne)) || !r.sub_one) r.general = true;
    if (f & kUpdNotOne) r.sub_one = false;
  } else if (p == UpdPart::refresh) {  // dm_store_update_wants
    if (f & kUpdNaN) r.general = true;
  }
  return r;
}
static Result old_apply_check(const uint32_t* h_flags, int64_t nu, bool late, bool general, bool sub_one) {
  Result r;
  r.general = general, r.sub_one = sub_one;
  const uint32_t f0 = h_flags[0], f1 = h_flags[1], f2 = h_flags[2];
  auto fail = [&](int code, const std::string& msg) { r.msg = msg; return code; };
  auto reject = [&](uint32_t f, const char* part) -> int {
    const std::string p = std::string(late ? "an earlier asynchronous batch's " : "") + part;
    if (f & kUpdRange) return fail(DM_E_RANGE, p + ": row out of range");
    if (f & kUpdCount) return fail(DM_E_INVAL, p + ": packed values must match the mask's set bits");
    if (f & kUpdDup) return fail(DM_E_INVAL, p + ": rows must be unique within one part");
    return fail(DM_E_INVAL, p + ": subclients must be in [0, 2^31-2]");
  };
  if (f0 & kUpdReject) return r.code = reject(f0, "wants refresh"), r;
  if (f0 & kUpdNaN) r.general = true;
  if (f1 & kUpdReject) return r.code = reject(f1, "release"), r;
  if (f2 & kUpdReject) return r.code = reject(f2, "upsert"), r;
  if (nu > 0) {
    if ((f2 & (kUpdNaN | kUpdNotOne)) || !r.sub_one) r.general = true;
    if (f2 & kUpdNotOne) r.sub_one = false;
  }
  return r;
}

// ---- the header ----
static Result new_single(UpdPart p, uint32_t f, bool general, bool sub_one) {
  Result r;
  r.general = general, r.sub_one = sub_one;
  const UpdOutcome o = update_outcome(p, f, false);  // as a single call's end asks (dm_store_update.cpp single_end)
  if (o.code == DM_OK) update_values(p, f, r.general, r.sub_one);
  r.code = o.code, r.msg = o.msg;
  return r;
}
static Result new_batch(const uint32_t* f, int64_t nu, bool late, bool general, bool sub_one) {
  Result r;
  r.general = general, r.sub_one = sub_one;
  const UpdOutcome o = batch_outcome(f, nu > 0, late, r.general, r.sub_one);
  r.code = o.code, r.msg = o.msg;
  return r;
}

// the bits each part's kernels can set (the header's table)
static constexpr uint32_t kUpsertBits = kUpdRange | kUpdDup | kUpdSub | kUpdNaN | kUpdNotOne;
static constexpr uint32_t kRefreshBits = kUpdRange | kUpdDup | kUpdNaN;
static constexpr uint32_t kReleaseBits = kUpdRange | kUpdDup;
static constexpr uint32_t kMaskBits = kUpdRange | kUpdCount | kUpdNaN;

static std::vector<uint32_t> subsets(uint32_t bits) {
  std::vector<uint32_t> v;
  for (uint32_t f = 0; f < 64; ++f)
    if ((f & ~bits) == 0) v.push_back(f);
  return v;
}

static void show(const char* name, const Result& r) {
  printf("%s code=%d general=%d sub_one=%d \"%s\"\n", name, r.code, r.general, r.sub_one, r.msg.c_str());
}
static void batch(const char* name, uint32_t f0, uint32_t f1, uint32_t f2, int64_t nu, bool late) {
  // as the device leaves them: each word carries the reject bits of the one before
  f1 |= f0 & kUpdReject;
  f2 |= f1 & kUpdReject;
  const uint32_t f[3] = {f0, f1, f2};
  show(name, new_batch(f, nu, late, false, true));
}

int main() {
  long single_cases = 0, batch_cases = 0, bad = 0;
  static const struct {
    UpdPart p;
    uint32_t bits;
  } singles[] = {{UpdPart::upsert, kUpsertBits},
                 {UpdPart::refresh, kRefreshBits},
                 {UpdPart::release, kReleaseBits},
                 {UpdPart::refresh_mask, kMaskBits}};
  for (const auto& s : singles)
    for (uint32_t f : subsets(s.bits))
      for (int prior = 0; prior < 4; ++prior) {
        ++single_cases;
        bad += !(old_single(s.p, f, prior & 1, prior & 2) == new_single(s.p, f, prior & 1, prior & 2));
      }
  // a batch: own bits per word, plus what k_carry_reject brings from the word before
  for (uint32_t o0 : subsets(kMaskBits))
    for (uint32_t o1 : subsets(kReleaseBits))
      for (uint32_t o2 : subsets(kUpsertBits)) {
        const uint32_t f1 = o1 | (o0 & kUpdReject);
        const uint32_t f[3] = {o0, f1, o2 | (f1 & kUpdReject)};
        for (int64_t nu : {0, 7})
          for (int late = 0; late < 2; ++late)
            for (int prior = 0; prior < 4; ++prior) {
              ++batch_cases;
              bad += !(old_apply_check(f, nu, late, prior & 1, prior & 2) == new_batch(f, nu, late, prior & 1, prior & 2));
            }
      }
  printf("cases %ld disagreements %ld (single %ld batch %ld)\n", single_cases + batch_cases, bad, single_cases,
         batch_cases);

  show("upsert_ok", new_single(UpdPart::upsert, 0, false, true));
  show("upsert_not_one", new_single(UpdPart::upsert, kUpdNotOne, false, true));
  show("upsert_ones_into_mixed_store", new_single(UpdPart::upsert, 0, false, false));
  show("upsert_nan", new_single(UpdPart::upsert, kUpdNaN, false, true));
  show("upsert_bad_subclients", new_single(UpdPart::upsert, kUpdSub | kUpdNotOne, false, true));
  show("upsert_duplicate_row", new_single(UpdPart::upsert, kUpdDup, false, true));
  show("upsert_range_and_duplicate", new_single(UpdPart::upsert, kUpdRange | kUpdDup | kUpdNaN, false, true));
  show("refresh_nan", new_single(UpdPart::refresh, kUpdNaN, false, true));
  show("refresh_duplicate_row", new_single(UpdPart::refresh, kUpdDup | kUpdNaN, false, true));
  show("release_duplicate_row", new_single(UpdPart::release, kUpdDup, false, true));
  show("release_row_out_of_range", new_single(UpdPart::release, kUpdRange, false, true));
  show("mask_bit_past_end", new_single(UpdPart::refresh_mask, kUpdRange | kUpdCount, false, true));
  show("mask_count_mismatch", new_single(UpdPart::refresh_mask, kUpdCount, false, true));
  show("mask_nan", new_single(UpdPart::refresh_mask, kUpdNaN, false, true));
  batch("batch_ok", 0, 0, 0, 5, false);
  batch("batch_refresh_nan", kUpdNaN, 0, 0, 0, false);
  batch("batch_count_mismatch_carried_into_upsert", kUpdCount, 0, kUpdNotOne, 5, false);
  batch("batch_release_duplicate", 0, kUpdDup, 0, 5, false);
  batch("batch_release_duplicate_after_refresh_nan", kUpdNaN, kUpdDup, kUpdNotOne, 5, false);
  batch("batch_upsert_bad_subclients", 0, 0, kUpdSub | kUpdNotOne, 5, false);
  batch("batch_upsert_range_after_clean_parts", 0, 0, kUpdRange, 5, false);
  batch("batch_upsert_not_one", 0, 0, kUpdNotOne, 5, false);
  batch("batch_no_arrivals_word_ignored", 0, 0, kUpdNotOne, 0, false);
  batch("late_nan", kUpdNaN, 0, 0, 0, true);
  batch("late_upsert_nan", 0, 0, kUpdNaN, 5, true);
  batch("late_mask_bit_past_end", kUpdRange, 0, 0, 0, true);
  batch("late_release_duplicate", 0, kUpdDup, 0, 5, true);
  batch("late_upsert_duplicate", 0, 0, kUpdDup, 5, true);
  return 0;
}
