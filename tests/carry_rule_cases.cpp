// The carried root round's host rule (doorman_amd/csrc/dm_carry_rule.h) on the CPU: every
// combination of the inputs each function mentions checked against a transcription of the rule
// as the issue states it, then the launch order the rule gives over a few steps; one line per
// table for tests/test_carry_rule.py.  Stand-alone: it may be built with
// -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "dm_carry_rule.h"

using namespace dm;

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::printf("FAILED %s (line %d, case %ld)\n", #x, __LINE__, n); \
      std::exit(1);                                                    \
    }                                                                  \
  } while (0)

// carrying: hier_G == 1, the exchange on the leaf's stream, the template pipe on, the switch on
static void carry_table() {
  long n = 0, carried = 0;
  const int servers[3] = {1, 2, 8};
  for (unsigned m = 0; m < 8; ++m)
    for (int g : servers) {
      CarryInputs in;
      in.carry_ok = m & 1, in.same_stream = m >> 1 & 1, in.pipelined = m >> 2 & 1;
      in.servers = g;
      const bool want = g == 1 && (m & 7) == 7;
      CHECK(carry_round(in) == want);
      carried += want;
      n += 1;
    }
  CHECK(carry_round(CarryInputs{}));  // the defaults are the attached single-server pair
  std::printf("carry cases=%ld carried=%ld\n", n, carried);
}

// riding: the tick is exactly one launch, of the fused form; the bin has one part; the part's
// items are every resource of the leaf
static void ride_table() {
  long n = 0, rides = 0, could = 0;
  const int64_t R = 1000;
  const int64_t items[4] = {0, R - 1, R, R + 1};
  for (int classes = 0; classes <= 3; ++classes)
    for (unsigned m = 0; m < 32; ++m)
      for (int64_t it : items) {
        TickShape t;
        t.work_classes = classes;
        t.split_bin = m & 1;
        t.parts = (m >> 1 & 1) ? 2 : 1;
        t.general = m >> 2 & 1;
        t.writeback = m >> 3 & 1;
        t.items = it, t.resources = R;
        const bool fused = m >> 4 & 1;
        const bool shape = classes == 1 && t.split_bin && t.parts == 1 && !t.general && t.writeback && it == R;
        CHECK(may_ride(t) == shape);
        CHECK((place_round(t, fused) == RoundPlace::ride) == (shape && fused));
        CHECK(place_round(t, false) == RoundPlace::before_tick);
        could += shape;
        rides += shape && fused;
        n += 1;
      }
  TickShape empty;  // a leaf without resources never rides
  CHECK(!may_ride(empty));
  std::printf("ride cases=%ld shapes=%ld rides=%ld\n", n, could, rides);
}

// flushing: every other call launches a carried round unless dm_hier_step holds it
static void flush_table() {
  long n = 0, flushed = 0;
  for (unsigned m = 0; m < 4; ++m) {
    const bool want = (m & 1) && !(m & 2);
    CHECK(flush_round(m & 1, m & 2) == want);
    flushed += want;
    n += 1;
  }
  std::printf("flush cases=%ld flushed=%ld\n", n, flushed);
}

// The launches of a run of steps (L: a leaf tick, R: a root round, + within one launch), each
// step's tick fused ('f') or not ('n'), with a flushing call ('s') anywhere between steps.
static std::string order(const char* script, bool carry_ok) {
  std::string out;
  bool carried = false;
  int k = 0;
  long n = 0;
  TickShape one;
  one.items = one.resources = 100;
  CarryInputs ci;
  ci.carry_ok = carry_ok;
  for (const char* s = script; *s; ++s, ++n) {
    if (*s == 's') {
      if (flush_round(carried, false)) out += "R" + std::to_string(k - 1) + " ";
      carried = false;
      out += "| ";
      continue;
    }
    CHECK(!flush_round(carried, true));  // dm_hier_step holds it for its tick
    if (carried && place_round(one, *s == 'f') == RoundPlace::ride)
      out += "R" + std::to_string(k - 1) + "+";
    else if (carried)
      out += "R" + std::to_string(k - 1) + " ";
    out += "L" + std::to_string(k) + " ";
    carried = carry_round(ci);
    if (!carried) out += "R" + std::to_string(k) + " ";
    k += 1;
  }
  return out;
}

int main() {
  carry_table();
  ride_table();
  flush_table();
  std::printf("order on  %s\n", order("nnfffsfnfs", true).c_str());
  std::printf("order off %s\n", order("nnfffsfnfs", false).c_str());
  return 0;
}
