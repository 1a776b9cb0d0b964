// dm_carry_rule.h — where the root's round of an attached pair's step runs: in a launch of
// its own behind the leaf tick that published its request (L0 R0 L1 R1 ...), or carried by the
// host and run inside the next leaf tick's one launch (L0 | R0+L1 | R1+L2 | ...).  Plain C++17,
// no HIP, tested on the CPU (tests/test_carry_rule.py): the rule is written once, here, and
// carried out by dm_hier_host.cpp (carrying, flushing) and dm_tick.cpp (riding).
//
// Why no order is lost.  With one server the root holds one row per resource, and the round for
// resource r reads r's published record, root row and root configuration and writes r's root
// row, sums and template; its only grid-wide input is the flags word of the published block,
// which every workgroup of the publishing tick ORs into, so the round cannot ride in that tick's
// launch.  It can ride in the next: at lag 1 the templates round t-1 stages are first taken by
// tick t+1 (TemplateQueue::take), tick t reads the leaf's configuration (round t-2's buffer) and
// the leaf store, and round t-1 writes the root store, the status word and a free template slot.
// The publish ring has at least three blocks, so the block of tick t-1, the block tick t writes
// and the block whose flags tick t clears are three buffers, and by stream order block t-1 is
// final when launch t starts.  Every result is bit for bit the two-launch order's.
//
// What a caller sees: after dm_hier_step the round's writes (root rows, sums, status, staged
// templates) are on the stream only after the next library call on either context, each of
// which first launches a carried round (flush): the step's own next call lets it ride or
// launches it ahead of its tick.
#pragma once
#include <cstdint>

namespace dm {

// dm_hier_step, after its leaf tick: carry the round, or launch it now?
struct CarryInputs {
  bool carry_ok = true;     // DM_CARRY_ROUND
  int servers = 1;          // the exchange's layout (dm_hier_layout): G
  bool same_stream = true;  // the exchange runs on the leaf's stream
  bool pipelined = true;    // the leaf's template pipe is on: the round writes a staged slot
};
inline bool carry_round(const CarryInputs& in) {
  return in.carry_ok && in.servers == 1 && in.same_stream && in.pipelined;
}

// The next dm_hier_step's leaf tick, with a round carried.
enum class RoundPlace {
  ride,         // inside the tick's one launch (k_block_fused's ROOT build)
  before_tick,  // a plain k_hier_tick ahead of the tick's launches: the order it had
};
// What the host knows of the tick before its first launch: the round runs ahead of the tick
// unless the tick can only be one launch of a workgroup bin.
struct TickShape {
  int work_classes = 1;   // non-empty work classes: bins, the small tiles, the large chain
  bool split_bin = true;  // ... and the one is a workgroup bin (3-6)
  int parts = 1;          // the bin's stream parts
  bool general = false;   // the tick may run k_general
  bool writeback = true;
  int64_t items = 0;      // the part's items
  int64_t resources = 0;  // the leaf's resources
};
inline bool may_ride(const TickShape& t) {
  return t.work_classes == 1 && t.split_bin && t.parts == 1 && !t.general && t.writeback && t.items > 0 &&
         t.items == t.resources;
}
// ... and once the part's form is chosen (dm_split_form.h choose_form): only the fused form is
// one launch.
inline RoundPlace place_round(const TickShape& t, bool fused) {
  return may_ride(t) && fused ? RoundPlace::ride : RoundPlace::before_tick;
}

// Every other exported call that takes the leaf or the root launches a carried round first;
// dm_hier_step holds it for its own tick (held).
inline bool flush_round(bool carried, bool held) { return carried && !held; }

}  // namespace dm
