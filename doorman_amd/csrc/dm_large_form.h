// dm_large_form.h — which launches the large-resource chain runs this tick, and which output
// column the tick writes: the one decision behind Tick::outputs and Tick::large_chain
// (dm_tick.cpp), from what the host knows of the tick and of the chain (dm_large_chain.h
// LargeChain).  Plain C++17, no HIP: the rule is tested on the CPU (tests/test_large_form.py).
//
// The forms:
//   the chain          A, B, C, MAP: four launches over the chunks, a second read of the rows
//   heterogeneous      A, B, T, C, C_HET, E, MAP, MAP_HET, FIN: the chain on a store that may
//                      hold FairShare resources with mixed subclient counts
//   speculative        SPEC, then REDO_FULL or REDO_LIGHT: one launch that writes its gets
//                      before they are verified, and a redo for the resources whose totals moved
#pragma once
#include <cstdint>

namespace dm {

// The chain's launches (the unit dm_tick_large.hip has a kernel for each), named in launch order.
enum class LargePhase : uint8_t { A, B, T, C, C_HET, E, MAP, MAP_HET, FIN, SPEC, REDO_FULL, REDO_LIGHT };
constexpr int kLargePhases = 12;

struct LargeInputs {
  bool spec_chain = true;        // DM_SPEC_CHAIN
  bool writeback = false, recompute = false;
  bool inplace = false, alternate = false;  // DM_WB_INPLACE, DM_WB_ALTERNATE (never both: dm_apportion rejects it)
  bool expl_rows = false;        // the store may hold explicit-expiry rows
  bool may_general = false;      // some non-small resource may need k_general
  int nchunks = 0;
  bool live_ok = false;          // the last call that changed the store was a writeback tick through the chain
  bool stream_written = false;   // a store beyond the Infinity Cache whose rows a call wrote since the last writeback tick
  int redo_light = 1;            // DM_REDO_LIGHT: 0 never, 1 while the redo finds nothing marked, 2 always
  bool same_write_epoch = false;  // no row written since the last speculative tick
  bool cycle = false;            // a workgroup-bin part asks for the alternate column (dm_split_form.h CycleAuto)
};

struct LargeForm {
  bool pingpong = false;  // the tick writes the alternate gets column, which becomes the store's has
  bool het = false;       // heterogeneous FairShare is decided on the chain (Partials::s_set)
  bool b_first = false;   // Partials::b_first
  bool s_live = false;    // Partials::s_live
  bool spec = false;      // the speculative form
  // The speculative form's redo runs the light build (seq[1] == REDO_LIGHT) always under
  // DM_REDO_LIGHT=2, and under 1 while no row was written since the last speculative tick and
  // the last redo the host saw found nothing marked.  That last term is a host-mapped word
  // which the reader clears, so it is read only when the other terms leave the choice to it:
  // ask_seen says so, the word's owner (LargeChain::take_seen) reads it, and seen() takes
  // the answer.
  bool ask_seen = false;
  void seen() { seq[1] = LargePhase::REDO_FULL; }
  bool leaves_live = false;  // the tick runs the chain in a form that leaves Partials::uni and live for s_live
  LargePhase seq[9] = {};    // this tick's launches, in launch order
  int n = 0;
};

inline LargeForm choose_large(const LargeInputs& in) {
  LargeForm f;
  // The speculative form writes its gets before they are verified, so they must not land on
  // the store's has column: a tick that may take it writes the alternate column whatever
  // the store's size, and a tick told to write in place does not take it.  It needs pass
  // A's round 1 to be exact (b_first's terms) and no resource that the chain hands on.
  const bool spec_eligible = in.spec_chain && in.writeback && !in.recompute && !in.expl_rows && !in.may_general &&
                             in.nchunks > 0;
  // ... and a tick for which a workgroup-bin part asks writes it for the cycle form's sake;
  // the caller's DM_WB_INPLACE goes before that too.
  f.pingpong = in.writeback && !in.inplace && (in.alternate || spec_eligible || in.stream_written || in.cycle);
  // spec implies pingpong && !het && b_first && writeback && nchunks > 0 (the terms the chain's
  // launches once spelled out again)
  f.spec = spec_eligible && !in.inplace;
  f.het = in.may_general && in.nchunks > 0;
  f.b_first = !f.het && !in.recompute && !in.expl_rows;
  f.s_live = !f.het && in.live_ok && !in.expl_rows;
  f.leaves_live = in.writeback && in.nchunks > 0 && !f.het;
  auto add = [&f](LargePhase ph) { f.seq[f.n++] = ph; };
  if (f.spec) {
    f.ask_seen = in.redo_light == 1 && in.same_write_epoch;
    add(LargePhase::SPEC);
    add(in.redo_light == 2 || f.ask_seen ? LargePhase::REDO_LIGHT : LargePhase::REDO_FULL);
  } else if (in.nchunks > 0) {
    add(LargePhase::A);
    add(LargePhase::B);
    if (f.het) add(LargePhase::T);
    add(LargePhase::C);
    if (f.het) add(LargePhase::C_HET), add(LargePhase::E);
    add(LargePhase::MAP);  // without het its last-arriving chunks do FIN's work
    if (f.het) add(LargePhase::MAP_HET), add(LargePhase::FIN);
  }
  return f;
}

}  // namespace dm
