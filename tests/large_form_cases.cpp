// The cases of tests/test_large_form.py: dm_large_form.h alone against a transcription of
// the expressions Tick::outputs() and Tick::large_chain() held before the header existed
// (written from that code, not from the header), over every combination of the inputs; then
// one line per named case:
//   <case> <pingpong><het><b_first><s_live><spec><ask_seen><leaves_live> <phase>,<phase>,...
#include <cstdio>
#include <initializer_list>

#include "dm_large_form.h"

using namespace dm;

// ---- the parent's code, transcribed ----------------------------------------------------
namespace parent {
constexpr uint32_t DM_WRITEBACK = 1, DM_AGG_RECOMPUTE = 2, DM_WB_INPLACE = 4, DM_WB_ALTERNATE = 8;  // any distinct bits
struct Ctx {  // what the two functions read of the context
  bool spec_chain, expl_rows, general, chain_live_ok, stream_written;
  int nch, redo_light;
  uint64_t redo_epoch, write_epoch;
  int seen;  // h_serr[1]
};
struct Out {
  bool pingpong, het, b_first, s_live, spec, exchanged, chain_live_ok;
  int cls[9], phase[9], n;  // launches: 0 the chain's launcher, 1 the speculative one; its phase argument
};
inline Out tick(Ctx& c, uint32_t flags) {
  Out o{};
  // Tick::outputs()
  const bool wb = flags & DM_WRITEBACK;
  const bool spec_eligible = c.spec_chain && wb && !(flags & DM_AGG_RECOMPUTE) && !c.expl_rows && !c.general && c.nch > 0;
  o.pingpong = wb && !(flags & DM_WB_INPLACE) && ((flags & DM_WB_ALTERNATE) || spec_eligible || c.stream_written);
  // (out_gets: the alternate column on a pingpong tick and the result column on a tick that
  // is no writeback tick, else the has column)
  const bool out_is_has = wb && !o.pingpong;
  const bool recompute = flags & DM_AGG_RECOMPUTE;
  const bool live_ok = c.chain_live_ok;
  c.chain_live_ok = false;
  // Tick::large_chain()
  const int nch = c.nch;
  const bool het = c.general && nch > 0;
  o.het = het;
  o.b_first = !het && !recompute && !c.expl_rows;
  o.s_live = !het && live_ok && !c.expl_rows;
  static constexpr int kSeq[9] = {0, 1, 5, 2, 6, 7, 3, 8, 4};
  const bool spec = c.spec_chain && !het && o.b_first && wb && !out_is_has && nch > 0;
  o.spec = spec;
  if (spec) {
    bool exchanged = false;
    auto exchange = [&] {
      exchanged = true;
      const int v = c.seen;
      c.seen = 0;
      return v;
    };
    const bool light = c.redo_light == 2 || (c.redo_light == 1 && c.redo_epoch == c.write_epoch && exchange() == 0);
    o.exchanged = exchanged;
    c.redo_epoch = c.write_epoch;
    const int redo_phase = light ? 2 : 1;
    for (int ph = 0; ph < 2; ++ph) {
      o.cls[o.n] = 1;
      o.phase[o.n++] = ph == 0 ? 0 : redo_phase;
    }
  }
  for (int i = 0; i < 9 && nch > 0 && !spec; ++i) {
    const int ph = kSeq[i];
    if (ph >= 5 && !het) continue;
    if (ph == 4 && !het) continue;
    o.cls[o.n] = 0;
    o.phase[o.n++] = ph;
  }
  const bool chain_live = nch > 0 && !het;
  // Tick::finish()
  o.chain_live_ok = wb && chain_live;
  return o;
}
// the kernels the parent's two launchers started for a phase argument
constexpr LargePhase kChain[9] = {LargePhase::A,   LargePhase::B, LargePhase::C,     LargePhase::MAP,    LargePhase::FIN,
                                  LargePhase::T,   LargePhase::C_HET, LargePhase::E, LargePhase::MAP_HET};
constexpr LargePhase kSpec[3] = {LargePhase::SPEC, LargePhase::REDO_FULL, LargePhase::REDO_LIGHT};
}  // namespace parent

static const char* const kNames[kLargePhases] = {"A", "B", "T", "C", "C_HET", "E", "MAP", "MAP_HET", "FIN", "SPEC",
                                                 "REDO_FULL", "REDO_LIGHT"};

// the new code's tick: the rule, and the owner's part (the word is read only when asked)
static LargeForm tick(const LargeInputs& in, int& seen, bool& exchanged) {
  LargeForm f = choose_large(in);
  exchanged = false;
  if (f.spec && f.ask_seen) {
    exchanged = true;
    const int v = seen;
    seen = 0;
    if (v) f.seen();
  }
  return f;
}

static void show(const char* name, const LargeInputs& in, int seen = 0) {
  bool ex;
  const LargeForm f = tick(in, seen, ex);
  printf("%s %d%d%d%d%d%d%d ", name, f.pingpong, f.het, f.b_first, f.s_live, f.spec, f.ask_seen, f.leaves_live);
  for (int i = 0; i < f.n; ++i) printf("%s%s", i ? "," : "", kNames[(int)f.seq[i]]);
  printf("%s\n", f.n ? "" : "-");
}

static LargeInputs steady() {  // the steady speculative tick of a store with large resources
  LargeInputs in;
  in.writeback = in.live_ok = in.same_write_epoch = true;
  in.nchunks = 3;
  return in;
}
template <typename F>
static void with(const char* name, F&& change, int seen = 0) {
  LargeInputs in = steady();
  change(in);
  show(name, in, seen);
}

int main() {
  long cases = 0, disagree = 0, identity = 0, implied = 0, seq_het = 0, seq_plain = 0, seq_bad = 0;
  for (int bits = 0; bits < 256; ++bits)
    for (int col = 0; col < 3; ++col)  // auto, in place, alternate
      for (int nch : {0, 3})
        for (int rl = 0; rl < 3; ++rl)
          for (int seen0 = 0; seen0 < 2; ++seen0) {
            LargeInputs in;
            in.spec_chain = bits & 1;
            in.writeback = bits & 2;
            in.recompute = bits & 4;
            in.expl_rows = bits & 8;
            in.may_general = bits & 16;
            in.live_ok = bits & 32;
            in.stream_written = bits & 64;
            in.same_write_epoch = bits & 128;
            in.inplace = col == 1;
            in.alternate = col == 2;
            in.nchunks = nch;
            in.redo_light = rl;
            parent::Ctx c{in.spec_chain,   in.expl_rows, in.may_general, in.live_ok, in.stream_written, nch, rl,
                          in.same_write_epoch ? 5u : 4u, 5u, seen0};
            const uint32_t flags = (in.writeback ? parent::DM_WRITEBACK : 0) | (in.recompute ? parent::DM_AGG_RECOMPUTE : 0) |
                                   (in.inplace ? parent::DM_WB_INPLACE : 0) | (in.alternate ? parent::DM_WB_ALTERNATE : 0);
            const parent::Out o = parent::tick(c, flags);
            int seen = seen0;
            bool exchanged;
            const LargeForm f = tick(in, seen, exchanged);
            ++cases;
            bool same = f.pingpong == o.pingpong && f.het == o.het && f.b_first == o.b_first && f.s_live == o.s_live &&
                        f.spec == o.spec && f.leaves_live == o.chain_live_ok && exchanged == o.exchanged &&
                        seen == c.seen && f.n == o.n;
            bool seq_same = f.n == o.n;
            for (int i = 0; i < f.n && seq_same; ++i)
              seq_same = f.seq[i] == (o.cls[i] ? parent::kSpec : parent::kChain)[o.phase[i]];
            disagree += !(same && seq_same);
            seq_bad += !seq_same;
            if (nch > 0 && !f.spec) (f.het ? seq_het : seq_plain) += 1;
            const bool spec_eligible = in.spec_chain && in.writeback && !in.recompute && !in.expl_rows &&
                                       !in.may_general && nch > 0;
            identity += f.spec != (spec_eligible && !in.inplace);
            implied += f.spec && !(f.pingpong && !f.het && f.b_first && in.writeback && nch > 0);
          }
  printf("cases %ld disagreements %ld sequence_mismatches %ld (het %ld plain %ld) identity_violations %ld "
         "implication_violations %ld\n",
         cases, disagree, seq_bad, seq_het, seq_plain, identity, implied);

  with("steady_spec", [](LargeInputs&) {});
  with("spec_chain_off", [](LargeInputs& in) { in.spec_chain = false; });
  with("not_writeback", [](LargeInputs& in) { in.writeback = false; });
  with("recompute", [](LargeInputs& in) { in.recompute = true; });
  with("explicit_rows", [](LargeInputs& in) { in.expl_rows = true; });
  with("may_general", [](LargeInputs& in) { in.may_general = true; });
  with("no_chunks", [](LargeInputs& in) { in.nchunks = 0; });
  with("inplace", [](LargeInputs& in) { in.inplace = true; });
  with("inplace_stream_written", [](LargeInputs& in) { in.inplace = in.stream_written = true; });
  with("alternate", [](LargeInputs& in) { in.alternate = true; });
  with("alternate_spec_off", [](LargeInputs& in) { in.alternate = true, in.spec_chain = false; });
  with("stream_written_spec_off", [](LargeInputs& in) { in.stream_written = true, in.spec_chain = false; });
  with("chain_not_live", [](LargeInputs& in) { in.spec_chain = in.live_ok = false; });
  with("het_not_writeback", [](LargeInputs& in) { in.may_general = true, in.writeback = false; });
  with("may_general_no_chunks", [](LargeInputs& in) { in.may_general = true, in.nchunks = 0; });
  with("redo_light_0", [](LargeInputs& in) { in.redo_light = 0; }, 0);
  with("redo_light_1_unseen", [](LargeInputs& in) { in.redo_light = 1; }, 0);
  with("redo_light_1_seen", [](LargeInputs& in) { in.redo_light = 1; }, 1);
  with("redo_light_1_rows_written", [](LargeInputs& in) { in.same_write_epoch = false; }, 0);
  with("redo_light_2_seen", [](LargeInputs& in) { in.redo_light = 2; }, 1);
  with("redo_light_2_rows_written", [](LargeInputs& in) { in.redo_light = 2, in.same_write_epoch = false; }, 1);
  // the word is set and not asked (it stays set for the tick that may use it): ask_seen reads 0
  with("seen_not_asked_rows_written", [](LargeInputs& in) { in.same_write_epoch = false; }, 1);
  with("seen_not_asked_redo_light_0", [](LargeInputs& in) { in.redo_light = 0; }, 1);
  with("seen_not_asked_no_spec", [](LargeInputs& in) { in.inplace = true; }, 1);
  return 0;
}
