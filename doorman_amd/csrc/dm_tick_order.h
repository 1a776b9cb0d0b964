// dm_tick_order.h — which stream waits for which around a tick: the tick-done signal's
// bookkeeping (TickSignal), the decisions that put another stream behind the leaf's last
// tick (follow_last_tick, root_round_order, slot_reuse, take_templates), the host half of a
// pipelined leaf's template slots (TemplateQueue) and the queue calibration's schedule and
// choice (QueueCalib).  Plain C++17, no HIP: nothing here touches a stream, so the rules are
// tested on the CPU (tests/test_tick_order.py).  The owners that hold the HIP handles and
// carry a decision out are in dm_ctx.h (StreamOrder, TickDone, TemplatePipe,
// QueueCalibration); a missed wait is a race, not a failing assertion, so each rule is
// written once, here.
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

namespace dm {

constexpr int kAux = 4;       // auxiliary streams: independent size bins of one tick run concurrently
constexpr int kTickEv = 16;   // the ring of tick events (per stream part)
constexpr int kTplSlots = 4;  // staged templates: in use + pending (lag 2) + the one being written

// The tick-done signal: ticks numbered by seq (never reset).  The last kernel of a
// one-class split tick (C1, C3: the dense kernel, or the rest kernel after it) is launched
// with a stop event (hipExtLaunchKernel: the kernel's own completion signal, no marker
// packet of its own on the leaf's queue -- each marker cost a ~10-us bubble per N = 8 shard
// step), one event per tick in a ring (TickDone, dm_ctx.h); another queue waits on it.
// Round 4 stored a word from a one-wave k_tick_done after the dense kernel (5 us of the
// leaf's queue): the N = 8 rehearsal step 60.2-60.7 -> 58.7-58.8 us (round 5,
// gpurun_out/r5b2shard, three alternations).
// The event covers the tick's leases and sums, not every launch of it: once per row epoch a
// writeback tick enqueues k_count_undense after the event-carrying kernel on the same
// stream (check_dense).  That kernel only reads the work items' hints and writes a
// host-mapped count, which no consumer of the event (the exchange, a template slot's reuse)
// touches; a consumer that needed it would have to join the stream.
struct TickSignal {
  uint64_t seq = 0;        // the last tick's number
  bool flagged = false;    // ... and whether its last kernels complete the ring's events [*][seq % kTickEv]
  int nev[kTickEv] = {};   // the parts that completed each flagged tick's events
  unsigned part_mask = 0;  // auxiliary streams of the last flagged tick's parts
  // set by the first consumer on another stream (the exchange's order, a template slot's
  // reuse): before it, no tick carries the event
  bool wanted = false;
  unsigned unjoined = 0;   // auxiliary streams with work not yet joined into the context stream

  void begin() {  // a new tick
    seq += 1;
    flagged = false;
  }
  void want() { wanted = true; }
  // one_class: the tick runs one work class, a split bin (on the context stream, or in
  // stream parts): its last kernel completes the tick's event when a consumer wants one
  bool carries(bool one_class) const { return one_class && wanted; }
  void flag(bool one_class, int nparts) {  // the bin's parts will complete this tick's events
    if (!carries(one_class)) return;
    flagged = true;
    nev[seq % kTickEv] = nparts;
    part_mask = 0;
  }
  void add_part(unsigned stream_bit) { part_mask |= stream_bit; }  // (0: the part runs on the context stream)
  void unflag() {  // a part in the one-kernel form carries no event: consumers join instead
    flagged = false;
    part_mask = 0;
  }
  // the last tick's events cover every auxiliary stream's unjoined work, so a consumer
  // may wait on them instead of joining (which would make the next tick's parts wait
  // for each other: 49 -> 74 us per tick on the N = 8 shard, tools/shard_split.py)
  bool covers() const { return flagged && part_mask != 0 && (unjoined & ~part_mask) == 0; }
};

// How a consumer stream gets behind the leaf's work: not at all (stream order, or already
// ordered), on the tick's events (TickDone::wait), or on an event recorded on the leaf's
// context stream (after a join, when class streams hold work).
enum class TickWait { none, tick_events, event };

// dm_hier_step, several servers: the exchange stream after the tick that wrote the block.
// On the tick's events when its last kernels complete them (no marker on the leaf's queues;
// the leaf's stream parts stay unjoined), else after a join, on an event.
struct FollowOrder {
  bool join;      // join the leaf's class streams into its context stream first
  TickWait wait;
};
inline FollowOrder follow_last_tick(const TickSignal& sig, bool same_stream) {
  const bool cover = !same_stream && sig.covers();
  FollowOrder o{!cover, TickWait::none};
  if (same_stream) return o;  // stream order
  // (flagged with no part on a class stream: the tick ran on the context stream alone)
  o.wait = cover || (sig.flagged && sig.part_mask == 0) ? TickWait::tick_events : TickWait::event;
  return o;
}

// The head of dm_hier_root_tick.  A pipelined leaf whose last tick's events cover its
// streams stays unjoined (the round writes a free template slot, and waits on those
// events); otherwise the leaf's streams join first.  hs_ordered: dm_hier_step already put
// the round's stream behind the tick.
struct RoundOrder {
  bool cover, join;
  TickWait wait;  // the root round after the leaf's prior work (its publish)
};
inline RoundOrder root_round_order(const TickSignal& sig, bool same, bool pipelined, bool hs_ordered) {
  const bool cover = !same && pipelined && sig.covers();
  RoundOrder o{cover, !cover, TickWait::none};
  if (!same && !hs_ordered) o.wait = cover ? TickWait::tick_events : TickWait::event;
  return o;
}

// Before a round writes a template slot, the ticks that read the slot's old templates must
// be done.
enum class SlotReuse {
  stream_order,     // the leaf's ticks precede this round on the one stream
  covered,          // this round already waits for the leaf's last tick, whose events cover
                    // every earlier tick on the same streams
  tick_events,      // wait on the events of tick free_seq
  join_then_event,  // that tick's events were recorded again since: everything the leaf holds
  lazy_token,       // the slot's (lazy) token on the leaf's stream
  none              // the slot was never read
};
// free_rec, free_seq: the slot's (TemplatePipe); cover: root_round_order's
inline SlotReuse slot_reuse(const TickSignal& sig, bool same, bool free_rec, uint64_t free_seq, bool cover,
                            bool hs_ordered) {
  if (same) return SlotReuse::stream_order;
  if (free_rec && free_seq > 0) {
    if (cover && hs_ordered && free_seq <= sig.seq) return SlotReuse::covered;
    if (sig.seq - free_seq < (uint64_t)kTickEv - 1) return SlotReuse::tick_events;
    return SlotReuse::join_then_event;
  }
  return free_rec ? SlotReuse::lazy_token : SlotReuse::none;
}

// A leaf tick takes staged templates.  host_wait: the round that wrote them ran on another
// stream, so the host waits for it (TemplatePipe).  Deferred class work also read the old
// templates: joined, unless the last tick's events cover it (the slot's reuse then waits
// on them).
struct TakeOrder {
  bool keep;          // the class streams stay unjoined
  bool join, dirty;   // else: join them, and they fork after the wait
  uint64_t free_seq;  // the old templates' slot is free once this tick's events completed (0: its token)
};
inline TakeOrder take_templates(const TickSignal& sig, bool host_wait) {
  const bool keep = host_wait && sig.covers();
  return TakeOrder{keep, !keep, !keep, sig.flagged ? sig.seq : 0};
}

// The host half of a pipelined leaf's templates (dm_hier_pipeline).  An exchange stages the
// leaf's new templates in a free slot; the leaf's ticks take the staged templates of the
// exchanges enqueued before the previous tick (one tick of lag).
struct TemplateQueue {
  struct Staged {
    int slot;
    int64_t tag;  // leaf ticks issued before the exchange was enqueued
  };
  std::vector<Staged> pending;  // oldest first
  std::vector<int> free_slots;
  int lag = 1;  // ticks between an exchange and the first tick that takes its templates, minus one
  int64_t ticks_issued = 0;

  // Before a tick: the slot whose templates it takes (the newest that is due), or -1.  The
  // older due ones are superseded: their slots are free.
  int take() {
    int slot = -1;
    size_t n = 0;
    while (n < pending.size() && pending[n].tag + (lag - 1) < ticks_issued) slot = pending[n++].slot;
    for (size_t i = 0; i + 1 < n; ++i) free_slots.push_back(pending[i].slot);
    pending.erase(pending.begin(), pending.begin() + (std::ptrdiff_t)n);
    return slot;
  }
  void release(int slot) { free_slots.push_back(slot); }  // its templates were swapped out: free after the ticks enqueued
  void tick() { ticks_issued += 1; }
  int next_free() const { return free_slots.empty() ? -1 : free_slots.front(); }  // -1: too many staged exchanges
  int newest() const { return pending.empty() ? -1 : pending.back().slot; }
  void stage(int slot) {  // a round wrote next_free()
    free_slots.erase(free_slots.begin());
    pending.push_back(Staged{slot, ticks_issued});
  }
  void reset() {
    pending.clear();
    free_slots.clear();
    for (int i = 0; i < kTplSlots; ++i) free_slots.push_back(i);
  }
  void drop_pending() { pending.clear(); }  // staged exchanges were computed for an old configuration
};

// Queue calibration: which of the four auxiliary streams -- four hardware queues -- carries
// which work class moved configs[2]'s tick from 111 to 157 us over the 24 assignments
// (profiles/r05_queues.txt), and a queue's place in the process's creation order, which a
// host that made streams of its own first shifts, decides which assignment is best.  So
// the context times every assignment on its first forked writeback ticks (windows of
// kCalibWin ticks, each between joins of every class stream, HIP events on the context
// stream), times the best kCalibFinal again over longer windows, and keeps the fastest.
// (the skip: a context's first ticks run slow -- first-touch, and the GPU reaches its
// sustained-load operating point only after ~0.1-0.3 s of back-to-back work,
// profiles/r06_c4_variants.md -- which biases the candidates timed first; round 2
// therefore also interleaves its candidates, kCalibRep2 short windows each, and sums
// them, so that a drift of the clocks falls on every candidate alike)
// Here: the schedule (on_tick: which tick opens or closes a window) and the choice
// (on_times); QueueCalibration (dm_ctx.h) holds the streams and the windows' events.
struct QueueCalib {
  static constexpr int kCalibSkip = 1024, kCalibWin = 6, kCalibFinal = 3, kCalibWin2 = 4, kCalibRep2 = 4;
  using Perm = std::array<int, kAux>;  // class stream i runs on the perm[i]-th created queue
  enum class Phase { Pending, Round1, Round2, Waiting, Done };  // (Waiting: for the windows' events; Done: or off)
  Phase phase = Phase::Pending;
  int skip = 0;   // forked writeback ticks seen while Pending
  int k = 0;      // the open window (an index into cand)
  int t = 0;      // ticks in the open window, this one included
  int round = 0;
  std::vector<Perm> cand;  // the round's windows, in order
  std::vector<int> of_ev;  // candidate timed by each window opened
  bool log = false;        // test hook (DM_QUEUE_CALIB=2): every window's assignment and time per tick
  int64_t best = -1;       // the chosen permutation (perm[0] + 4 perm[1] + 16 perm[2] + 64 perm[3])

  struct Action {
    enum Kind {
      none,
      start,             // apply perm, open a window
      close_then_start,  // close the open window, apply perm, open the next
      close_then_wait,   // close the round's last window
      poll,              // the last window's end event done?  then on_times
      done               // apply perm: the choice
    } kind = none;
    Perm perm{};
  };

  // One forked writeback tick, before it forks.  own_queue: each auxiliary stream has a
  // hardware queue of its own (else the assignment does not choose hardware queues).
  Action on_tick(bool own_queue) {
    switch (phase) {
      case Phase::Done: return {};
      case Phase::Pending: {
        if (!own_queue) {
          phase = Phase::Done;
          return {};
        }
        if (++skip < kCalibSkip) return {};
        Perm pm{0, 1, 2, 3};
        cand.clear();
        do cand.push_back(pm);
        while (std::next_permutation(pm.begin(), pm.end()));
        phase = Phase::Round1;
        round = 1;
        return open(Action::start, 0);  // this tick is the window's first
      }
      case Phase::Round1:
      case Phase::Round2: {
        if (++t <= window()) return {};
        if (k + 1 < (int)cand.size()) return open(Action::close_then_start, k + 1);
        k += 1;
        t = 1;
        phase = Phase::Waiting;  // polled by later ticks
        return {Action::close_then_wait, {}};
      }
      case Phase::Waiting: break;
    }
    return {Action::poll, {}};
  }

  // Every window's time, in the order the windows were opened.
  Action on_times(const std::vector<float>& ms) {
    std::vector<std::pair<float, size_t>> tm;
    for (size_t w = 0; w < ms.size(); ++w) tm.push_back({ms[w], w});
    if (log)
      for (const auto& pr : tm) {
        const Perm& pm = cand[(size_t)of_ev[pr.second]];
        fprintf(stderr, "[dm queue calibration] round %d perm %d%d%d%d %.2f us/tick\n", round, pm[0], pm[1], pm[2],
                pm[3], 1000.0 * pr.first / window());
      }
    std::sort(tm.begin(), tm.end());  // by (time, window)
    if (round == 1) {  // round 2: the best of round 1 over interleaved windows
      // the best kCalibFinal of round 1, and the creation-order assignment (the measured
      // default) so that the choice is never worse than not calibrating
      std::vector<Perm> fin;
      const Perm ident{0, 1, 2, 3};
      for (int i = 0; i < kCalibFinal; ++i) fin.push_back(cand[(size_t)of_ev[tm[(size_t)i].second]]);
      if (std::find(fin.begin(), fin.end(), ident) == fin.end()) fin.push_back(ident);
      of_ev.clear();
      cand.clear();
      for (int r = 0; r < kCalibRep2; ++r)  // interleaved: fin[0], fin[1], ..., fin[0], ...
        cand.insert(cand.end(), fin.begin(), fin.end());
      phase = Phase::Round2;
      round = 2;
      return open(Action::start, 0);
    }
    // round 2: each candidate's windows summed
    std::vector<std::pair<Perm, float>> sum;
    for (const auto& pr : tm) {
      const Perm& pm = cand[(size_t)of_ev[pr.second]];
      auto it = std::find_if(sum.begin(), sum.end(), [&](const auto& x) { return x.first == pm; });
      if (it == sum.end()) sum.push_back({pm, pr.first});
      else it->second += pr.first;
    }
    const Perm pick =
        std::min_element(sum.begin(), sum.end(), [](const auto& a, const auto& b) { return a.second < b.second; })->first;
    of_ev.clear();
    phase = Phase::Done;
    best = pick[0] + 4 * pick[1] + 16 * pick[2] + 64 * pick[3];
    return {Action::done, pick};
  }

 private:
  int window() const { return round == 1 ? kCalibWin : kCalibWin2; }
  Action open(Action::Kind kind, int window_k) {
    k = window_k;
    t = 1;
    of_ev.push_back(k);
    return {kind, cand[(size_t)k]};
  }
};

}  // namespace dm
