// The cases of tests/test_tick_order.py: dm_tick_order.h alone, one line per case.
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "dm_tick_order.h"

using namespace dm;

static const char* name(TickWait w) {
  return w == TickWait::none ? "none" : w == TickWait::tick_events ? "tick_events" : "event";
}
static const char* name(SlotReuse r) {
  switch (r) {
    case SlotReuse::stream_order: return "stream_order";
    case SlotReuse::covered: return "covered";
    case SlotReuse::tick_events: return "tick_events";
    case SlotReuse::join_then_event: return "join_then_event";
    case SlotReuse::lazy_token: return "lazy_token";
    case SlotReuse::none: break;
  }
  return "none";
}
static const char* name(QueueCalib::Phase p) {
  switch (p) {
    case QueueCalib::Phase::Pending: return "Pending";
    case QueueCalib::Phase::Round1: return "Round1";
    case QueueCalib::Phase::Round2: return "Round2";
    case QueueCalib::Phase::Waiting: return "Waiting";
    case QueueCalib::Phase::Done: break;
  }
  return "Done";
}
static void show(const QueueCalib::Action& a) {
  static const char* const kinds[] = {"none", "start", "close_then_start", "close_then_wait", "poll", "done"};
  printf("%s", kinds[a.kind]);
  if (a.kind == QueueCalib::Action::start || a.kind == QueueCalib::Action::close_then_start ||
      a.kind == QueueCalib::Action::done)
    printf("(%d%d%d%d)", a.perm[0], a.perm[1], a.perm[2], a.perm[3]);
}

// The last tick of a leaf in stream parts on auxiliary streams 1 and 2, both parts' last
// kernels completing its events, tick 40.
static TickSignal parts_tick() {
  TickSignal s;
  s.seq = 40;
  s.wanted = s.flagged = true;
  s.nev[40 % kTickEv] = 2;
  s.part_mask = s.unjoined = 0x6;
  return s;
}

static void follow(const char* n, const TickSignal& s, bool same) {
  const FollowOrder o = follow_last_tick(s, same);
  printf("%s join=%d wait=%s\n", n, o.join, name(o.wait));
}

static void reuse(const char* n, const TickSignal& s, bool same, bool rec, uint64_t free_seq, bool cover, bool ordered) {
  printf("%s %s\n", n, name(slot_reuse(s, same, rec, free_seq, cover, ordered)));
}

static void queue_state(const char* n, const TemplateQueue& q, int got) {
  printf("%s got=%d pending=", n, got);
  for (const auto& p : q.pending) printf("%d@%lld,", p.slot, (long long)p.tag);
  printf(" free=");
  for (int f : q.free_slots) printf("%d,", f);
  printf("\n");
}

static void signal_state(const char* n, const TickSignal& s) {
  printf("%s seq=%llu flagged=%d nev=%d mask=%x unjoined=%x covers=%d\n", n, (unsigned long long)s.seq, s.flagged,
         s.nev[s.seq % kTickEv], s.part_mask, s.unjoined, s.covers());
}

// A calibration run to the end of round 1's windows: the ticks on which something happened.
static QueueCalib round1_done(bool print) {
  QueueCalib q;
  for (int tick = 1; q.phase != QueueCalib::Phase::Waiting; ++tick) {
    const QueueCalib::Action a = q.on_tick(true);
    const bool edge = tick <= QueueCalib::kCalibSkip + 2 * QueueCalib::kCalibWin || a.kind == QueueCalib::Action::close_then_wait;
    if (print && a.kind != QueueCalib::Action::none && edge) {
      printf("calib_round1 tick=%d ", tick);
      show(a);
      printf(" phase=%s windows=%d\n", name(q.phase), (int)q.of_ev.size());
    }
  }
  return q;
}

// Round 1's times: window w (the w-th permutation of 0123 in lexicographic order) takes
// 100 + w ms, except the ones given.
static std::vector<float> times24(std::initializer_list<std::pair<int, float>> set) {
  std::vector<float> ms;
  for (int w = 0; w < 24; ++w) ms.push_back(100.0f + (float)w);
  for (const auto& s : set) ms[(size_t)s.first] = s.second;
  return ms;
}

// Round 2 from these round-1 times, then round 2's windows with the times given (cycled).
static void two_rounds(const char* n, std::initializer_list<std::pair<int, float>> r1, std::vector<float> r2) {
  QueueCalib q = round1_done(false);
  printf("%s poll=", n);
  show(q.on_tick(true));
  QueueCalib::Action a = q.on_times(times24(r1));
  printf(" round2=");
  show(a);
  printf(" phase=%s schedule=", name(q.phase));
  for (const auto& pm : q.cand) printf("%d%d%d%d,", pm[0], pm[1], pm[2], pm[3]);
  printf(" ticks=");
  int opened = 1;
  for (int tick = 2; q.phase == QueueCalib::Phase::Round2; ++tick) {
    a = q.on_tick(true);
    if (a.kind == QueueCalib::Action::none) continue;
    printf("%d:", tick);
    show(a);
    printf(",");
    opened += a.kind == QueueCalib::Action::close_then_start;
  }
  std::vector<float> ms;
  for (int w = 0; w < opened; ++w) ms.push_back(r2[(size_t)w % r2.size()]);
  a = q.on_times(ms);
  printf(" windows=%d pick=", opened);
  show(a);
  printf(" phase=%s best=%lld\n", name(q.phase), (long long)q.best);
}

int main() {
  // follow_last_tick
  TickSignal s = parts_tick();
  follow("follow_same_stream", s, true);
  follow("follow_parts_cover", s, false);
  s.part_mask = s.unjoined = 0;
  follow("follow_flagged_not_forked", s, false);
  s = parts_tick();
  s.flagged = false;
  follow("follow_not_flagged", s, false);
  s = parts_tick();
  s.unjoined |= 0x8;
  follow("follow_cover_broken", s, false);

  // root_round_order: same x pipelined x covers x hs_ordered
  for (int i = 0; i < 16; ++i) {
    const bool same = i & 8, pipelined = i & 4, covers = i & 2, ordered = i & 1;
    s = parts_tick();
    if (!covers) s.unjoined |= 0x1;
    const RoundOrder o = root_round_order(s, same, pipelined, ordered);
    printf("round_same%d_pipe%d_covers%d_ordered%d cover=%d join=%d wait=%s\n", same, pipelined, covers, ordered, o.cover,
           o.join, name(o.wait));
  }

  // slot_reuse
  s = parts_tick();
  reuse("reuse_same_stream", s, true, true, 38, false, false);
  reuse("reuse_covered", s, false, true, 38, true, true);
  reuse("reuse_covered_not_ordered", s, false, true, 38, true, false);
  reuse("reuse_ordered_not_covered", s, false, true, 38, false, true);
  reuse("reuse_ring_14_back", s, false, true, 40 - (kTickEv - 2), false, false);
  reuse("reuse_ring_15_back", s, false, true, 40 - (kTickEv - 1), false, false);
  reuse("reuse_this_tick_ordered", s, false, true, 40, true, true);
  reuse("reuse_this_tick_not_ordered", s, false, true, 40, true, false);
  reuse("reuse_token", s, false, true, 0, true, true);
  reuse("reuse_never_read", s, false, false, 0, false, false);
  reuse("reuse_never_read_stale_seq", s, false, false, 38, false, false);

  // take_templates
  for (int i = 0; i < 4; ++i) {
    s = parts_tick();
    if (i & 1) s.unjoined |= 0x1;
    const TakeOrder o = take_templates(s, i & 2);
    printf("take_hostwait%d_covers%d keep=%d join=%d dirty=%d free_seq=%llu\n", (i >> 1) & 1, !(i & 1), o.keep, o.join,
           o.dirty, (unsigned long long)o.free_seq);
  }
  s = parts_tick();
  s.flagged = false;
  printf("take_not_flagged free_seq=%llu\n", (unsigned long long)take_templates(s, true).free_seq);

  // TemplateQueue
  {
    TemplateQueue q;
    q.reset();
    q.ticks_issued = 10;
    queue_state("queue_nothing_pending", q, q.take());
    q.stage(q.next_free());  // an exchange after tick 10
    queue_state("queue_lag1_same_tick", q, q.take());
    q.tick();
    queue_state("queue_lag1_next_tick", q, q.take());
  }
  {
    TemplateQueue q;
    q.reset();
    q.lag = 2;
    q.ticks_issued = 10;
    q.stage(q.next_free());
    q.tick();
    queue_state("queue_lag2_next_tick", q, q.take());
    q.tick();
    queue_state("queue_lag2_one_later", q, q.take());
  }
  {
    TemplateQueue q;
    q.reset();
    q.ticks_issued = 10;
    q.stage(q.next_free());  // slot 0, due
    q.stage(q.next_free());  // slot 1, due: the newest due
    q.tick();
    q.stage(q.next_free());  // slot 2, enqueued after tick 11: not due before tick 12
    queue_state("queue_three_two_due", q, q.take());
    q.release(1);
    queue_state("queue_released", q, -1);
    q.stage(q.next_free());
    q.stage(q.next_free());
    q.stage(q.next_free());
    queue_state("queue_no_slot_free", q, q.next_free());
    printf("queue_newest %d\n", q.newest());
    q.drop_pending();
    queue_state("queue_dropped", q, q.newest());
    q.reset();
    queue_state("queue_reset", q, q.next_free());
  }

  // TickSignal
  {
    TickSignal t;
    t.seq = 7;
    t.flag(true, 2);
    signal_state("signal_not_wanted", t);
    t.want();
    t.flag(false, 2);
    signal_state("signal_not_one_class", t);
    printf("signal_carries %d%d\n", t.carries(true), t.carries(false));
    t.unjoined |= 0x6;  // the tick forked onto streams 1 and 2
    t.flag(true, 2);
    t.add_part(0x2);
    t.add_part(0x4);
    signal_state("signal_two_parts", t);
    t.unflag();
    signal_state("signal_unflag_mixed", t);
    t.flag(true, 2);
    t.add_part(0x2);
    t.add_part(0x4);
    t.begin();
    signal_state("signal_begin", t);
    t.flag(true, 1);
    t.add_part(0);
    signal_state("signal_context_stream", t);
    t.flag(true, 1);
    t.add_part(0x2);
    signal_state("signal_one_part_other_unjoined", t);
    t.unjoined = 0;  // a join
    signal_state("signal_after_join", t);
  }

  // QueueCalib
  {
    QueueCalib q;
    printf("calib_shared_queues ");
    show(q.on_tick(false));
    printf(" phase=%s best=%lld\n", name(q.phase), (long long)q.best);
    q = QueueCalib();
    q.phase = QueueCalib::Phase::Done;  // DM_QUEUE_CALIB=0
    printf("calib_off ");
    show(q.on_tick(true));
    printf(" phase=%s\n", name(q.phase));
  }
  const QueueCalib r1 = round1_done(true);
  printf("calib_round1_end windows=%d candidates=%d last=%d%d%d%d\n", (int)r1.of_ev.size(), (int)r1.cand.size(),
         r1.cand[23][0], r1.cand[23][1], r1.cand[23][2], r1.cand[23][3]);
  // the identity (window 0) is the slowest: appended; round 2's sums decide
  two_rounds("calib_identity_appended", {{0, 200.0f}}, {10.0f, 9.0f, 11.0f, 12.0f});
  // the identity among the finalists, not first: not duplicated
  two_rounds("calib_identity_among", {{0, 101.5f}, {1, 99.0f}}, {10.0f, 11.0f, 9.5f});
  // equal times in round 1 (windows 5 and 9): the earlier window first
  two_rounds("calib_round1_tie", {{9, 50.0f}, {5, 50.0f}, {0, 60.0f}}, {10.0f, 10.0f, 12.0f});
  // equal sums in round 2: 4 x 10 on every finalist
  two_rounds("calib_equal_sums", {{0, 200.0f}}, {10.0f});
  // equal sums of two, from different terms: windows (8, 12) and (12, 8) against the rest
  two_rounds("calib_equal_sums_of_two", {{0, 200.0f}},
             {30.0f, 8.0f, 12.0f, 30.0f, 30.0f, 12.0f, 8.0f, 30.0f, 30.0f, 10.0f, 10.0f, 30.0f, 30.0f, 10.0f, 10.0f, 30.0f});
  return 0;
}
