"""Which stream waits for which around a tick (doorman_amd/csrc/dm_tick_order.h): the tick-done
signal's bookkeeping, the orders that put another stream behind the leaf's last tick
(follow_last_tick, root_round_order, slot_reuse, take_templates), the host half of the
pipelined leaf's template slots (TemplateQueue) and the queue calibration's schedule and
choice (QueueCalib).

The header is plain C++17, so the rules run on the CPU: tests/tick_order_cases.cpp includes
it alone, prints one line per case, and the lines are compared with the table below.  The
table was written from the code as it stood before the header existed, not from the header:
commit_templates and calib_step (dm_tick.cpp), dm_hier_root_tick and dm_hier_step
(dm_hier_host.cpp), Tick::bins / bin_part / launch_mixed and dm_apportion for the signal.
Each of those bodies, with its HIP calls replaced by a note of the call, was run on the
same cases (a join, a wait on the tick's events, a wait on an event, calib_apply and
calib_mark were what it recorded), and the answers agree with a reading of the code by hand:
window 0 opens on the kCalibSkip-th forked writeback tick (1024), the next kCalibWin = 6
ticks later, the 24th closes on tick 1024 + 24 * 6 = 1168; the ring bound admits a wait on
a tick's events up to kTickEv - 2 = 14 ticks back.

The signal in most cases is the last tick (40) of a leaf in stream parts on auxiliary
streams 1 and 2 (mask 6), both unjoined, both parts' last kernels completing its events.
Calibration lines: round 1's window w (the w-th permutation of 0123) takes 100 + w ms
unless the case says otherwise; `ticks=` are the round-2 ticks on which a window closes.
A permutation abcd encodes as a + 4 b + 16 c + 64 d (0213 -> 216).
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = """\
follow_same_stream join=1 wait=none
follow_parts_cover join=0 wait=tick_events
follow_flagged_not_forked join=1 wait=tick_events
follow_not_flagged join=1 wait=event
follow_cover_broken join=1 wait=event
round_same0_pipe0_covers0_ordered0 cover=0 join=1 wait=event
round_same0_pipe0_covers0_ordered1 cover=0 join=1 wait=none
round_same0_pipe0_covers1_ordered0 cover=0 join=1 wait=event
round_same0_pipe0_covers1_ordered1 cover=0 join=1 wait=none
round_same0_pipe1_covers0_ordered0 cover=0 join=1 wait=event
round_same0_pipe1_covers0_ordered1 cover=0 join=1 wait=none
round_same0_pipe1_covers1_ordered0 cover=1 join=0 wait=tick_events
round_same0_pipe1_covers1_ordered1 cover=1 join=0 wait=none
round_same1_pipe0_covers0_ordered0 cover=0 join=1 wait=none
round_same1_pipe0_covers0_ordered1 cover=0 join=1 wait=none
round_same1_pipe0_covers1_ordered0 cover=0 join=1 wait=none
round_same1_pipe0_covers1_ordered1 cover=0 join=1 wait=none
round_same1_pipe1_covers0_ordered0 cover=0 join=1 wait=none
round_same1_pipe1_covers0_ordered1 cover=0 join=1 wait=none
round_same1_pipe1_covers1_ordered0 cover=0 join=1 wait=none
round_same1_pipe1_covers1_ordered1 cover=0 join=1 wait=none
reuse_same_stream stream_order
reuse_covered covered
reuse_covered_not_ordered tick_events
reuse_ordered_not_covered tick_events
reuse_ring_14_back tick_events
reuse_ring_15_back join_then_event
reuse_this_tick_ordered covered
reuse_this_tick_not_ordered tick_events
reuse_token lazy_token
reuse_never_read none
reuse_never_read_stale_seq none
take_hostwait0_covers1 keep=0 join=1 dirty=1 free_seq=40
take_hostwait0_covers0 keep=0 join=1 dirty=1 free_seq=40
take_hostwait1_covers1 keep=1 join=0 dirty=0 free_seq=40
take_hostwait1_covers0 keep=0 join=1 dirty=1 free_seq=40
take_not_flagged free_seq=0
queue_nothing_pending got=-1 pending= free=0,1,2,3,
queue_lag1_same_tick got=-1 pending=0@10, free=1,2,3,
queue_lag1_next_tick got=0 pending= free=1,2,3,
queue_lag2_next_tick got=-1 pending=0@10, free=1,2,3,
queue_lag2_one_later got=0 pending= free=1,2,3,
queue_three_two_due got=1 pending=2@11, free=3,0,
queue_released got=-1 pending=2@11, free=3,0,1,
queue_no_slot_free got=-1 pending=2@11,3@11,0@11,1@11, free=
queue_newest 1
queue_dropped got=-1 pending= free=
queue_reset got=0 pending= free=0,1,2,3,
signal_not_wanted seq=7 flagged=0 nev=0 mask=0 unjoined=0 covers=0
signal_not_one_class seq=7 flagged=0 nev=0 mask=0 unjoined=0 covers=0
signal_carries 10
signal_two_parts seq=7 flagged=1 nev=2 mask=6 unjoined=6 covers=1
signal_unflag_mixed seq=7 flagged=0 nev=2 mask=0 unjoined=6 covers=0
signal_begin seq=8 flagged=0 nev=0 mask=6 unjoined=6 covers=0
signal_context_stream seq=8 flagged=1 nev=1 mask=0 unjoined=6 covers=0
signal_one_part_other_unjoined seq=8 flagged=1 nev=1 mask=2 unjoined=6 covers=0
signal_after_join seq=8 flagged=1 nev=1 mask=2 unjoined=0 covers=1
calib_shared_queues none phase=Done best=-1
calib_off none phase=Done
calib_round1 tick=1024 start(0123) phase=Round1 windows=1
calib_round1 tick=1030 close_then_start(0132) phase=Round1 windows=2
calib_round1 tick=1036 close_then_start(0213) phase=Round1 windows=3
calib_round1 tick=1168 close_then_wait phase=Waiting windows=24
calib_round1_end windows=24 candidates=24 last=3210
calib_identity_appended poll=poll round2=start(0132) phase=Round2 schedule=0132,0213,0231,0123,0132,0213,0231,0123,0132,0213,0231,0123,0132,0213,0231,0123, ticks=5:close_then_start(0213),9:close_then_start(0231),13:close_then_start(0123),17:close_then_start(0132),21:close_then_start(0213),25:close_then_start(0231),29:close_then_start(0123),33:close_then_start(0132),37:close_then_start(0213),41:close_then_start(0231),45:close_then_start(0123),49:close_then_start(0132),53:close_then_start(0213),57:close_then_start(0231),61:close_then_start(0123),65:close_then_wait, windows=16 pick=done(0213) phase=Done best=216
calib_identity_among poll=poll round2=start(0132) phase=Round2 schedule=0132,0123,0213,0132,0123,0213,0132,0123,0213,0132,0123,0213, ticks=5:close_then_start(0123),9:close_then_start(0213),13:close_then_start(0132),17:close_then_start(0123),21:close_then_start(0213),25:close_then_start(0132),29:close_then_start(0123),33:close_then_start(0213),37:close_then_start(0132),41:close_then_start(0123),45:close_then_start(0213),49:close_then_wait, windows=12 pick=done(0213) phase=Done best=216
calib_round1_tie poll=poll round2=start(0321) phase=Round2 schedule=0321,1230,0123,0321,1230,0123,0321,1230,0123,0321,1230,0123, ticks=5:close_then_start(1230),9:close_then_start(0123),13:close_then_start(0321),17:close_then_start(1230),21:close_then_start(0123),25:close_then_start(0321),29:close_then_start(1230),33:close_then_start(0123),37:close_then_start(0321),41:close_then_start(1230),45:close_then_start(0123),49:close_then_wait, windows=12 pick=done(0321) phase=Done best=108
calib_equal_sums poll=poll round2=start(0132) phase=Round2 schedule=0132,0213,0231,0123,0132,0213,0231,0123,0132,0213,0231,0123,0132,0213,0231,0123, ticks=5:close_then_start(0213),9:close_then_start(0231),13:close_then_start(0123),17:close_then_start(0132),21:close_then_start(0213),25:close_then_start(0231),29:close_then_start(0123),33:close_then_start(0132),37:close_then_start(0213),41:close_then_start(0231),45:close_then_start(0123),49:close_then_start(0132),53:close_then_start(0213),57:close_then_start(0231),61:close_then_start(0123),65:close_then_wait, windows=16 pick=done(0132) phase=Done best=180
calib_equal_sums_of_two poll=poll round2=start(0132) phase=Round2 schedule=0132,0213,0231,0123,0132,0213,0231,0123,0132,0213,0231,0123,0132,0213,0231,0123, ticks=5:close_then_start(0213),9:close_then_start(0231),13:close_then_start(0123),17:close_then_start(0132),21:close_then_start(0213),25:close_then_start(0231),29:close_then_start(0123),33:close_then_start(0132),37:close_then_start(0213),41:close_then_start(0231),45:close_then_start(0123),49:close_then_start(0132),53:close_then_start(0213),57:close_then_start(0231),61:close_then_start(0123),65:close_then_wait, windows=16 pick=done(0213) phase=Done best=216
"""


def test_tick_order_cases(tmp_path):
    exe = str(tmp_path / "tick_order_cases")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "doorman_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "tick_order_cases.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=30).stdout
    got, want = out.splitlines(), EXPECTED.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want), (got[len(want):], want[len(got):])
