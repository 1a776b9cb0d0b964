"""The host rule of the cycle form (doorman_amd/csrc/dm_split_form.h choose_form and
cycle_auto_step, dm_large_form.h choose_large), on the CPU as tests/test_split_form.py runs
the split form's: tests/cycle_form_cases.cpp includes the two headers alone.

Its table runs choose_form over every combination of the inputs a rule mentions (786,432)
and checks each answer against the rule as stated: the form is the steady builds' twin on a
writeback tick that writes the alternate column because the caller or a part asked; it trusts
the keys only when the part's last tick in this row epoch was a cycle-form tick (never the
FIXED build's fix_live); every other launch leaves cyc_live 0; and with DM_CYCLE=0, without
the ask, in place, or with DM_FIXED=0 every answer is the one choose_form gives without the
form's inputs.  The counts below follow from the rule: 80 = 16 combinations of the four
inputs the form ignores x 5 of (counts, kept record, DM_KEEP_UPDATES) that admit a steady
build; half of them with cyc_live current; 761,856 = all but the 2^12 x 6 in which the five
conditions of a cycle tick hold.

The other lines are sequences of cycle_auto_step from a part of a store beyond the Infinity
Cache whose in-place sweep tells 30,600 items every tick: it asks after kCycleTrigger = 8
consecutive such ticks; never with an empty list, a record of another epoch, a
cache-resident store or DM_CYCLE=0, nor when the list holds no more items than kept refreshes
wrote rows lately (recent := recent - recent / 8 + the tick's rows: 100 rows a tick against a
list of 100, or 10,000 against 30,600, whose sum passes 30,600 at the fourth tick; 1,000 a tick
reach 5,253 after eight and do not keep 30,600 from counting); an interruption or a new row epoch starts the count
over; it is judged by the count the device told with the stamp of the try's kCycleSettle-th
(8th) cycle-form launch, seen by the host on the 9th when the device keeps up and not before
that stamp arrives however far the host runs ahead (a tick that could not run the form
carries no stamp, and kCycleIdle = 16 of them in a row give the ask up as a failed try
does; an in-place sweep's count has stamp 0, and neither it nor the stamp an earlier try left
in the told word judges a later try); it stays if the count fell to half
at most, else waits 64 ticks, doubling to 4,096 (8 + the wait between tries)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = """\
table cases=786432 cycle=80 trusted=40 parent_same=761856
engages_after 8
engaged on=1 base=30600
empty_list -1
record_of_another_epoch -1
cache_resident_store -1
dm_cycle_0 -1
refresh_driven_list -1
persistent_beyond_refreshes 8 recent=5253
refreshes_outweigh -1
interrupted_then 8
new_epoch_then 8
engaged_new_epoch on=0
judged told=0 stays=1 after=-1 skip=0 wait=64
judged told=15300 stays=1 after=-1 skip=0 wait=64
judged told=15301 stays=0 after=9 skip=64 wait=128
judged told=30600 stays=0 after=9 skip=64 wait=128
device_behind on=1 judged=0 launches=50
device_caught_up on=1 judged=1
idle_ticks on=1 judged=0 launches=0 idle=15
idle_again on=1 idle=15
idle_gives_up on=0 skip=64 wait=128
second_try_stamp_0 on=1 judged=0
second_try_stale_stamp on=1 judged=0
backoff 8 72 136 264 520 1032 2056 4104 4104 wait=4096
column ok
"""


def test_cycle_form_cases(tmp_path):
    exe = str(tmp_path / "cycle_form_cases")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "doorman_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cycle_form_cases.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    got, want = out.splitlines(), EXPECTED.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want), (got[len(want):], want[len(got):])
