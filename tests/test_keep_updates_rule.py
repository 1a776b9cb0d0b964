"""dm_keep_keys' DM_KEEP_UPDATES on the CPU: which calls it keeps (doorman_amd/csrc/
dm_row_epoch.h) and what the form's choice makes of a kept update (dm_split_form.h).

Both headers are plain C++17: tests/keep_updates_cases.cpp includes them alone and prints one
line per case.  The tables below are written from the feature's statement, not from the
headers:

  * the mode is a bit set; any non-zero value keeps the two wants refreshes as mode 1 did
    (deferred, the key-clearing build only while keys are in use, kept unless rejected or NaN);
  * bit 2 keeps release, upsert and the synchronous apply in the same way; kUpdNotOne is not
    an outcome that ends it (only a rejected part or a NaN does);
  * every other writer (load, plan, apply_async, decide, clean, relayout, config_load,
    root_tick) starts a row epoch before it launches under every mode;
  * modes 0 and 1 are the table of tests/test_row_epoch.py for all 13 writers, and the two
    functions of that test answer as the new ones do (`legacy_same=1`).

The form (a line reads `<case> <split><steady><skip_rest><fixed><use_keys><sweep> rest= list=
live=`; a part of 1000 items at its fixed point in row epoch 7 with keys in use):

  * the added inputs' defaults print what tests/test_split_form.py expects for the same cases;
  * with the bit set, a tick that can run the FIXED build (steady allowed, one stream part, no
    recompute, writeback in place) keeps the steady, FIXED and sweep forms and fix_live while
    the items not dense, the items with mask bits and the rows written since the count are
    together at most n / 4 -- pending update or not; at n / 4 + 1 the part runs today's forms;
  * a pending update (the record is the host's copy) never yields skip_rest: 1,920
    combinations of every other input;
  * the row kernel's grid hint counts the kept updates' rows as it counts refreshed values:
    t = told + rows -> max(16, t + t / 8 + (64 if t else 0)), at most the part's items.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WRITERS = ("refresh", "refresh_mask", "load", "plan", "upsert", "release", "apply", "apply_async", "decide", "clean",
           "relayout", "config_load", "root_tick")
REFRESHES = ("refresh", "refresh_mask")
UPDATES = ("upsert", "release", "apply")
ALWAYS_EPOCH = "ok=epoch nan=epoch rejected=epoch nan+rejected=epoch"
KEPT = "ok=kept nan=epoch rejected=epoch nan+rejected=epoch"


def expected_rule():
    lines = []
    for mode in (0, 1, 2, 3):
        for w in WRITERS:
            for keys in (0, 1):
                keeps = (mode != 0 and w in REFRESHES) or (mode & 2 and w in UPDATES)
                if keeps:
                    lines.append(f"{w} mode={mode} keys={keys} -> defer=1 build={'keys' if keys else 'plain'} | {KEPT}")
                else:
                    lines.append(f"{w} mode={mode} keys={keys} -> defer=0 build=plain | {ALWAYS_EPOCH}")
    return lines


FIXED_WITH_KEYS = "110111 rest=16 list=16 live=7"
DENSE_REST = "100000 rest=16 list=16 live=0"
DENSE_ALONE = "101000 rest=16 list=16 live=0"

EXPECTED_FORM = f"""\
legacy_same=1
default_fixed_next_tick {FIXED_WITH_KEYS}
default_some_undense {DENSE_REST}
default_released_rows_only {DENSE_ALONE}
default_two_parts {DENSE_ALONE}
bit_clear_released_rows {DENSE_ALONE}
bit_set_not_writeback {DENSE_ALONE}
bit_set_alternate_column {DENSE_ALONE}
bit_set_recompute {DENSE_ALONE}
bit_set_steady_off {DENSE_ALONE}
few_released_rows {FIXED_WITH_KEYS}
few_undense {FIXED_WITH_KEYS}
pending_one_row {FIXED_WITH_KEYS}
pending_bit_cleared {DENSE_REST}
pending_two_parts {DENSE_REST}
pending_record_of_older_epoch {DENSE_REST}
quarter_undense_250 {FIXED_WITH_KEYS}
quarter_undense_251 {DENSE_REST}
quarter_masks_250 {FIXED_WITH_KEYS}
quarter_masks_251 {DENSE_REST}
quarter_rows_250 {FIXED_WITH_KEYS}
quarter_rows_251 {DENSE_REST}
quarter_mixed_250 {FIXED_WITH_KEYS}
quarter_mixed_251 {DENSE_REST}
quarter_live_record_251 {DENSE_ALONE}
pending_never_skip_rest combos=1920 skip_rest=0
list_grid told=0 rows=0 -> 16 sweep=1
list_grid told=8 rows=0 -> 73 sweep=1
list_grid told=0 rows=100 -> 176 sweep=1
list_grid told=8 rows=100 -> 185 sweep=1
list_grid told=0 rows=200000 -> 100000 sweep=1
list_grid told=8 rows=200000 -> 100000 sweep=1
"""


def test_keep_updates_cases(tmp_path):
    exe = str(tmp_path / "keep_updates_cases")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "doorman_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "keep_updates_cases.cpp")], check=True)
    got = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=30).stdout.splitlines()
    want = expected_rule()
    assert len(want) == 4 * 13 * 2
    want += EXPECTED_FORM.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want), (got[len(want):], want[len(got):])


def test_modes_0_and_1_are_the_refresh_table():
    """The first half of the table above is tests/test_row_epoch.py's, line for line."""
    import test_row_epoch
    assert expected_rule()[:2 * 13 * 2] == test_row_epoch.expected()
