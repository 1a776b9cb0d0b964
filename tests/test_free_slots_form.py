"""dm_keep_keys' DM_KEEP_FREE_SLOTS in the launch form of a workgroup bin's stream part
(doorman_amd/csrc/dm_split_form.h: FormInputs::keep_free, FormInputs::rec_arrivals,
PartForm::masked), on the CPU as tests/test_split_form.py: tests/free_slots_form_cases.cpp
includes the header alone and prints one line per case.

The table was written from the rules as DESIGN.md §3.1 states them, not from the header:

  * with the bit clear choose_form ignores the new fields: over a grid of 8 density records x
    2^11 flag settings x 3 DM_STEADY values x 3 kept-row counts, an arrival count of 123
    changes no field of the result, and `masked` is never set;
  * with it set, a part of 1000 items that all carry a mask bit, verified in row epoch 7, with
    no arrival and no kept update's rows, runs steady: FIXED with keys and the sweep on a
    writeback tick in place, the cycle form on a cycle tick, the plain steady build on any
    other tick, each with `masked` set;
  * odd items are those not dense, those with an arrival bit and the rows of kept updates:
    250 of them keep the forms (a quarter of the part), 251 fall back to today's;
  * a record whose high half is zero gives `masked == false` (the kernels of today), unless
    it is a kept estimate and kept updates wrote rows since (each may have set a mask bit);
  * a recompute tick, a bin in two stream parts, DM_STEADY=0 and 2, an unverified record and
    a part that does not try the split stay off.

A line reads `<case> <split><steady><skip_rest><fixed><use_keys><sweep> cycle=<0|1>
masked=<0|1> live=<fix_live> cyc=<cyc_live>`.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = """\
bit_clear cases=147456 differ=0 masked=0
all_masked_inplace 110111 cycle=0 masked=1 live=7 cyc=0
all_masked_sweep_off 110110 cycle=0 masked=1 live=7 cyc=0
all_masked_keys_stale 110100 cycle=0 masked=1 live=7 cyc=0
all_masked_cycle 110010 cycle=1 masked=1 live=0 cyc=7
all_masked_cycle_first 110000 cycle=1 masked=1 live=0 cyc=7
all_masked_not_writeback 110000 cycle=0 masked=1 live=0 cyc=0
all_masked_alternate_unasked 110000 cycle=0 masked=1 live=0 cyc=0
bit_clear_all_masked 101000 cycle=0 masked=0 live=0 cyc=0
bit_clear_keep_updates 101000 cycle=0 masked=0 live=0 cyc=0
arrivals_250 110111 cycle=0 masked=1 live=7 cyc=0
arrivals_251 101000 cycle=0 masked=0 live=0 cyc=0
undense_250 110111 cycle=0 masked=1 live=7 cyc=0
undense_251 100000 cycle=0 masked=0 live=0 cyc=0
mixed_250 110111 cycle=0 masked=1 live=7 cyc=0
mixed_251 100000 cycle=0 masked=0 live=0 cyc=0
arrival_not_writeback 101000 cycle=0 masked=0 live=0 cyc=0
no_mask_bit 110111 cycle=0 masked=0 live=7 cyc=0
no_mask_bit_5_undense 110111 cycle=0 masked=0 live=7 cyc=0
kept_estimate_after_updates 110111 cycle=0 masked=1 live=7 cyc=0
recompute 101000 cycle=0 masked=0 live=0 cyc=0
two_parts 101000 cycle=0 masked=0 live=0 cyc=0
steady_off 101000 cycle=0 masked=0 live=0 cyc=0
steady_2 100000 cycle=0 masked=0 live=0 cyc=0
not_verified 100000 cycle=0 masked=0 live=0 cyc=0
not_tried 000000 cycle=0 masked=0 live=0 cyc=0
"""


def test_free_slots_form_cases(tmp_path):
    exe = str(tmp_path / "free_slots_form_cases")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "doorman_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "free_slots_form_cases.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=30).stdout
    got, want = out.splitlines(), EXPECTED.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want), (got[len(want):], want[len(got):])
