"""The host rule of the fused form (doorman_amd/csrc/dm_split_form.h choose_form,
PartForm::fused), on the CPU as tests/test_cycle_form.py runs the cycle form's:
tests/fused_form_cases.cpp includes the header alone.

Its table runs choose_form over every combination of the inputs the rule mentions (2^20 x 3
values of DM_STEADY x 4 told counts around the threshold) and checks each answer against the
rule as stated: a part runs fused when the bit is set (DM_FUSED), its form is the sweep or the
cycle form with keys in use, not masked, no judgement of CycleAuto pending, and the sweep
record is of this row epoch with told + refreshed at most the threshold.  Every other field
of the answer, fix_live and cyc_live included, is the one choose_form gives with the fused
form's inputs at their defaults, and with fused_ok false no answer is fused.

The counts follow from the rule.  With told in {0, limit - 1, limit, limit + 1} and refreshed
in {0, 1}, 5 of the 8 sums are within the limit.  The sweep: every input fixed but
DM_KEEP_FREE_SLOTS (the record has no marked item, so no masked build), cyc_live, DM_CYCLE and
the ask: 2 x 2 x 4 x 5 = 80.  The cycle form with keys in use: free are fix_live, DM_SWEEP and
DM_KEEP_FREE_SLOTS: 2 x 2 x 2 x 5 = 40.

The threshold: a 3,400th of the part's items, at least 4 (profiles/fused_ab.md)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = """\
table cases=12582912 fused=120 cycle=40 sweep=80
limit 4 4 4 29 4934
"""


def test_fused_form_cases(tmp_path):
    exe = str(tmp_path / "fused_form_cases")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "doorman_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "fused_form_cases.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    got, want = out.splitlines(), EXPECTED.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want), (got[len(want):], want[len(got):])


def test_engine_names_the_slot():
    from doorman_amd import engine
    assert engine._PLAN_NAMES[:len(engine._BIN_NAMES)] == engine._BIN_NAMES
    assert engine._PLAN_NAMES[26] == "fused_parts"
