"""The host rule of the carried root round (doorman_amd/csrc/dm_carry_rule.h), on the CPU as
tests/test_fused_form.py runs the fused form's: tests/carry_rule_cases.cpp includes the header
alone.

Its tables run the three functions over every combination of the inputs they mention and check
each answer against the rule as stated.  Carrying: the switch, the servers (1, 2, 8), the stream
and the template pipe, 2 x 3 x 2 x 2 = 24 cases of which one carries.  Riding: the work classes
(0..3), a workgroup bin or not, one part or two, k_general, writeback, the item count around the
leaf's resources (0, R - 1, R, R + 1) and the chosen form, 4 x 32 x 4 = 512 cases; 2 have the
shape (the form is free) and one of them rides.  Flushing: carried x held, one of four.

The order lines are the launches of eight steps (n: a tick that is not fused, f: a fused one, s: a
call that flushes): with the carry a round rides in the next fused tick, runs ahead of a tick
that is not, and a flush launches the last one; without it every round follows its tick.  The two
lines name the same launches in the same order: the carry only joins neighbours."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = """\
carry cases=24 carried=1
ride cases=512 shapes=2 rides=1
flush cases=4 flushed=1
order on  L0 R0 L1 R1+L2 R2+L3 R3+L4 R4 | L5 R5 L6 R6+L7 R7 |
order off L0 R0 L1 R1 L2 R2 L3 R3 L4 R4 | L5 R5 L6 R6 L7 R7 |
"""


def test_carry_rule_cases(tmp_path):
    exe = str(tmp_path / "carry_rule_cases")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "doorman_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "carry_rule_cases.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    got, want = [line.rstrip() for line in out.splitlines()], EXPECTED.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want), (got[len(want):], want[len(got):])
    on, off = got[3][len("order on  "):], got[4][len("order off "):]
    assert on.replace("+", " ") == off  # the same launches' work in the same order


def test_engine_names_the_slot():
    from doorman_amd import engine
    assert engine._PLAN_NAMES[26] == "fused_parts"
    assert engine._PLAN_NAMES[29] == "rounds_in_tick" and len(engine._PLAN_NAMES) == 30
