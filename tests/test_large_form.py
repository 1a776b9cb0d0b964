"""The form of a tick's large-resource chain (doorman_amd/csrc/dm_large_form.h): the output
column, the chain's flags (het, b_first, s_live), whether the tick takes the speculative form,
which build its redo runs and whether the host-mapped `seen` word is asked, and the launches
in order.

The header is plain C++17, so the rule runs on the CPU: tests/large_form_cases.cpp includes it
alone.  Beside it that file holds a transcription of the expressions Tick::outputs() and
Tick::large_chain() held before the header existed, which derived the speculative form twice
from different terms, and runs both over every combination of the inputs (every boolean, the
three column-flag states, 0 and 3 chunks, DM_REDO_LIGHT 0, 1 and 2, the word clear and set).
Its first line counts the cases in which any output differs, and the cases that break

    spec == spec_eligible && !inplace
    spec implies pingpong && !het && b_first && writeback && nchunks > 0

The table below is for readers; it was written from the same earlier code.  A line reads
`<case> <pingpong><het><b_first><s_live><spec><ask_seen><leaves_live> <launches>`; the cases
start from the steady speculative tick: a writeback tick of a store with large resources, no
explicit-expiry rows, nothing written since the last tick, the `seen` word clear.
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = """\
steady_spec 1011111 SPEC,REDO_LIGHT
spec_chain_off 0011001 A,B,C,MAP
not_writeback 0011000 A,B,C,MAP
recompute 0001001 A,B,C,MAP
explicit_rows 0000001 A,B,C,MAP
may_general 0100000 A,B,T,C,C_HET,E,MAP,MAP_HET,FIN
no_chunks 0011000 -
inplace 0011001 A,B,C,MAP
inplace_stream_written 0011001 A,B,C,MAP
alternate 1011111 SPEC,REDO_LIGHT
alternate_spec_off 1011001 A,B,C,MAP
stream_written_spec_off 1011001 A,B,C,MAP
chain_not_live 0010001 A,B,C,MAP
het_not_writeback 0100000 A,B,T,C,C_HET,E,MAP,MAP_HET,FIN
may_general_no_chunks 0011000 -
redo_light_0 1011101 SPEC,REDO_FULL
redo_light_1_unseen 1011111 SPEC,REDO_LIGHT
redo_light_1_seen 1011111 SPEC,REDO_FULL
redo_light_1_rows_written 1011101 SPEC,REDO_FULL
redo_light_2_seen 1011101 SPEC,REDO_LIGHT
redo_light_2_rows_written 1011101 SPEC,REDO_LIGHT
seen_not_asked_rows_written 1011101 SPEC,REDO_FULL
seen_not_asked_redo_light_0 1011101 SPEC,REDO_FULL
seen_not_asked_no_spec 0011001 A,B,C,MAP
"""


def test_large_form_cases(tmp_path):
    exe = str(tmp_path / "large_form_cases")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "doorman_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "large_form_cases.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=30).stdout
    head, got = out.splitlines()[0], out.splitlines()[1:]
    m = re.fullmatch(r"cases (\d+) disagreements (\d+) sequence_mismatches (\d+) \(het (\d+) plain (\d+)\) "
                     r"identity_violations (\d+) implication_violations (\d+)", head)
    assert m, head
    cases, disagree, seq_bad, seq_het, seq_plain, identity, implied = (int(v) for v in m.groups())
    assert cases == 256 * 3 * 2 * 3 * 2
    assert disagree == 0, head      # no output field differs from the earlier code's, the word's reading included
    assert identity == 0, head      # spec == spec_eligible && !inplace
    assert implied == 0, head       # spec implies pingpong && !het && b_first && writeback && nchunks > 0
    assert seq_bad == 0 and seq_het > 0 and seq_plain > 0, head  # the earlier kSeq walk, with het and without
    want = EXPECTED.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want), (got[len(want):], want[len(got):])
