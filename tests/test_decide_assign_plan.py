"""The selection of a round's Assign (doorman_amd/csrc/dm_decide_assign.h): of a round of
requests, the grouped positions of the last request on each distinct row -- the requests whose
values dm_decide_assign gathers on the device and hands to the upsert's row step -- and the
element counts of the buffers that holds them.  The gather kernel indexes the round's columns
by these positions alone.

The header is plain C++17, so it runs on the CPU: tests/decide_assign_cases.cpp includes it
(and dm_decide_plan.h, whose plan it reads) and checks every round against a restatement with
a map: exactly one position per distinct row, that row's last request in the caller's order,
ascending positions inside the round, counts that cover what the kernels index.  The rounds:
no repeats; a row asked 2 and 3 times, adjacent and interleaved with other rows and other
resources; two rows interleaved; every request on one row; one request; 64 and 65 requests on
one resource (the fast path's threshold, where the plan also links repeats); requests arriving
in descending resource order; and a fixed sweep of 40 mixed rounds.

The table below was worked out by hand from the rounds (resources of 10, 100 and 20 rows: a
request's resource follows from its row; the grouped order is stable by resource).  A line
reads `<case> n=<requests> m=<selected> sel=<first 8 positions> rows=<their rows>
breaches=<failed checks>`.
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = """\
no_repeats n=5 m=5 sel=0,1,2,3,4 rows=3,4,12,13,111 breaches=0
twice_adjacent n=3 m=2 sel=1,2 rows=3,12 breaches=0
thrice_adjacent n=4 m=2 sel=0,3 rows=3,12 breaches=0
twice_interleaved n=5 m=4 sel=0,1,3,4 rows=3,4,12,111 breaches=0
thrice_interleaved n=8 m=6 sel=0,2,4,5,6,7 rows=3,13,14,12,111,112 breaches=0
two_rows_interleaved n=6 m=3 sel=2,4,5 rows=12,13,111 breaches=0
all_on_one_row n=9 m=1 sel=8 rows=57 breaches=0
one_request n=1 m=1 sel=0 rows=129 breaches=0
k64_one_resource n=64 m=63 sel=1,2,3,4,5,6,7,8 rows=11,12,13,14,15,16,17,18 breaches=0
k65_one_resource n=67 m=51 sel=1,17,18,19,20,21,22,23 rows=2,25,26,27,28,29,30,31 breaches=0
descending_resources n=9 m=6 sel=1,2,4,5,7,8 rows=0,9,10,50,111,120 breaches=0
"""


def test_decide_assign_cases(tmp_path):
    exe = str(tmp_path / "decide_assign_cases")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "doorman_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "decide_assign_cases.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=30).stdout
    head, got = out.splitlines()[0], out.splitlines()[1:]
    m = re.fullmatch(r"cases (\d+) named (\d+) breaches (\d+)", head)
    assert m, head
    cases, named, breaches = (int(v) for v in m.groups())
    assert cases == 51 and named == 11, head
    assert breaches == 0, out  # (the sweep's rounds print no line: the total counts them)
    want = EXPECTED.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want), (got[len(want):], want[len(got):])
