"""The host's plan of a round of requests (doorman_amd/csrc/dm_decide_plan.h): the request
checks, the stable order by resource, the work items of k_decide and of the fast path, the
`prev` links, the fast path's four areas, the event blocks' bounds, the scan-part count, and
the element count of every device buffer of the round.  The fast path's kernels index their
buffers by these numbers alone.

The header is plain C++17, so the plan runs on the CPU: tests/decide_plan_cases.cpp includes
it alone.  Beside it that file holds a transcription of the code dm_decide held before the
header existed (one 190-line function: its checks, grouping, items, offsets, bounds, and the
count of each `ensure` and `upload` line) and runs both over the smallest shapes at which each
rule can go wrong: requests at and below the fast path's threshold (kFdMin = 64), a resource
below it grouped between two above, request counts at and one past an event block (kFdBlock =
2048) and a scan chunk (kFdChunk = 1024) on resources smaller and larger than the round,
resources of 1, kFdRows = 4096 and 4097 rows, rows asked twice, once among others and never,
interleaved resources, resources of differing sizes, row 0 and the last row, the fast path
switched off, the four rejections behind a valid request, and a fixed sweep of mixed rounds.
Its first line counts the cases, the fields in which the plan differs from the earlier code
(every field of every item, every link, bound and buffer count, the error kind), and the
breaches of what the kernels need whatever either says (disjoint dense areas inside the
buffers' counts, blocks that tile an item's events, links to the nearest earlier request on
the same row of the same resource).

The table below is for readers; it was written from the earlier code's arithmetic.  A line
reads `<case> <error> order=<first 8> items=<resource>:<1 + fast slot>:<qlo>-<qhi>@<scratch
offset>,... scratch=<rows> fast=<item>:<k0>+<K>:n<rows>:blk<nblk>:ch<nch>:<m0>/<e0>/<b0>/<c0>:
r<repeats>,... mebc=<the areas' totals> parts=<scan parts> last_end=<the last block's end
bound> prev=<links set>`.
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = """\
below_min ok order=0,1,2,3,4,5,6,7 items=0:0:0-63@0 scratch=100 fast=- mebc=0/0/0/0 parts=0 last_end=-1 prev=empty:0
at_min ok order=0,1,2,3,4,5,6,7 items=0:1:0-64@0 scratch=100 fast=0:0+64:n100:blk1:ch1:0/0/0/0:r0 mebc=101/128/1/1 parts=1 last_end=128 prev=0
small_between ok order=1,3,5,7,9,11,13,15 items=0:1:0-64@0,1:0:64-127@100,2:2:127-191@200 scratch=300 fast=0:0+64:n100:blk1:ch1:0/0/0/0:r0,2:127+64:n100:blk1:ch1:101/128/1/1:r0 mebc=202/256/2/2 parts=1 last_end=256 prev=0
K2048_n2548 ok order=0,1,2,3,4,5,6,7 items=0:1:0-2048@0,1:2:2048-2112@2548 scratch=2628 fast=0:0+2048:n2548:blk1:ch1:0/0/0/0:r0,1:2048+64:n80:blk1:ch1:2549/4096/1/1:r0 mebc=2630/4224/2/2 parts=3 last_end=4224 prev=0
K2049_n2549 ok order=0,1,2,3,4,5,6,7 items=0:1:0-2049@0,1:2:2049-2113@2549 scratch=2629 fast=0:0+2049:n2549:blk2:ch1:0/0/0/0:r0,1:2049+64:n80:blk1:ch1:2550/4098/2/1:r0 mebc=2631/4226/3/2 parts=3 last_end=4226 prev=0
K1024_n1524 ok order=0,1,2,3,4,5,6,7 items=0:1:0-1024@0,1:2:1024-1088@1524 scratch=1604 fast=0:0+1024:n1524:blk1:ch1:0/0/0/0:r0,1:1024+64:n80:blk1:ch1:1525/2048/1/1:r0 mebc=1606/2176/2/2 parts=2 last_end=2176 prev=0
K1025_n1525 ok order=0,1,2,3,4,5,6,7 items=0:1:0-1025@0,1:2:1025-1089@1525 scratch=1605 fast=0:0+1025:n1525:blk1:ch1:0/0/0/0:r0,1:1025+64:n80:blk1:ch1:1526/2050/1/1:r0 mebc=1607/2178/2/2 parts=2 last_end=2178 prev=0
rows1 ok order=0,1,2,3,4,5,6,7 items=0:1:0-64@0,1:2:64-129@1 scratch=71 fast=0:0+64:n1:blk1:ch1:0/0/0/0:r1,1:64+65:n70:blk1:ch1:2/128/1/1:r0 mebc=73/258/2/2 parts=1 last_end=258 prev=63
rows4096 ok order=0,1,2,3,4,5,6,7 items=0:1:0-64@0,1:2:64-129@4096 scratch=4166 fast=0:0+64:n4096:blk1:ch1:0/0/0/0:r0,1:64+65:n70:blk1:ch1:4097/128/1/1:r0 mebc=4168/258/2/2 parts=5 last_end=258 prev=0
rows4097 ok order=0,1,2,3,4,5,6,7 items=0:1:0-64@0,1:2:64-129@4097 scratch=4167 fast=0:0+64:n4097:blk1:ch2:0/0/0/0:r0,1:64+65:n70:blk1:ch1:4098/128/1/2:r0 mebc=4169/258/2/3 parts=5 last_end=258 prev=0
one_row_chain ok order=0,1,2,3,4,5,6,7 items=0:0:0-1@0,1:1:1-71@9 scratch=109 fast=1:1+70:n100:blk1:ch1:0/0/0/0:r1 mebc=101/140/1/1 parts=1 last_end=140 prev=69
one_row_twice ok order=1,3,5,7,9,11,13,15 items=0:1:0-70@0,1:2:70-141@100 scratch=200 fast=0:0+70:n100:blk1:ch1:0/0/0/0:r0,1:70+71:n100:blk1:ch1:101/140/1/1:r1 mebc=202/282/2/2 parts=1 last_end=282 prev=1
interleaved ok order=1,4,7,10,2,5,8,11 items=0:0:0-4@0,1:0:4-8@4,2:0:8-12@9 scratch=15 fast=- mebc=0/0/0/0 parts=0 last_end=-1 prev=empty:0
interleaved_fast_off ok order=1,4,6,8,10,12,14,16 items=0:0:0-130@0,1:0:130-134@90,2:0:134-264@95 scratch=295 fast=- mebc=0/0/0/0 parts=0 last_end=-1 prev=empty:0
scratch_offsets ok order=1,4,2,0,3 items=0:0:0-2@0,2:0:2-3@5,3:0:3-4@6,4:0:4-5@4103 scratch=4115 fast=- mebc=0/0/0/0 parts=0 last_end=-1 prev=empty:0
extreme_rows ok order=1,0,2,3,4,5,6,7 items=0:0:0-1@0,2:1:1-66@3 scratch=73 fast=1:1+65:n70:blk1:ch1:0/0/0/0:r1 mebc=71/130/1/1 parts=1 last_end=130 prev=1
row_minus_1 row_range
row_N row_range
sub_minus_1 subclients
sub_over_max subclients
sub_fails_before_row subclients
row_fails_before_sub row_range
one_request_fails_both row_range
"""


def test_decide_plan_cases(tmp_path):
    exe = str(tmp_path / "decide_plan_cases")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "doorman_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "decide_plan_cases.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=30).stdout
    head, got = out.splitlines()[0], out.splitlines()[1:]
    m = re.fullmatch(r"cases (\d+) disagreements (\d+) invariant_violations (\d+) \(fast rounds (\d+) rejected (\d+)\)", head)
    assert m, head
    cases, disagree, broken, fast_rounds, rejected = (int(v) for v in m.groups())
    assert cases == 197
    assert disagree == 0, head  # no field differs from the earlier code's
    assert broken == 0, head    # every area inside its buffer, every link and bound where the kernels expect it
    assert fast_rounds > 100 and rejected == 7, head
    want = EXPECTED.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want), (got[len(want):], want[len(got):])
