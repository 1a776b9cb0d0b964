"""What a store update's flags word means (doorman_amd/csrc/dm_update_outcome.h): the error
code and message of a rejected call or part, and what the value bits (a NaN wants, subclients
other than one) do to the context's maybe_general / all_sub_one.

The header is plain C++17, so the rule runs on the CPU: tests/update_outcome_cases.cpp includes
it alone.  Beside it that file holds a transcription of the three places that mapped the flags
before the header existed (finish_update with the single calls' tails, the masked refresh's
tail, apply_check) and runs both over every flags word the call's kernels can set:

    row upsert      Range, Dup, Sub, NaN, NotOne
    row refresh     Range, Dup, NaN
    release         Range, Dup
    masked refresh  Range, Count, NaN
    a batch         a triple (masked refresh, release, upsert), each word with the reject
                    bits carried from the one before; with arrivals and without; late or not

each with both prior values of maybe_general and of all_sub_one.  Its first line counts the
cases in which the code, the message or either resulting boolean differs.

The table below is for readers; it was written from the same earlier code.  A line reads
`<case> code=<code> general=<maybe_general> sub_one=<all_sub_one> "<message>"`, from
maybe_general clear and all_sub_one set (but `upsert_ones_into_mixed_store`: all_sub_one
clear); -1 is DM_E_INVAL, -5 DM_E_RANGE.
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = """\
upsert_ok code=0 general=0 sub_one=1 ""
upsert_not_one code=0 general=1 sub_one=0 ""
upsert_ones_into_mixed_store code=0 general=1 sub_one=0 ""
upsert_nan code=0 general=1 sub_one=1 ""
upsert_bad_subclients code=-1 general=0 sub_one=1 "subclients must be in [0, 2^31-2]"
upsert_duplicate_row code=-1 general=0 sub_one=1 "rows must be unique within one call"
upsert_range_and_duplicate code=-5 general=0 sub_one=1 "row out of range"
refresh_nan code=0 general=1 sub_one=1 ""
refresh_duplicate_row code=-1 general=0 sub_one=1 "rows must be unique within one call"
release_duplicate_row code=-1 general=0 sub_one=1 "rows must be unique within one call"
release_row_out_of_range code=-5 general=0 sub_one=1 "row out of range"
mask_bit_past_end code=-5 general=0 sub_one=1 "mask bit past the store's end"
mask_count_mismatch code=-1 general=0 sub_one=1 "packed values must match the mask's set bits"
mask_nan code=0 general=1 sub_one=1 ""
batch_ok code=0 general=0 sub_one=1 ""
batch_refresh_nan code=0 general=1 sub_one=1 ""
batch_count_mismatch_carried_into_upsert code=-1 general=0 sub_one=1 "wants refresh: packed values must match the mask's set bits"
batch_release_duplicate code=-1 general=0 sub_one=1 "release: rows must be unique within one part"
batch_release_duplicate_after_refresh_nan code=-1 general=1 sub_one=1 "release: rows must be unique within one part"
batch_upsert_bad_subclients code=-1 general=0 sub_one=1 "upsert: subclients must be in [0, 2^31-2]"
batch_upsert_range_after_clean_parts code=-5 general=0 sub_one=1 "upsert: row out of range"
batch_upsert_not_one code=0 general=1 sub_one=0 ""
batch_no_arrivals_word_ignored code=0 general=0 sub_one=1 ""
late_nan code=0 general=1 sub_one=1 ""
late_upsert_nan code=0 general=1 sub_one=1 ""
late_mask_bit_past_end code=-5 general=0 sub_one=1 "an earlier asynchronous batch's wants refresh: row out of range"
late_release_duplicate code=-1 general=0 sub_one=1 "an earlier asynchronous batch's release: rows must be unique within one part"
late_upsert_duplicate code=-1 general=0 sub_one=1 "an earlier asynchronous batch's upsert: rows must be unique within one part"
"""


def test_update_outcome_cases(tmp_path):
    exe = str(tmp_path / "update_outcome_cases")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "doorman_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "update_outcome_cases.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=30).stdout
    head, got = out.splitlines()[0], out.splitlines()[1:]
    m = re.fullmatch(r"cases (\d+) disagreements (\d+) \(single (\d+) batch (\d+)\)", head)
    assert m, head
    cases, disagree, single, batch = (int(v) for v in m.groups())
    # subsets of each call's bits x 4 priors; the batch's own bits per word x arrivals x late x 4 priors
    assert single == (32 + 8 + 4 + 8) * 4
    assert batch == 8 * 4 * 32 * 2 * 2 * 4
    assert cases == single + batch
    assert disagree == 0, head  # code, message, maybe_general and all_sub_one as the earlier code gave them
    want = EXPECTED.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want), (got[len(want):], want[len(got):])
