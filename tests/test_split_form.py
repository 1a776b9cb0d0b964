"""The launch form of a workgroup bin's stream part (doorman_amd/csrc/dm_split_form.h): the
back-off of the split form and the choice among mixed, dense + rest, dense alone, steady,
FIXED rewriting keys, FIXED with keys and the sweep, with the grids and the next fix_live.

The header is plain C++17, so the rules run on the CPU: tests/split_form_cases.cpp includes
it alone, prints one line per case, and the lines are compared with the table below.  The
table was written from Tick::bin_part as it stood before the header existed (one function
that made the same decisions inline), not from the header.

A line reads `<case> mixed live=<fix_live>` or
`<case> <split><steady><skip_rest><fixed><use_keys><sweep> rest=<grid> list=<grid> live=<fix_live>`;
the cases start from a part of 1000 items at its fixed point in row epoch 7 with keys in use.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = """\
no_hints mixed live=0
split_bit_clear mixed live=0
not_tried mixed live=0
backoff_tries 64 192 448 960 1984 4032 8128 12224 16320 wait=4096 skip=0
backoff_good_equal try=1 wait=64 skip=0
backoff_after_good next_try=64 wait=128
not_verified 100000 rest=16 list=16 live=0
verified_some_undense 100000 rest=16 list=16 live=0
verified_released_rows_only 101000 rest=16 list=16 live=0
verified_clean_two_parts 101000 rest=16 list=16 live=0
verified_clean_steady_off 101000 rest=16 list=16 live=0
verified_clean_steady_2 100000 rest=16 list=16 live=0
verified_clean_recompute 101000 rest=16 list=16 live=0
steady_not_writeback 110000 rest=16 list=16 live=0
steady_alternate_column 110000 rest=16 list=16 live=0
steady_fixed_off 110000 rest=16 list=16 live=0
fixed_keys_stale 110100 rest=16 list=16 live=7
fixed_keys_never 110100 rest=16 list=16 live=7
fixed_next_tick 110111 rest=16 list=16 live=7
fixed_next_tick_sweep_off 110110 rest=16 list=16 live=7
rest_grid_0 110111 rest=16 list=16 live=7
rest_grid_16 110111 rest=16 list=16 live=7
rest_grid_17 110111 rest=17 list=16 live=7
rest_grid_512 110111 rest=512 list=16 live=7
rest_grid_513 110111 rest=512 list=16 live=7
list_grid_stale_record 110111 rest=16 list=100000 live=7
list_grid_told_0 110111 rest=16 list=16 live=7
list_grid_told_8 110111 rest=16 list=73 live=7
list_grid_told_1000 110111 rest=16 list=1189 live=7
list_grid_margin_beyond_n 110111 rest=16 list=1000 live=7
"""


def test_split_form_cases(tmp_path):
    exe = str(tmp_path / "split_form_cases")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "doorman_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "split_form_cases.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=30).stdout
    got, want = out.splitlines(), EXPECTED.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want), (got[len(want):], want[len(got):])
