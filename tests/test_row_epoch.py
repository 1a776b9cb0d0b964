"""Which calls start a row epoch, and which build of the wants-refresh kernels runs
(doorman_amd/csrc/dm_row_epoch.h).

The header is plain C++17, so the rule runs on the CPU: tests/row_epoch_cases.cpp includes it
alone and prints one line per (writer, dm_keep_keys mode, keys in use), with how the call
ends for each outcome of its flags.  The lines are compared with the table below, which is
written from the feature's statement, not from the header:

  * mode off: every writer starts a row epoch before it launches (nothing is deferred) and
    launches the plain kernels, whatever its outcome;
  * mode on: the two refresh calls decide after their flags are back; they launch the
    key-clearing build only while some part has keys in use; a refresh is kept only when it
    was neither rejected nor flagged NaN;
  * mode on: every other writer (load, plan, upsert, release, the two batch calls, decide,
    clean, re-layout, config load, the root tick) behaves as with the mode off.  Those
    writers call dm_ctx::rows_changed() directly and never ask the header; their rows pin
    that the rule, asked, would not keep them (only the two refresh calls pass through it;
    tests/test_keep_keys_gpu.py::test_around_other_events checks the writers themselves).

After those lines, the sweep's grid hint (dm_split_form.h): a kept refresh's values are added
to the count the device last told before the margin of an eighth and 64, since each may have
cleared a key the device has not counted yet; with none refreshed the hint is what it was
(tests/test_split_form.py's list_grid cases).  The grid is a hint: the row kernel strides.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REFRESHES = ("refresh", "refresh_mask")
OTHERS = ("load", "plan", "upsert", "release", "apply", "apply_async", "decide", "clean", "relayout", "config_load",
          "root_tick")
ALWAYS_EPOCH = "ok=epoch nan=epoch rejected=epoch nan+rejected=epoch"


def expected():
    lines = []
    for mode in (0, 1):
        for w in REFRESHES + OTHERS:
            for keys in (0, 1):
                if mode == 1 and w in REFRESHES:
                    build = "keys" if keys else "plain"
                    lines.append(f"{w} mode=1 keys={keys} -> defer=1 build={build} | "
                                 "ok=kept nan=epoch rejected=epoch nan+rejected=epoch")
                else:
                    lines.append(f"{w} mode={mode} keys={keys} -> defer=0 build=plain | {ALWAYS_EPOCH}")
    return lines


def test_row_epoch_cases(tmp_path):
    exe = str(tmp_path / "row_epoch_cases")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "doorman_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "row_epoch_cases.cpp")], check=True)
    got = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=30).stdout.splitlines()
    want = expected()
    assert len(want) == 2 * 13 * 2
    # told + refreshed = t: max(16, t + t / 8 + (64 if t else 0)), at most the part's 100,000 items
    want += ["list_grid told=0 refreshed=0 -> 16 sweep=1", "list_grid told=0 refreshed=100 -> 176 sweep=1",
             "list_grid told=8 refreshed=100 -> 185 sweep=1", "list_grid told=1000 refreshed=0 -> 1189 sweep=1",
             "list_grid told=1000 refreshed=10000 -> 12439 sweep=1",
             "list_grid told=0 refreshed=200000 -> 100000 sweep=1"]
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want), (got[len(want):], want[len(got):])
