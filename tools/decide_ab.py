"""Interleaved A/B timing of dm_decide of two library builds in ONE process (as tools/ab.py).

  python tools/decide_ab.py PARENT.so [--new LIB.so ...] [--runs 10] [--out profiles/NAME.md]

Two rounds: the 100k-request round of test_decide_100k_requests_on_a_100k_client_resource (one fast item), and
200 requests on a 30-resource store (no fast item).  A run of a build is a fresh engine (the device time of a
round moves by a percent or two with where an engine's buffers happen to lie, so an engine kept for all runs
would measure its allocations, not its build): load, two warm-up calls, then three unprofiled calls (wall time)
and three profiled ones (the "decide" device time of dm_kernel_times), the median of each three.  The runs
alternate between the builds and the build that goes first rotates.  The parent's library is measured twice, the
second series as the control: what two series of one build differ by.  Per series: median, min and max of both
times, and the host share (wall - device: planning, staging, the copies, the launches and the wait).  Exit
status 1 when a median of a new build lies outside the range of the parent's first series.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (one HIP runtime)

from doorman_amd import workloads as W  # noqa: E402
from doorman_amd.engine import Engine  # noqa: E402
from test_server_gpu import NOW, _fast_round_snapshot  # noqa: E402


def round_100k():
    rng = np.random.default_rng(5)
    n = 100_000
    snap = _fast_round_snapshot(rng, np.array([n], np.int64), [W.FAIR_SHARE], [1])
    rows = rng.permutation(n).astype(np.int64)
    return snap, (rows, np.zeros(n), rng.uniform(0.0, 3.0, n) * snap["capacity"][0] / n, np.ones(n, np.int64))


def round_200():
    rng = np.random.default_rng(900)
    snap = W.add_store_sums(W.random_snapshot(rng, 30, 60))
    N = len(snap["wants"])
    rows = rng.choice(N, 200, replace=N < 200).astype(np.int64)
    cap_row = np.repeat(snap["capacity"], np.diff(snap["seg_off"]))
    return snap, (rows, np.zeros(200), rng.uniform(0, 2, 200) * cap_row[rows] / 10, np.maximum(snap["subclients"][rows], 1))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("--new", action="append", help="default: the tree's library")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    news = a.new or [os.path.join(ROOT, "doorman_amd", "libdoorman_hip.so")]
    libs = [("parent", a.parent)] + [("new" if len(news) == 1 else os.path.basename(p), p) for p in news]
    libs.append(("parent, a second series", a.parent))
    lines = ["# dm_decide, parent against new: wall and device time", "",
             "`tools/decide_ab.py`: one process, %d interleaved runs of each row, a fresh engine a run, the first build of a run rotating; us." % a.runs, "",
             "| round | build | wall median | wall min - max | device median | device min - max | host share (median wall - median device) |",
             "|---|---|---|---|---|---|---|"]
    outside = []
    for name, make in (("100k requests, one 100k-client resource", round_100k), ("200 requests, 30 resources", round_200)):
        snap, r = make()
        wall, dev, outs = [[] for _ in libs], [[] for _ in libs], [None] * len(libs)
        for k in range(a.runs):
            for i in [j % len(libs) for j in range(k, k + len(libs))]:
                with Engine(0, os.path.abspath(libs[i][1])) as e:
                    e.load(snap)
                    for _ in range(2):
                        outs[i] = tuple(x.tobytes() for x in e.decide(NOW, *r))
                    w, d = [], []
                    for _ in range(3):
                        e.sync()
                        t0 = time.perf_counter()
                        e.decide(NOW, *r)
                        w.append((time.perf_counter() - t0) * 1e6)
                    e.set_profiling(True)
                    for _ in range(3):
                        e.reset_kernel_times()
                        e.decide(NOW, *r)
                        d.append(e.kernel_times()["decide"][1] * 1e3)
                    wall[i].append(statistics.median(w))
                    dev[i].append(statistics.median(d))
        for i, (label, _) in enumerate(libs):
            mw, md = statistics.median(wall[i]), statistics.median(dev[i])
            lines.append("| %s | %s | %.1f | %.1f - %.1f | %.1f | %.1f - %.1f | %.1f (%.0f %%) |" % (
                name, label, mw, min(wall[i]), max(wall[i]), md, min(dev[i]), max(dev[i]), mw - md, 100 * (mw - md) / mw))
        for i in range(1, len(libs) - 1):
            for what, v in (("wall", wall), ("device", dev)):
                if not min(v[0]) <= statistics.median(v[i]) <= max(v[0]):
                    outside.append("%s: %s's %s median %.1f us lies outside the parent's %.1f - %.1f us" % (
                        name, libs[i][0], what, statistics.median(v[i]), min(v[0]), max(v[0])))
        same = all(o == outs[0] for o in outs)
        lines.append("| %s | outputs | %s | | | | |" % (name, "byte-equal" if same else "DIFFER"))
        if not same:
            outside.append("%s: the builds' outputs differ" % name)
    lines += [""] + (["Outside the parent's range:", ""] + ["- " + o for o in outside] if outside else
                     ["Every median of a new build lies inside the parent's range."])
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)
    return 1 if outside else 0


if __name__ == "__main__":
    sys.exit(main())
