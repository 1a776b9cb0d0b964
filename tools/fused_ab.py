"""The fused form against the two-kernel forms at a given listed share: where the threshold of
dm_split_form.h fused_limit comes from.

  python tools/fused_ab.py [--resources 100000] [--runs 10] [--shares 0,1e-4,1e-3,1e-2,1e-1,1]
                           [--chunk-lib tools/ab_libs/chunk32.so] [--out FILE.md]

tools/keep_keys_ab.py's store (R resources x 1,000 rows, FairShare, every resource under
capacity, at its fixed point, in place) in engines of one process: "two" with DM_FUSED=0 (the
sweep, the row kernel, the rest kernel), "fused" with DM_FUSED=2 (one launch whatever count the
device told), and with --chunk-lib a second fused engine from a build with another
kFusedChunk (make variant NAME=chunk32 DEFS=-DDM_FUSED_CHUNK=32).  All under dm_keep_keys 1:
a round refreshes one row in each of k = share x R resources with a changed value, which
clears those k keys and keeps the row epoch, so the next tick lists exactly k items; then a
synchronous writeback tick, timed alone on the host clock.  The engines take turns, run by
run; two rounds settle, `runs` are timed, three more run under dm_set_profiling for the dense
and rest classes' device time.  share 1 is the mispredicted tick: fused chosen and every item
listed.

Prints one JSON line; --out also writes the table as Markdown.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from doorman_amd import workloads as W  # noqa: E402
from keep_keys_ab import spread  # noqa: E402
from sweep_share import all_fixed_store  # noqa: E402

NOW = W.NOW_NS
STEP = 1.0 / 1024


def engine(snap, fused, lib=None):
    from doorman_amd.engine import Engine
    os.environ["DM_FUSED"] = fused  # read when the context is created
    try:
        e = Engine(0, lib)
    finally:
        del os.environ["DM_FUSED"]
    e.keep_keys(1)
    e.load(snap)
    for _ in range(5):  # hints, keys written, keys used and the count told, fused
        e.apportion(NOW, writeback=True)
    R = len(snap["seg_off"]) - 1
    assert e.store_stats()["fixed_items"] == R, e.store_stats()
    assert (e.plan_info()["fused_parts"] > 0) == (fused != "0"), e.plan_info()
    return e


def rounds(engs, snap, k, runs, rng):
    R = len(snap["seg_off"]) - 1
    clients = len(snap["wants"]) // R
    rows = (rng.choice(R, k, replace=False).astype(np.int64) * clients + rng.integers(0, clients, k)).astype(np.int64)
    base = snap["wants"][rows].copy()
    vals = (base, base + STEP)
    n = {name: 0 for name in engs}

    def round_of(name):
        e = engs[name]
        n[name] += 1
        if k:
            e.update_wants(rows, vals[n[name] & 1])
        t0 = time.perf_counter()
        e.apportion(NOW, writeback=True)
        return 1e6 * (time.perf_counter() - t0)

    for _ in range(2):
        for name in engs:
            round_of(name)
    times = {name: [] for name in engs}
    for _ in range(runs):
        for name in reversed(list(engs)):
            times[name].append(round_of(name))
    out = {}
    for name, e in engs.items():
        e.set_profiling(True)
        e.reset_kernel_times()
        for _ in range(3):
            round_of(name)
        kt = e.kernel_times()
        e.set_profiling(False)
        out[name] = {"tick_us": spread(times[name]), "runs": [round(t, 1) for t in times[name]],
                     "classes_us": {c: round(1000.0 * ms / 3, 1) for c, (_, ms) in sorted(kt.items())
                                    if c.endswith("_dense") or c.endswith("_rest")},
                     "fused_parts": e.plan_info()["fused_parts"]}
    for e in engs.values():  # back at the stored values and the fixed point
        if k:
            e.update_wants(rows, base)
        for _ in range(4):
            e.apportion(NOW, writeback=True)
    return out


def markdown(out):
    names = list(out["cases"][0]["engines"])
    L = ["| listed share | k | " + " | ".join("%s: tick us, median (min - max); classes" % n for n in names) + " |",
         "|---|---|" + "---|" * len(names)]
    for c in out["cases"]:
        cells = []
        for n in names:
            r = c["engines"][n]
            t = r["tick_us"]
            cells.append("%.1f (%.1f - %.1f); %s" % (t["median"], t["min"], t["max"],
                                                     ", ".join("%s %.1f" % kv for kv in r["classes_us"].items())))
        L.append("| %g | %d | %s |" % (c["share"], c["k"], " | ".join(cells)))
    return "\n".join(L) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--resources", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--shares", default="0,1e-4,1e-3,1e-2,1e-1,1")
    ap.add_argument("--chunk-lib", default=None, help="a build with another kFusedChunk (tools/ab_libs/NAME.so)")
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(3)
    t0 = time.perf_counter()
    snap = all_fixed_store(a.resources)
    engs = {"two": engine(snap, "0"), "fused": engine(snap, "2")}
    if a.chunk_lib:
        engs["fused_chunk"] = engine(snap, "2", a.chunk_lib)
    out = {"resources": a.resources, "runs": a.runs, "cases": []}
    try:
        for s in (float(x) for x in a.shares.split(",") if x):
            k = min(a.resources, int(round(s * a.resources)))
            out["cases"].append({"share": s, "k": k, "engines": rounds(engs, snap, k, a.runs, rng)})
            print(json.dumps(out["cases"][-1]), flush=True)
    finally:
        for e in engs.values():
            e.close()
    out["seconds"] = round(time.perf_counter() - t0, 1)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(markdown(out))
