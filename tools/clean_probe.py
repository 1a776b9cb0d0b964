"""dm_store_clean against the host route it replaces, on one store in one process.

A 16M-row store of 1000-row resources (the re-layout probe's size) with 1% of its rows
lapsed, in two states:
  explicit   as loaded: every row carries its own expiry, the lapsed rows scattered
  followers  after a writeback tick: every live row a follower of its (dense) resource, the
             lapsed rows being the resources whose lease is shorter than the wait
Timed on a fresh state every time (the released rows are put back, and in the followers
state a writeback tick makes them followers again), the routes alternating:
  peek          dm_store_clean(DM_CLEAN_PEEK) alone
  device route  dm_store_clean + dm_read_cleaned of the whole list
  host route    dm_read_store of the expiry column, the predicate in numpy, dm_store_release
Host wall time around each route (all three are synchronous); medians after a warm-up.
One more clean per state runs with the library's profiling on, for the HIP-event time of
its two passes.
The PCIe bytes are what the code moves: the device route 8 B per released row + the 16-B
result, the host route 8 B per row read + 8 B per released row sent.
usage: python tools/clean_probe.py [--rows 16000000] [--out profiles/clean_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (first: the library binds to the HIP runtime torch loads)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from doorman_amd import workloads as W  # noqa: E402
from doorman_amd.engine import Engine, _ptr  # noqa: E402

S = W.NS


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16_000_000)
    ap.add_argument("--clients", type=int, default=1000)
    ap.add_argument("--lapsed", type=float, default=0.01)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    R = a.rows // a.clients
    rng = np.random.default_rng(5)
    snap = W.uniform(R, a.clients, kind="mixed", seed=5)
    N = len(snap["wants"])
    now = W.NOW_NS
    eng = Engine(0)
    exp_buf = np.empty(N, np.int64)

    def host_route(when):
        eng._chk(eng._L.dm_read_store(eng._ctx, 0, N, None, None, None, _ptr(exp_buf)))
        rows = np.flatnonzero((exp_buf != W.RELEASED) & (when > exp_buf))
        eng.release(rows)
        return rows

    def measure(fresh, when_of):
        """fresh(k) brings the store into the state's k-th fresh copy; when_of(k) is the
        time its clean runs at."""
        peek, dev, host, released = [], [], [], None
        for k in range(a.runs + 2):
            fresh(3 * k)
            tp, p = wall(lambda: eng.clean(when_of(3 * k), peek=True, want_rows=False))
            td, d = wall(lambda: eng.clean(when_of(3 * k)))
            fresh(3 * k + 1)
            th, h = wall(lambda: host_route(when_of(3 * k + 1)))
            assert p["released"] == d["released"] == len(d["rows"]) == len(h), (p["released"], d["released"], len(h))
            assert np.array_equal(d["rows"], h)
            released = len(h)
            if k >= 2:  # warm-up: the first calls allocate
                peek.append(tp)
                dev.append(td)
                host.append(th)
        # the two passes' HIP-event time (the library's own profiling: the count pass with its
        # scan and reduction, then the apply pass, both under the store_release class)
        k = 3 * (a.runs + 2)
        fresh(k)
        eng.set_profiling(True)
        eng.reset_kernel_times()
        eng.clean(when_of(k), want_rows=False)
        launches, kernels_ms = eng.kernel_times()["store_release"]
        eng.set_profiling(False)
        med = statistics.median
        return {"released_rows": released,
                "clean_passes_ms_events": round(kernels_ms, 4), "clean_passes_launch_groups": launches,
                "peek_ms_wall_median": round(med(peek), 3),
                "device_route_ms_wall_median": round(med(dev), 3),
                "device_route_ms_wall_all": [round(x, 3) for x in dev],
                "host_route_ms_wall_median": round(med(host), 2),
                "host_route_ms_wall_all": [round(x, 2) for x in host],
                "host_over_device": round(med(host) / med(dev), 1),
                "device_route_pcie_bytes": 8 * released + 16,
                "host_route_pcie_bytes": 8 * N + 8 * released}

    # -- explicit: 1% of the rows, scattered, expired a second ago --
    lapsed = np.sort(rng.choice(N, int(N * a.lapsed), replace=False))
    snap["expiry_ns"][:] = now + 300 * S
    snap["expiry_ns"][lapsed] = now - S
    eng.load(snap)
    back = (lapsed, snap["has"][lapsed], snap["wants"][lapsed], snap["subclients"][lapsed], snap["expiry_ns"][lapsed])
    explicit = measure(lambda k: eng.upsert(*back) if k else None, lambda k: now)
    assert explicit["released_rows"] == len(lapsed)

    # -- followers: 1% of the resources hold 10-s leases, the rest 300-s ones; a writeback tick
    # at T makes every live row a follower, the clean runs a minute later --
    short = np.sort(rng.choice(R, max(int(R * a.lapsed), 1), replace=False))
    snap["lease_length_s"][:] = 300
    snap["lease_length_s"][short] = 10
    snap["expiry_ns"][:] = now + 300 * S
    eng.load(snap)
    rows = (short[:, None] * a.clients + np.arange(a.clients)[None, :]).ravel().astype(np.int64)
    arrivals = (rows, snap["has"][rows], snap["wants"][rows], np.ones(len(rows), np.int32), None)

    def fresh_followers(k):
        t = now + 100 * k * S
        if k:
            eng.apply(upsert=arrivals, now_ns=t)
        eng.apportion(t, writeback=True)
        eng.sync()

    fresh_followers(0)
    stats = eng.store_stats()
    followers = measure(lambda k: fresh_followers(k + 1), lambda k: now + (100 * (k + 1) + 60) * S)
    followers["dense_resources"] = stats["dense_resources"]
    assert followers["released_rows"] == len(rows)

    out = {"rows": N, "resources": R, "rows_per_resource": a.clients, "lapsed_fraction": a.lapsed, "runs": a.runs,
           "explicit": explicit, "followers": followers}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    eng.close()


if __name__ == "__main__":
    main()
