"""dm_store_relayout against the host route it replaces, on one store in one session.

A 16M-row dense store of 1000-row resources (C1's shape, every row a live follower after
two writeback ticks).  Timed:
  device route  dm_store_relayout growing every segment x2 (HIP events on the context
                stream around the call, and host wall time): median of 10 after warm-up;
                the shrink back to the first layout between runs is timed too
  host route    dm_read_store of every row + dm_read_resources, the permutation in numpy,
                dm_store_load with the running sums, dm_config_load (wall time; it is
                host-synchronous): median of 3
  tick          the writeback tick on the same store (HIP events), for the bandwidth the
                tick reaches beside the gather's
usage: python tools/relayout_probe.py [--rows 16000000] [--out profiles/relayout_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from doorman_amd import workloads as W  # noqa: E402
from doorman_amd.engine import Engine  # noqa: E402

HBM_PEAK = 8.0e12  # MI355X: 8 TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16_000_000)
    ap.add_argument("--clients", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    R = a.rows // a.clients
    snap = W.uniform(R, a.clients, kind="mixed", seed=5)
    N = len(snap["wants"])
    off1 = snap["seg_off"].copy()
    off2 = 2 * off1
    eng = Engine(0)
    ext = torch.cuda.ExternalStream(eng.stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(ext)
        fn()
        e1.record(ext)
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    eng.load(snap)
    now = W.NOW_NS
    for _ in range(3):
        now += W.NS
        eng.apportion(now, writeback=True)
    eng.sync()
    ticks = []
    for _ in range(20):
        now += W.NS
        ticks.append(timed(lambda: eng.apportion(now, writeback=True))[0])
    tick_ms = statistics.median(ticks)

    grow, shrink = [], []
    for i in range(a.runs + 2):
        g = timed(lambda: eng.relayout(off2))
        s = timed(lambda: eng.relayout(off1))
        if i >= 2:  # warm-up: the first calls allocate
            grow.append(g)
            shrink.append(s)
    # the kept rows are what the first layout held
    now += W.NS
    eng.apportion(now, writeback=True)

    def host_route():
        st = eng.read_store()
        res = eng.resources(safe=False)
        new = {"seg_off": off2, "has": np.zeros(2 * N), "wants": np.zeros(2 * N),
               "subclients": np.zeros(2 * N, np.int64), "expiry_ns": np.full(2 * N, W.RELEASED, np.int64)}
        dst = (np.arange(N, dtype=np.int64) + np.repeat(off1[:-1], a.clients))
        for k in ("has", "wants", "subclients", "expiry_ns"):
            new[k][dst] = st[k]
        new["agg_count"], new["agg_sum_has"], new["agg_sum_wants"] = res["count"], res["sum_has"], res["sum_wants"]
        eng.load_store(new)
        eng.load_config(snap)

    host = []
    for i in range(a.host_runs + 1 if a.host_runs > 0 else 0):
        t0 = time.perf_counter()
        host_route()
        dt = (time.perf_counter() - t0) * 1e3
        eng.relayout(off1)
        if i >= 1:
            host.append(dt)

    g_ev = statistics.median(x[0] for x in grow)
    g_wall = statistics.median(x[1] for x in grow)
    moved = 56 * N + 28 * N  # 28 B read + 28 B written per row kept, 28 B written per new free row
    out = {
        "rows": N, "resources": R, "rows_per_resource": a.clients,
        "relayout_grow_x2_ms_events_median": round(g_ev, 3),
        "relayout_grow_x2_ms_wall_median": round(g_wall, 3),
        "relayout_grow_x2_ms_events_all": [round(x[0], 3) for x in grow],
        "relayout_shrink_back_ms_events_median": round(statistics.median(x[0] for x in shrink), 3),
        "host_route_ms_wall_median": round(statistics.median(host), 1) if host else None,
        "host_route_ms_wall_all": [round(x, 1) for x in host],
        "host_route_pcie_bytes": 32 * N + 32 * 2 * N,
        "relayout_pcie_bytes": 8 * (R + 1) + 12,
        "relayout_hbm_bytes": moved,
        "relayout_call_GBps": round(moved / (g_ev * 1e-3) / 1e9, 1),
        "relayout_call_fraction_of_hbm_peak": round(moved / (g_ev * 1e-3) / HBM_PEAK, 4),
        "tick_writeback_ms_events_median": round(tick_ms, 4),
        "tick_GBps_at_28B_per_row": round(28 * N / (tick_ms * 1e-3) / 1e9, 1),
        "speedup_wall": round(statistics.median(host) / g_wall, 1) if host else None,
    }
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    eng.close()


if __name__ == "__main__":
    main()
