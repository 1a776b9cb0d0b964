"""The store loaded from and read into device memory against the host calls, on one store in
one process, the routes interleaved run by run.

A store of 1000-row resources (16M rows by default; --rows 100000000 is C3's shape).  Host
wall time around each synchronous call, one warm-up of each route, then --runs runs:
  (a) host load     dm_store_load of the snapshot from pageable numpy arrays and from
                    page-locked ones (dm_host_alloc), without running sums (the host's
                    row-order loop) -- the code as it was before the device route existed
  (b) device load   dm_store_load_device of the same snapshot from torch tensors, with the
                    running sums given and without (the row-order sum pass on the device)
  (c) reads         read_store against read_store_device of every row, leases against
                    leases_device after a writeback tick
with the bytes each route moves, computed from the shapes (the kernels' and copies' loads and
stores), and the HBM rate of (b).  The sum pass's share of (b) is the difference of its two
forms: the pass with the sums given reads the same rows for maybe_general and leaves out
only the chains and the has column.
usage: python tools/device_io_probe.py [--rows 16000000] [--out profiles/device_io_probe.json]
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
STORE = ("seg_off", "wants", "has", "subclients", "expiry_ns")


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3),
            "all_ms": [round(x, 3) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16_000_000)
    ap.add_argument("--clients", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    R = a.rows // a.clients
    snap = W.uniform(R, a.clients, kind="mixed", seed=5)
    N = len(snap["wants"])
    eng = Engine(0)
    pageable = {k: np.ascontiguousarray(snap[k]) for k in STORE}
    pinned = {}
    for k in STORE:
        pinned[k] = eng.host_empty(len(pageable[k]), pageable[k].dtype)
        pinned[k][:] = pageable[k]
    dev = {k: torch.from_numpy(pageable[k]).to("cuda:0") for k in STORE}
    sums = W.add_store_sums({k: pageable[k] for k in STORE})
    dev_agg = dict(dev, **{k: torch.from_numpy(np.ascontiguousarray(sums[k])).to("cuda:0")
                           for k in ("agg_count", "agg_sum_has", "agg_sum_wants")})
    torch.cuda.synchronize()

    routes = {
        "host_load_pageable": lambda: eng.load_store(pageable),
        "host_load_pinned": lambda: eng.load_store(pinned),
        "device_load_sums_given": lambda: eng.load_store_device(dev_agg),
        "device_load_sums_recomputed": lambda: eng.load_store_device(dev),
    }
    t = {k: [] for k in routes}
    for i in range(a.runs + 1):
        for k, fn in routes.items():
            dt = wall(fn)
            if i >= 1:  # warm-up: the first calls allocate
                t[k].append(dt)

    # the two loads left the same store: the running sums of the last device load against the host's
    dev_res = eng.resources(safe=False)
    eng.load_store(pageable)
    host_res = eng.resources(safe=False)
    sums_equal = all(np.array_equal(np.ascontiguousarray(dev_res[k]).view(np.int64),
                                    np.ascontiguousarray(host_res[k]).view(np.int64))
                     for k in ("count", "sum_has", "sum_wants"))

    eng.load_config(snap)
    eng.apportion(W.NOW_NS + W.NS, writeback=True)
    reads = {
        "read_store_host": lambda: eng.read_store(),
        "read_store_device": lambda: eng.read_store_device(),
        "leases_host": lambda: eng.leases(),
        "leases_device": lambda: eng.leases_device(),
    }
    t.update({k: [] for k in reads})
    for i in range(a.runs + 1):
        for k, fn in reads.items():
            dt = wall(fn)
            if i >= 1:
                t[k].append(dt)

    # bytes, from the shapes.  Host load: wants, has, expiry at 8 B, subclients staged as 4 B,
    # seg_off, the 32-B sums records and the explicit flags.  Device load: the check (16 B
    # read), three column copies (16 B each), the subclients pass (8 in, 4 out), the
    # per-resource pass (wants, subclients, expiry; has too when it sums).
    host_pcie = 28 * N + 8 * (R + 1) + 33 * R
    dev_pcie = 8 * (R + 1) + 8
    dev_hbm = {"device_load_sums_given": (16 + 48 + 12 + 24) * N + 56 * R,
               "device_load_sums_recomputed": (16 + 48 + 12 + 32) * N + 32 * R}
    med = {k: statistics.median(v) for k, v in t.items()}
    chain = med["device_load_sums_recomputed"] - med["device_load_sums_given"]

    def below(devk, hostks):
        return all(max(t[devk]) < min(t[h]) for h in hostks)

    out = {
        "rows": N, "resources": R, "rows_per_resource": a.clients, "runs": a.runs,
        **{k: stats(v) for k, v in t.items()},
        "host_load_pcie_bytes": host_pcie,
        "device_load_pcie_bytes": dev_pcie,
        "device_load_hbm_bytes": dev_hbm,
        "device_load_GBps": {k: round(dev_hbm[k] / (med[k] * 1e-3) / 1e9, 1) for k in dev_hbm},
        "device_load_fraction_of_hbm_peak": {k: round(dev_hbm[k] / (med[k] * 1e-3) / HBM_PEAK, 4) for k in dev_hbm},
        "sum_pass_ms_by_difference": round(chain, 3),
        "sum_pass_share_of_device_load": round(chain / med["device_load_sums_recomputed"], 3),
        "read_store_host_pcie_bytes": 32 * N,
        "read_store_device_hbm_bytes": (32 + 12 + 16) * N,
        "leases_host_pcie_bytes": 16 * N,
        "leases_device_hbm_bytes": (16 + 12 + 8) * N,
        "sums_bit_equal_host_and_device_load": bool(sums_equal),
        "every_device_load_below_every_host_load": below("device_load_sums_given", ("host_load_pageable", "host_load_pinned"))
        and below("device_load_sums_recomputed", ("host_load_pageable", "host_load_pinned")),
        "every_device_read_below_every_host_read": below("read_store_device", ("read_store_host",))
        and below("leases_device", ("leases_host",)),
        "speedup_load_recomputed_vs_pinned": round(med["host_load_pinned"] / med["device_load_sums_recomputed"], 1),
        "speedup_read_store": round(med["read_store_host"] / med["read_store_device"], 1),
        "speedup_leases": round(med["leases_host"] / med["leases_device"], 1),
    }
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        both = {}
        if os.path.exists(a.out):  # one entry per size: a second run adds its own
            with open(a.out) as f:
                both = json.load(f)
        both[f"rows_{N}"] = out
        with open(a.out, "w") as f:
            json.dump(both, f, indent=1)
            f.write("\n")
    eng.close()


if __name__ == "__main__":
    main()
