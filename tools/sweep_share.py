"""What the skip path of the FIXED dense kernel costs on its own: a store of configs[3]'s
shape (R resources x 1,000 rows, FairShare) in which every resource is at its fixed point
(every resource under capacity, wants multiples of 2^-10: gets == wants in any summation
order), ticked back to back as bench.py ticks.

  python tools/sweep_share.py [R] [STEPS]

Prints one JSON line: the `block128x8_dense` class time per launch (dm_kernel_times, HIP
events around every launch) and the step time between two events, with the keys in use
(every workgroup returns after its record) and, beside it, the same store with DM_FIXED=0
(every workgroup loads its rows).  The first figure is what a sweep that checks the keys
with one lane per item could remove, less its own time.
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from doorman_amd import workloads as W  # noqa: E402


def all_fixed_store(R, clients=1000, seed=11, capacity=1000.0):
    rng = np.random.default_rng(seed)
    N = R * clients
    # sum of wants <= C / 2, every wants a multiple of 2^-10
    wants = np.round(rng.uniform(0.0, 1.0, N) * (0.5 * capacity / clients) * 1024.0) / 1024.0
    has = wants * 0.5
    exp = W.NOW_NS + rng.integers(30, 300, N, dtype=np.int64) * W.NS
    return W.make_snapshot(np.full(R, clients), wants, has, 1, exp, W.FAIR_SHARE, capacity, 300, 5)


def measure(snap, steps, fixed):
    import torch
    from doorman_amd.engine import Engine
    if fixed:
        os.environ.pop("DM_FIXED", None)
    else:
        os.environ["DM_FIXED"] = "0"  # read when the context is created
    R = len(snap["seg_off"]) - 1
    with Engine(0) as eng:
        eng.load(snap)
        now = W.NOW_NS
        step = lambda: eng.apportion(now, writeback=True, asynchronous=True, defer_join=True)  # noqa: E731
        for _ in range(3):  # (synchronous: the host reads each tick's hint count before the next)
            eng.apportion(now, writeback=True)
        stats = eng.store_stats()
        if fixed:
            assert stats["fixed_items"] == R, stats
        for i in range(400):  # bench.py's warm ticks
            step()
            if i % 8 == 7:
                eng.sync()
        eng.sync()
        ext = torch.cuda.ExternalStream(eng.stream)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        ev0.record(ext)
        for _ in range(steps):
            step()
        eng.join()
        ev1.record(ext)
        eng.sync()
        torch.cuda.synchronize()
        step_us = 1000.0 * ev0.elapsed_time(ev1) / steps
        eng.set_profiling(True)
        eng.reset_kernel_times()
        for _ in range(steps):
            step()
        eng.sync()
        kt = eng.kernel_times()
        eng.set_profiling(False)
        info = eng.plan_info()
    return {"fixed_items": stats["fixed_items"], "fixed_parts": info["fixed_parts"],
            "sweep_parts": info.get("sweep_parts", 0), "step_us": round(step_us, 2),
            "kernel_us": {k: round(1000.0 * ms / n, 2) for k, (n, ms) in sorted(kt.items())}}


if __name__ == "__main__":
    R = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    t0 = time.perf_counter()
    snap = all_fixed_store(R)
    out = {"resources": R, "rows": int(len(snap["wants"])), "steps": steps,
           "keys_in_use": measure(snap, steps, True), "DM_FIXED=0": measure(snap, steps, False),
           "seconds": None}
    out["seconds"] = round(time.perf_counter() - t0, 1)
    print(json.dumps(out))
