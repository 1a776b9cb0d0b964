"""dm_keep_keys' DM_KEEP_FREE_SLOTS side by side with mode 3: what a writeback tick costs on a
store of which a share of the resources holds a free slot.

  python tools/free_slots_ab.py [--resources 100000] [--runs 10] [--shares 0.01,0.3,1.0]
                                [--parent tools/ab_libs/parent.so [--parent-mode 7]] [--out profiles/free_slots_ab.md]

A store of configs[3]'s shape (R resources x 1,000 rows, FairShare, every resource under
capacity with wants multiples of 2^-10: tools/sweep_share.py's) is loaded into two engines in
one process, dm_keep_keys modes 3 and 7, and with --parent into a third, mode 3 on another
build of the library (the commit before the bit).  In a share f of the resources one row is
released (one row per resource in one dm_store_release call: one atomic per sum, no order to
show), and eight synchronous writeback ticks bring every engine to its steady state.  Then
`runs` timed rounds of one synchronous writeback tick each (host clock around the call), the
engines taking turns run by run; first in place, then, after eight more ticks to settle, with
DM_WB_ALTERNATE.  Per case and engine: median and range, the form of the last tick
(dm_plan_info) and the valid keys (dm_store_stats).

What counts as a gain: at a share, every mode-7 run below every mode-3 run (of this build and
of the parent's).  The ratio is stated as measured against the parent.

Prints one JSON line; --out also writes the table as Markdown.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from doorman_amd import workloads as W  # noqa: E402
from sweep_share import all_fixed_store  # noqa: E402

NOW = W.NOW_NS
SETTLE = 8


def spread(xs):
    return {"median": round(statistics.median(xs), 1), "min": round(min(xs), 1), "max": round(max(xs), 1)}


def state(e):
    info, st = e.plan_info(), e.store_stats()
    return {k: info.get(k, 0) for k in ("fixed_parts", "sweep_parts", "cycle_parts", "masked_parts", "wb_inplace")} | {
        "fixed_items": st["fixed_items"], "mode": e.keep_stats()["mode"]}


def one_share(snap, f, runs, parent, rng, parent_mode=3):
    from doorman_amd.engine import Engine
    R = len(snap["seg_off"]) - 1
    clients = len(snap["wants"]) // R
    k = max(1, int(round(f * R)))
    res = np.sort(rng.choice(R, k, replace=False).astype(np.int64))
    rows = res * clients + rng.integers(0, clients, k)
    names = ["mode3", "mode7"] + (["parent_mode%d" % parent_mode] if parent else [])
    engs = [Engine(0), Engine(0)] + ([Engine(0, parent)] if parent else [])
    out = {"share": f, "holders": k}
    try:
        for e, m in zip(engs, (3, 7, parent_mode)):
            e.keep_keys(m)
            e.load(snap)
            e.release(rows)
        for column in ("inplace", "alternate"):
            tick = lambda e: e.apportion(NOW, writeback=True, wb_columns=column)  # noqa: E731
            for e in engs:
                for _ in range(SETTLE):
                    tick(e)
            times = [[] for _ in engs]
            for _ in range(runs):
                for i in reversed(range(len(engs))):
                    t0 = time.perf_counter()
                    tick(engs[i])
                    times[i].append(1e6 * (time.perf_counter() - t0))
            out[column] = {n: {"tick_us": spread(t), "runs": [round(x, 1) for x in t], **state(e)}
                           for n, t, e in zip(names, times, engs)}
        # the three stores hold the same bits
        ref = engs[0].read_store()
        for e in engs[1:]:
            st = e.read_store()
            for c in ("has", "wants"):
                assert np.array_equal(ref[c].view(np.int64), st[c].view(np.int64)), c
    finally:
        for e in engs:
            e.close()
    return out


def markdown(out):
    L = ["# dm_keep_keys modes 3 and 7: a writeback tick of a store with free slots", "",
         "`python tools/free_slots_ab.py%s` on one MI355X: %d resources x 1,000 rows, FairShare, under capacity; in a "
         "share f of the resources one row is released; every engine ticked to its steady state; then %d timed "
         "synchronous writeback ticks each, the engines taking turns run by run; host time of the tick in us "
         "(median, min - max).  Forms: parts whose last tick ran FIXED with keys / as the sweep / the cycle form / "
         "a masked build, then the valid keys." % (" --parent PARENT.so" if out["parent"] else "", out["resources"],
                                                    out["runs"]), "",
         "| f | column | engine | tick us | forms (fixed, sweep, cycle, masked), keys |", "|---|---|---|---|---|"]
    for c in out["cases"]:
        for col in ("inplace", "alternate"):
            for n, v in c[col].items():
                t = v["tick_us"]
                L.append("| %g | %s | %s | %.1f (%.1f - %.1f) | %d, %d, %d, %d; %d |"
                         % (c["share"], col, n, t["median"], t["min"], t["max"], v["fixed_parts"], v["sweep_parts"],
                            v["cycle_parts"], v["masked_parts"], v["fixed_items"]))
    L += ["", "| f | column | every mode-7 run below every mode-3 run | ... and every parent run | mode 7 / parent (medians) |",
          "|---|---|---|---|---|"]
    for c in out["cases"]:
        for col in ("inplace", "alternate"):
            v = c[col]
            m7, m3 = v["mode7"]["tick_us"], v["mode3"]["tick_us"]
            par = next((x["tick_us"] for n, x in v.items() if n.startswith("parent_mode")), None)
            L.append("| %g | %s | %s | %s | %s |"
                     % (c["share"], col, "yes" if m7["max"] < m3["min"] else "no",
                        ("yes" if m7["max"] < par["min"] else "no") if par else "-",
                        "%.3f" % (m7["median"] / par["median"]) if par else "-"))
    return "\n".join(L) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--resources", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--shares", default="0.01,0.3,1.0")
    ap.add_argument("--parent", default=None, help="the parent commit's build of the library, for a third engine")
    ap.add_argument("--parent-mode", type=int, default=3, help="the third engine's dm_keep_keys mode (7: the masked builds of both libraries side by side)")
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(3)
    t0 = time.perf_counter()
    snap = all_fixed_store(a.resources)
    out = {"resources": a.resources, "rows": int(len(snap["wants"])), "runs": a.runs, "parent": bool(a.parent),
           "cases": []}
    for f in (float(x) for x in a.shares.split(",") if x):
        out["cases"].append(one_share(snap, f, a.runs, a.parent, rng, a.parent_mode))
    out["seconds"] = round(time.perf_counter() - t0, 1)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(markdown(out))
