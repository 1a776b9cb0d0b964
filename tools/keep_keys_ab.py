"""dm_keep_keys on and off, side by side: what a writeback tick costs after a wants refresh.

  python tools/keep_keys_ab.py [--resources 100000] [--runs 10] [--ks 100,1000,10000,100000]
                               [--refresh-resources 125000] [--out profiles/keep_keys_ab.md]

A store of configs[3]'s shape (R resources x 1,000 rows, FairShare, every resource under
capacity with wants multiples of 2^-10: tools/sweep_share.py's) is loaded into two engines
in one process, one with keep_keys(1), and brought to its fixed point.  A round refreshes
one row in each of k resources (dm_store_update_wants), then runs a synchronous writeback
tick; the same k resources every round, their rows' values alternating between two
multiples of 2^-10 ("changed") or re-sent as stored ("same").  Per (k, values) the two
engines take turns, run by run: two rounds to settle, then `runs` timed rounds each (host
clock around the refresh and the tick: both calls are synchronous), then three rounds under
dm_set_profiling for the tick's kernel classes (dm_kernel_times).  Medians and ranges.

Then the refresh calls alone at configs[4]'s refresh shape (a tenth of the rows by mask,
dm_store_update_wants_mask, over --refresh-resources x 1,000 rows): the engine with the mode
on and keys in use launches the key-clearing build, the other the plain one; the values are
the stored ones, so no key is cleared and no tick is needed between the calls.  The call's
host time (its copies included) per build.

--writer release,arrival,batch (DM_KEEP_UPDATES; --out profiles/keep_updates_ab.md): the two
engines run dm_keep_keys modes 1 and 3, so the first behaves as the commit before the bit did.
Per k, on the same store: "release" frees one row in each of k resources (dm_store_release),
"arrival" refills them (a narrow arrival through dm_store_apply: no expiry, the resource's
count), each followed by a synchronous writeback tick and timed with it, a release round and
an arrival round taking turns; "batch" is one dm_store_apply that frees one row in each of
the k resources and refills the row the batch before freed, then the tick.  Guidance: mode 3
pays for a tick that stays FIXED with a rest launch over the items that hold a released row
or an arrival, so it gains while those are few (at most a quarter of a bin's resources: above
that the tick runs as in mode 1, and the call has cleared keys for nothing).  Measured on the
100,000 x 1,000 store (profiles/keep_updates_ab.md): mode 3 takes a fifth to a quarter of mode
1's time at k = 100 and 1,000, four fifths at 10,000 for releases and arrivals; for a batch of
both at 10,000, and for every writer at 100,000, the two modes lie within each other's ranges
(mode 3's median 7 us above mode 1's for the batch at 100,000, 805 against 812 us): nothing
gained there, so a store whose every round writes a tenth of its resources or more can leave
the bit clear.

Prints one JSON line; --out also writes the tables as Markdown.
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
STEP = 1.0 / 1024
LIB = None  # --lib: another build of the library (make variant), for a run against a parent commit


def engines(snap, modes=(0, 1)):
    """(mode off, mode on), both at the store's fixed point with keys in use."""
    from doorman_amd.engine import Engine
    pair = (Engine(0, LIB), Engine(0, LIB))
    for e, m in zip(pair, modes):
        e.keep_keys(m)
    R = len(snap["seg_off"]) - 1
    for e in pair:
        e.load(snap)
        for _ in range(3):  # hints, keys written, keys used
            e.apportion(NOW, writeback=True)
        assert e.store_stats()["fixed_items"] == R, e.store_stats()
    return pair


def spread(xs):
    return {"median": round(statistics.median(xs), 1), "min": round(min(xs), 1), "max": round(max(xs), 1)}


def ab_rounds(pair, snap, k, changed, runs, rng):
    R = len(snap["seg_off"]) - 1
    clients = len(snap["wants"]) // R
    rows = (rng.choice(R, k, replace=False).astype(np.int64) * clients + rng.integers(0, clients, k)).astype(np.int64)
    base = snap["wants"][rows].copy()
    vals = (base, base + STEP) if changed else (base, base)
    n = [0, 0]
    out = {}

    def round_of(i):
        e = pair[i]
        n[i] += 1
        t0 = time.perf_counter()
        e.update_wants(rows, vals[n[i] & 1])
        e.apportion(NOW, writeback=True)
        return 1e6 * (time.perf_counter() - t0)

    for _ in range(2):
        for i in (0, 1):
            round_of(i)
    times = ([], [])
    for _ in range(runs):
        for i in (1, 0):
            times[i].append(round_of(i))
    for i, name in ((0, "off"), (1, "on")):
        e = pair[i]
        e.set_profiling(True)
        e.reset_kernel_times()
        for _ in range(3):
            round_of(i)
        kt = e.kernel_times()
        e.set_profiling(False)
        info = e.plan_info()
        out[name] = {"round_us": spread(times[i]), "runs": [round(t, 1) for t in times[i]],
                     "tick_kernels_us": {c: round(1000.0 * ms / 3, 1) for c, (_, ms) in sorted(kt.items())},
                     "fixed_parts": info["fixed_parts"], "sweep_parts": info["sweep_parts"],
                     "wb_inplace": info["wb_inplace"], "fixed_items": e.store_stats()["fixed_items"]}
    for e in pair:  # the store back at its values and its fixed point for the next case
        e.update_wants(rows, base)
        for _ in range(3):
            e.apportion(NOW, writeback=True)
    return out


def update_rounds(pair, snap, k, runs, rng, writers):
    """Modes 1 and 3 (pair[0], pair[1]): releases, arrivals and batches of both in k resources."""
    R = len(snap["seg_off"]) - 1
    clients = len(snap["wants"]) // R
    res = rng.choice(R, k, replace=False).astype(np.int64)
    first = rng.integers(0, clients - 1, k)
    X, Y = res * clients + first, res * clients + first + 1  # two rows of each resource
    one = np.ones(k, np.int32)
    tick = lambda e: e.apportion(NOW, writeback=True)  # noqa: E731
    arrive = lambda e, rows: e.apply(upsert=(rows, None, snap["wants"][rows], one, None), now_ns=NOW)  # noqa: E731

    def timed(e, call):
        t0 = time.perf_counter()
        call(e)
        tick(e)
        return 1e6 * (time.perf_counter() - t0)

    def state(e):
        info, ks = e.plan_info(), e.keep_stats()
        return {"fixed_parts": info["fixed_parts"], "sweep_parts": info["sweep_parts"],
                "wb_inplace": info["wb_inplace"], "fixed_items": e.store_stats()["fixed_items"],
                "kept": [ks["kept_releases"], ks["kept_batches"]]}

    out = {}
    if "release" in writers or "arrival" in writers:
        t_rel, t_arr, st_rel, st_arr = ([], []), ([], []), [None, None], [None, None]
        for r in range(runs + 2):
            for i in (1, 0):
                a = timed(pair[i], lambda e: e.release(X))
                st_rel[i] = state(pair[i])
                b = timed(pair[i], lambda e: arrive(e, X))
                st_arr[i] = state(pair[i])
                if r >= 2:
                    t_rel[i].append(a)
                    t_arr[i].append(b)
        for name, t, st in (("release", t_rel, st_rel), ("arrival", t_arr, st_arr)):
            out[name] = {m: {"round_us": spread(t[i]), "runs": [round(x, 1) for x in t[i]], **st[i]}
                         for i, m in ((0, "mode1"), (1, "mode3"))}
        for e in pair:
            for _ in range(3):
                tick(e)
    if "batch" in writers:
        for e in pair:  # one row of each resource free, as between two batches
            e.release(Y)
            tick(e)
        t, st = ([], []), [None, None]
        for r in range(runs + 2):
            free, take = (X, Y) if r % 2 == 0 else (Y, X)
            for i in (1, 0):
                cols = (take, None, snap["wants"][take], one, None)
                a = timed(pair[i], lambda e: e.apply(release_rows=free, upsert=cols, now_ns=NOW))
                st[i] = state(pair[i])
                if r >= 2:
                    t[i].append(a)
        out["batch"] = {m: {"round_us": spread(t[i]), "runs": [round(x, 1) for x in t[i]], **st[i]}
                        for i, m in ((0, "mode1"), (1, "mode3"))}
        last = Y if (runs + 2) % 2 == 0 else X  # the rows the last batch left free
        for e in pair:
            arrive(e, last)
            for _ in range(3):
                tick(e)
    return out


def updates_markdown(out):
    L = ["# dm_keep_keys modes 1 and 3: releases, arrivals and batches in k resources, then a writeback tick", "",
         "`python tools/keep_keys_ab.py --writer release,arrival,batch` on one MI355X: %d resources x 1,000 rows, "
         "FairShare, at its fixed point; two engines in one process, mode 1 (which treats these calls as the commit "
         "before DM_KEEP_UPDATES did) and mode 3, taking turns run by run; %d timed rounds each; host time of the "
         "call and the synchronous tick together, in us (median, min - max).  After the round: the parts whose tick "
         "ran with keys in use, and the valid keys." % (out["resources"], out["runs"]), "",
         "| writer | k | mode 1 | mode 3 | mode 3: parts with keys, keys | every mode-3 run below every mode-1 run |",
         "|---|---|---|---|---|---|"]
    for c in out["cases"]:
        for w in ("release", "arrival", "batch"):
            if w not in c:
                continue
            a, b = c[w]["mode1"]["round_us"], c[w]["mode3"]["round_us"]
            L.append("| %s | %d | %.1f (%.1f - %.1f) | %.1f (%.1f - %.1f) | %d, %d | %s |"
                     % (w, c["k"], a["median"], a["min"], a["max"], b["median"], b["min"], b["max"],
                        c[w]["mode3"]["fixed_parts"], c[w]["mode3"]["fixed_items"],
                        "yes" if b["max"] < a["min"] else "no"))
    return "\n".join(L) + "\n"


def refresh_calls(R, runs, rng):
    snap = all_fixed_store(R)
    N = len(snap["wants"])
    pair = engines(snap)
    try:
        bits = rng.random(N) < 0.1
        pad = (-N) % 64
        words = np.packbits(np.concatenate([bits, np.zeros(pad, bool)]), bitorder="little").view(np.uint64)
        vals = snap["wants"][bits].copy()
        times = ([], [])
        for r in range(runs + 2):
            for i in (1, 0):
                t0 = time.perf_counter()
                pair[i].update_wants_mask(words, vals)
                if r >= 2:
                    times[i].append(1e6 * (time.perf_counter() - t0))
        kept = pair[1].plan_info()["kept_refreshes"]
        items = pair[1].store_stats()["fixed_items"]
        assert kept == runs + 2 and items == R, (kept, items)  # every call ran the key-clearing build, no key cleared
        return {"rows": N, "values": int(bits.sum()), "plain_build_call_us": spread(times[0]),
                "key_clearing_build_call_us": spread(times[1]),
                "runs": {"plain": [round(t, 1) for t in times[0]], "key_clearing": [round(t, 1) for t in times[1]]}}
    finally:
        for e in pair:
            e.close()


def markdown(out):
    L = ["# dm_keep_keys on and off: a refresh of one row in each of k resources, then a writeback tick", "",
         "`python tools/keep_keys_ab.py` on one MI355X: %d resources x 1,000 rows, FairShare, at its fixed point; "
         "two engines in one process, taking turns run by run; %d timed rounds each; host time of the refresh call "
         "and the synchronous tick together, in us (median, min - max)." % (out["resources"], out["runs"]), "",
         "| k | values | mode off | mode on | on: keys after | every on run below every off run |", "|---|---|---|---|---|---|"]
    for c in out["cases"]:
        off, on = c["off"]["round_us"], c["on"]["round_us"]
        L.append("| %d | %s | %.1f (%.1f - %.1f) | %.1f (%.1f - %.1f) | %d | %s |"
                 % (c["k"], c["values"], off["median"], off["min"], off["max"], on["median"], on["min"], on["max"],
                    c["on"]["fixed_items"], "yes" if on["max"] < off["min"] else "no"))
    L += ["", "The tick's kernel classes (dm_kernel_times, us per round, three rounds under profiling):", "",
          "| k | values | mode | classes |", "|---|---|---|---|"]
    for c in out["cases"]:
        for m in ("off", "on"):
            L.append("| %d | %s | %s | %s |" % (c["k"], c["values"], m, ", ".join(
                "%s %.1f" % kv for kv in c[m]["tick_kernels_us"].items())))
    if out.get("refresh"):
        r = out["refresh"]
        p, q = r["plain_build_call_us"], r["key_clearing_build_call_us"]
        L += ["", "The masked refresh call alone, %d values over %d rows (stored values: no key cleared), host time of "
              "the call with its copies, us:" % (r["values"], r["rows"]), "",
              "| build | median | min - max |", "|---|---|---|",
              "| plain (`k_mask_apply`) | %.1f | %.1f - %.1f |" % (p["median"], p["min"], p["max"]),
              "| key-clearing (`k_mask_apply_keys`) | %.1f | %.1f - %.1f |" % (q["median"], q["min"], q["max"])]
    return "\n".join(L) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--resources", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--ks", default="100,1000,10000,100000")
    ap.add_argument("--refresh-resources", type=int, default=125_000, help="0: skip the refresh calls' part")
    ap.add_argument("--writer", default="refresh",
                    help="refresh (modes 0 and 1), or a list of release, arrival, batch (modes 1 and 3)")
    ap.add_argument("--out")
    ap.add_argument("--lib", default=None, help="another build of the library (tools/ab_libs/NAME.so)")
    a = ap.parse_args()
    LIB = a.lib
    rng = np.random.default_rng(3)
    t0 = time.perf_counter()
    snap = all_fixed_store(a.resources)
    out = {"resources": a.resources, "rows": int(len(snap["wants"])), "runs": a.runs, "cases": []}
    if a.writer != "refresh":
        pair = engines(snap, (1, 3))
        try:
            for k in (int(x) for x in a.ks.split(",") if x):
                k = min(k, a.resources)
                out["cases"].append({"k": k, **update_rounds(pair, snap, k, a.runs, rng, a.writer.split(","))})
        finally:
            for e in pair:
                e.close()
        out["seconds"] = round(time.perf_counter() - t0, 1)
        print(json.dumps(out))
        if a.out:
            with open(a.out, "w") as f:
                f.write(updates_markdown(out))
        sys.exit(0)
    pair = engines(snap)
    try:
        for k in (int(x) for x in a.ks.split(",") if x):  # (--ks "": the refresh calls' part alone)
            for changed in (True, False):
                c = ab_rounds(pair, snap, min(k, a.resources), changed, a.runs, rng)
                out["cases"].append({"k": min(k, a.resources), "values": "changed" if changed else "same", **c})
    finally:
        for e in pair:
            e.close()
    del snap
    if a.refresh_resources:
        out["refresh"] = refresh_calls(a.refresh_resources, a.runs, rng)
    out["seconds"] = round(time.perf_counter() - t0, 1)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(markdown(out))
