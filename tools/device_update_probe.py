"""A round of store updates from device memory against the host batch it replaces, on one
store in one process, the routes interleaved run by run.

A C4-shaped store of 1000-row resources (16M rows by default).  A round: 10 % of the rows
refresh their wants, 1 % leave, 1 % arrive (narrow arrivals: int32 subclients, no has, no
expiry column), as bench.py's C4 round.  Host wall time around each synchronous call, one
warm-up of each route, then --runs runs:
  (a) host round      Engine.apply from page-locked arrays (dm_host_alloc): the columns cross
                      PCIe on the copy stream and are staged before a kernel sees them
  (b) device round    Engine.apply_device of the same columns as torch tensors: the same
                      kernels on the caller's columns, nothing copied
  (c) host refresh    Engine.update_wants_mask of the round's refresh alone, page-locked
  (d) dense refresh   Engine.refresh_wants_device of the same refresh from a whole new wants
                      column (16 B a row read, 8 B more per differing row, 8 B per changed row
                      written): no mask and no packed values were ever built
Every call really changes its rows: the refresh alternates between two value sets, and the
departures and arrivals swap two row sets from call to call (the rows that left arrive next).
The bytes each route moves are computed from the shapes.
usage: python tools/device_update_probe.py [--rows 16000000] [--out profiles/device_update_probe.json]
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
    rng = np.random.default_rng(17)
    perm = rng.permutation(N)
    n_ref, n_swap = N // 10, N // 100
    S = np.sort(perm[:n_ref])                              # the rows that refresh
    P, Q = perm[n_ref:n_ref + n_swap], perm[n_ref + n_swap:n_ref + 2 * n_swap]  # live / free at the start
    for k, v in (("wants", 0.0), ("has", 0.0), ("subclients", 0), ("expiry_ns", W.RELEASED)):
        snap[k][Q] = v
    W.add_store_sums(snap)
    eng = Engine(0)
    eng.load(snap)
    now = W.NOW_NS + W.NS
    dev = torch.device("cuda", 0)

    def pinned(arr):
        out = eng.host_empty(len(arr), arr.dtype)
        out[:] = arr
        return out

    vals = [rng.uniform(0.1, 50.0, n_ref), rng.uniform(0.1, 50.0, n_ref)]
    w_arr = rng.uniform(0.1, 50.0, N)  # an arrival's wants, by row: the same at every arrival
    h_mask = pinned(W.rows_to_mask(S, N))
    h_vals = [pinned(v) for v in vals]
    h_rows = [pinned(P), pinned(Q)]
    h_arr_w = [pinned(w_arr[P]), pinned(w_arr[Q])]
    h_sub = pinned(np.ones(n_swap, np.int32))
    d_mask = torch.from_numpy(W.rows_to_mask(S, N).view(np.int64)).to(dev)
    d_vals = [torch.from_numpy(v).to(dev) for v in vals]
    d_rows = [torch.from_numpy(P).to(dev), torch.from_numpy(Q).to(dev)]
    d_arr_w = [torch.from_numpy(w_arr[P]).to(dev), torch.from_numpy(w_arr[Q]).to(dev)]
    d_sub = torch.ones(n_swap, dtype=torch.int32, device=dev)
    # the dense route's columns: the stored wants, the swapping rows at their arrival value (a
    # live one then equals what is stored, a released one is ignored), the refresh at either set
    cols = []
    for v in vals:
        c = snap["wants"].copy()
        c[P], c[Q] = w_arr[P], w_arr[Q]
        c[S] = v
        cols.append(torch.from_numpy(c).to(dev))
    torch.cuda.synchronize()
    # P's rows keep the wants they were loaded with until they first arrive: make them arrivals' now
    eng.update_wants(P, w_arr[P])

    state = {"ref": 0, "swap": 0, "dense_changed": []}

    def host_round():
        r, s = state["ref"], state["swap"]
        eng.apply(h_mask, h_vals[r], release_rows=h_rows[s], upsert=(h_rows[s ^ 1], None, h_arr_w[s ^ 1], h_sub, None),
                  now_ns=now)
        state["ref"], state["swap"] = r ^ 1, s ^ 1

    def device_round():
        r, s = state["ref"], state["swap"]
        eng.apply_device(d_mask, d_vals[r], release_rows=d_rows[s],
                         upsert=(d_rows[s ^ 1], None, d_arr_w[s ^ 1], d_sub, None), now_ns=now)
        state["ref"], state["swap"] = r ^ 1, s ^ 1

    def host_refresh():
        r = state["ref"]
        eng.update_wants_mask(h_mask, h_vals[r])
        state["ref"] = r ^ 1

    def dense_refresh():
        r = state["ref"]
        state["dense_changed"].append(eng.refresh_wants_device(cols[r]))
        state["ref"] = r ^ 1

    routes = {"host_round_pinned": host_round, "device_round": device_round, "host_refresh_pinned": host_refresh,
              "dense_refresh_device": dense_refresh}
    t = {k: [] for k in routes}
    for i in range(a.runs + 1):
        for k, fn in routes.items():
            dt = wall(fn)
            if i >= 1:  # warm-up: the first calls allocate
                t[k].append(dt)

    # the last refresh is in the store, whichever route made it
    got = eng.read_store()["wants"]
    applied = bool(np.array_equal(got[S].view(np.int64), vals[state["ref"] ^ 1].view(np.int64)))

    # bytes, from the shapes.  Host round over PCIe: the mask, 8 B per refreshed value, 8 B per
    # departure, 8 + 8 + 4 B per arrival.  Device round: the same columns read from HBM, the
    # count and apply passes' scratch (12 B per mask word), per refreshed row the stored wants
    # and subclients read and the wants written (20 B), per departure and arrival the row's
    # columns.  Dense refresh: 16 B per row read, 4 B more per differing row, 8 B per changed
    # row written.
    nwords = (N + 63) // 64
    host_pcie = 8 * nwords + 8 * n_ref + 8 * n_swap + 20 * n_swap
    dev_hbm = (16 + 12) * nwords + (8 + 20) * n_ref + (8 + 28 + 8) * n_swap + (20 + 28 + 8) * n_swap
    dense_hbm = 16 * N + 12 * n_ref
    med = {k: statistics.median(v) for k, v in t.items()}

    def below(devk, hostk):
        return max(t[devk]) < min(t[hostk])

    out = {
        "rows": N, "resources": R, "rows_per_resource": a.clients, "runs": a.runs,
        "refreshed_rows": int(n_ref), "departures": int(n_swap), "arrivals": int(n_swap),
        **{k: stats(v) for k, v in t.items()},
        "host_round_pcie_bytes": host_pcie,
        "device_round_pcie_bytes": 12,
        "device_round_hbm_bytes": dev_hbm,
        "dense_refresh_pcie_bytes": 12,
        "dense_refresh_hbm_bytes": dense_hbm,
        "dense_refresh_GBps": round(dense_hbm / (med["dense_refresh_device"] * 1e-3) / 1e9, 1),
        "dense_refresh_fraction_of_hbm_peak": round(dense_hbm / (med["dense_refresh_device"] * 1e-3) / HBM_PEAK, 4),
        "dense_refresh_rows_changed": sorted(set(state["dense_changed"])),
        "last_refresh_is_in_the_store": applied,
        "every_device_round_below_every_host_round": below("device_round", "host_round_pinned"),
        "every_dense_refresh_below_every_host_round": below("dense_refresh_device", "host_round_pinned"),
        "every_dense_refresh_below_every_host_refresh": below("dense_refresh_device", "host_refresh_pinned"),
        "speedup_round": round(med["host_round_pinned"] / med["device_round"], 1),
        "speedup_refresh_dense_vs_host_round": round(med["host_round_pinned"] / med["dense_refresh_device"], 1),
        "speedup_refresh_dense_vs_host_refresh": round(med["host_refresh_pinned"] / med["dense_refresh_device"], 1),
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
