"""Host time of a server-shaped round two ways, interleaved in ONE process: the pair dm_server_tick makes
(dm_decide, the host's gather of each row's last request, dm_store_upsert,
dm_read_resources for the counts) against the one call.

  python tools/decide_assign_ab.py [--runs 10] [--out profiles/decide_assign_ab.md]

Two stores: 1,000 resources of 1,000 rows with mixed kinds, rounds of K = 1,000, 10,000 and 100,000 requests
on distinct rows spread over the resources; and one 100,000-row FairShare resource with all K on it (DESIGN
7.1's case).  Two engines are loaded with the same store, one takes the pair and one the call; after three
warm-up rounds each (allocations, code objects) the runs alternate between them and the one that goes first
rotates.  A run is one round, timed with the host clock around calls that each end in a wait for the context
stream; every round refreshes the same rows with the same wants, so the two stores stay in step up to the last
bits of their running sums (the upsert's atomics add in an order that varies), which is why the two
ways' first rounds are compared by a relative difference and not by bytes.  Per way:
median, min and max over the runs, and for the pair its parts.  The floors -- a dm_store_upsert of one row and a
dm_read_resources of one resource, timed the same way -- estimate what the pair's two extra calls cost before a
byte of their columns moves (launches, the flags' copy, the wait); what the two calls take beyond their floors,
and the host's gather, is the share of the copies and of the kernels' own time.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (one HIP runtime)

from doorman_amd import workloads as W  # noqa: E402
from doorman_amd.engine import Engine, _ptr  # noqa: E402

NOW = W.NOW_NS


def spread_store():
    snap = W.uniform(1000, 1000, kind="mixed", seed=7)
    r = np.arange(1000)
    snap["kind"] = np.where(r % 4 == 2, W.STATIC, np.where(r % 8 == 7, W.NO_ALGORITHM, snap["kind"])).astype(np.int32)
    return W.add_store_sums(snap)


def one_store():
    return W.add_store_sums(W.uniform(1, 100_000, kind=W.FAIR_SHARE, seed=5, capacity=12345.678))


def requests(snap, K, seed):
    rng = np.random.default_rng(seed)
    N = len(snap["wants"])
    rows = rng.choice(N, K, replace=False).astype(np.int64)
    cap_row = np.repeat(snap["capacity"], np.diff(snap["seg_off"]))
    n_row = np.repeat(np.diff(snap["seg_off"]), np.diff(snap["seg_off"]))
    wants = rng.uniform(0.0, 3.0, K) * cap_row[rows] / n_row[rows]
    return rows, np.zeros(K), wants, np.ones(K, np.int64)


class Pair:
    """dm_decide + gather + dm_store_upsert + dm_read_resources, with the parts' times of the last run."""

    def __init__(self, e, q, R):
        self.e, self.L, self.q = e, e._L, q
        n = len(q[0])
        self.gets, self.exp = np.empty(n), np.empty(n, np.int64)
        rows = q[0]
        res = np.searchsorted(e.seg_off, rows, side="right") - 1
        self.rlo, self.rn = int(res.min()), int(res.max() - res.min() + 1)
        self.count = np.empty(self.rn, np.int64)
        last = {}
        for k, row in enumerate(rows):
            last[int(row)] = k
        self.last = np.array(sorted(last.values()), np.int64)  # (the server keeps this map in either form)
        self.parts = None

    def run(self):
        L, c, q = self.L, self.e._ctx, self.q
        n = len(q[0])
        t0 = time.perf_counter()
        assert L.dm_decide(c, NOW, n, *[_ptr(x) for x in q], _ptr(self.gets), _ptr(self.exp)) == 0
        t1 = time.perf_counter()
        k = self.last
        u = [np.ascontiguousarray(x[k]) for x in (q[0], self.gets, q[2], q[3], self.exp)]
        t2 = time.perf_counter()
        assert L.dm_store_upsert(c, len(k), *[_ptr(x) for x in u]) == 0
        t3 = time.perf_counter()
        assert L.dm_read_resources(c, self.rlo, self.rn, _ptr(self.count), None, None, None) == 0
        t4 = time.perf_counter()
        self.parts = [(b - a) * 1e6 for a, b in ((t0, t1), (t1, t2), (t2, t3), (t3, t4))]
        return (t4 - t0) * 1e6

    def floors(self):
        """A one-row upsert (the row's own values again) and a one-resource read."""
        L, c, q = self.L, self.e._ctx, self.q
        k = self.last[:1]
        u = [np.ascontiguousarray(x[k]) for x in (q[0], self.gets, q[2], q[3], self.exp)]
        t0 = time.perf_counter()
        assert L.dm_store_upsert(c, 1, *[_ptr(x) for x in u]) == 0
        t1 = time.perf_counter()
        assert L.dm_read_resources(c, self.rlo, 1, _ptr(self.count), None, None, None) == 0
        t2 = time.perf_counter()
        return (t1 - t0) * 1e6, (t2 - t1) * 1e6


class OneCall:
    def __init__(self, e, q):
        self.e, self.L, self.q = e, e._L, q
        n = len(q[0])
        self.gets, self.exp, self.safe = np.empty(n), np.empty(n, np.int64), np.empty(n)

    def run(self):
        q = self.q
        t0 = time.perf_counter()
        assert self.L.dm_decide_assign(self.e._ctx, NOW, len(q[0]), *[_ptr(x) for x in q], _ptr(self.gets),
                                       _ptr(self.exp), _ptr(self.safe)) == 0
        return (time.perf_counter() - t0) * 1e6


def med(v):
    return "%.0f (%.0f - %.0f)" % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = ["# A server-shaped round: dm_decide + dm_store_upsert + dm_read_resources against dm_decide_assign", "",
             "`tools/decide_assign_ab.py`: one process, two engines on one store, %d interleaved runs of each way after "
             "three warm-up rounds, the way that goes first rotating; host time in us, median (min - max)." % a.runs, "",
             "| store | K | pair | one call | one call / pair | pair: decide | gather | upsert | read_resources | "
             "floors: upsert of 1 row, read of 1 resource | results |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    notes = []
    for name, make in (("1,000 x 1,000, mixed kinds", spread_store), ("one 100k-row FairShare resource", one_store)):
        snap = make()
        with Engine(0) as ep, Engine(0) as eo:
            ep.load(snap)
            eo.load(snap)
            for K in (1000, 10_000, 100_000):
                q = requests(snap, K, K)
                pair, one = Pair(ep, q, len(snap["kind"])), OneCall(eo, q)
                cap_row = np.repeat(snap["capacity"], np.diff(snap["seg_off"]))[q[0]]
                for w in range(3):
                    pair.run()
                    one.run()
                    if w == 0:  # the first round: what the two ways decided and stored, against each other
                        dg = float(np.max(np.abs(pair.gets - one.gets) / np.maximum(np.abs(pair.gets), cap_row)))
                        sp, so = ep.read_store(), eo.read_store()
                        dh = float(np.max(np.abs(sp["has"][q[0]] - so["has"][q[0]]) / cap_row))
                        same = (pair.exp.tobytes() == one.exp.tobytes() and
                                all(sp[k].tobytes() == so[k].tobytes() for k in ("wants", "subclients", "expiry_ns")))
                        agree = "gets within %.1e, stored has within %.1e of the capacity; %s" % (
                            dg, dh, "expiries, wants and subclients byte-equal" if same else "expiries or rows DIFFER")
                tp, to, parts, fl = [], [], [], []
                for i in range(a.runs):
                    for w in ((0, 1) if i % 2 == 0 else (1, 0)):
                        ep.sync()
                        eo.sync()
                        if w == 0:
                            tp.append(pair.run())
                            parts.append(pair.parts)
                        else:
                            to.append(one.run())
                    fl.append(pair.floors())
                cols = list(zip(*parts))
                fu, fr = [f[0] for f in fl], [f[1] for f in fl]
                mp, mo = statistics.median(tp), statistics.median(to)
                lines.append("| %s | %d | %s | %s | %.2f | %s | %s | %s | %s | %s, %s | %s |" % (
                    name, K, med(tp), med(to), mo / mp, med(cols[0]), med(cols[1]), med(cols[2]), med(cols[3]), med(fu),
                    med(fr), agree))
                waits = statistics.median(fu) + statistics.median(fr)
                rest = statistics.median(cols[1]) + statistics.median(cols[2]) + statistics.median(cols[3]) - waits
                notes.append("- %s, K = %d: of the pair's %.0f us, the two extra calls' floors (launches, flags, wait) are "
                             "%.0f us (%.0f %%); the gather, the 40 B per row and the counts over PCIe and the kernels' own "
                             "time are %.0f us (%.0f %%); the one call saves %.0f us." % (
                                 name, K, mp, waits, 100 * waits / mp, rest, 100 * rest / mp, mp - mo))
    lines += ["", "Shares of the pair's time (medians; the floors are estimates of the two extra waits, see the tool's "
              "docstring):", ""] + notes
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
