"""The large-resource chain of two library builds, bit for bit, in ONE process (as tools/ab.py).

  python tools/chain_bits.py PARENT.so [--new LIB.so]

For a change that should leave the chain's results untouched but moves its kernels' text: the oracle
tolerances of tests/test_large_gpu.py cannot see a reordered sum, this can.  It builds that file's
stores -- large_sizes in its uniform, hetero, edge, recompute, no_expiry and learning variants (two seeds)
and the speculative test's eleven-resource store with its release / wants / capacity / lapse / peek plan --
and runs them on the parent's library and the tree's under DM_SPEC_CHAIN = 0, 1 and DM_REDO_LIGHT = 0, 1, 2
(both read when an engine is created).  After every tick leases(), read_store() and resources() of the two
engines are compared byte for byte.  One line per case; exit status 1 on any difference.

The store-update kernels add a batch's deltas to a resource's running sums with floating-point atomics
(dm_update_util.h), so after one update_wants or release call over many rows two engines of ONE library may
already differ in resources.sum_wants / sum_has by a rounding (seen in half of the runs).  The plan's
releases and wants refresh are therefore applied one row a call, in the same order on every engine: one add
a call, nothing left to order.  A third engine, the parent's library once more, is the control: a name that
still differs between the parent's two engines at some tick of a case is reported as unstable there and
does not count; every other difference does.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (one HIP runtime)

from doorman_amd import workloads as W  # noqa: E402
from doorman_amd.engine import Engine  # noqa: E402
from parity_util import snapshot_with_sizes  # noqa: E402
from test_large_gpu import large_sizes  # noqa: E402

NOW = W.NOW_NS
VARIANTS = ["uniform", "hetero", "edge", "recompute", "no_expiry", "learning"]


def state(e):
    """Everything a tick leaves that a caller can read, as bytes per name."""
    gets, exp = e.leases()
    out = {"leases.gets": gets, "leases.expiry": exp}
    out.update(("store." + k, v) for k, v in e.read_store().items())
    out.update(("resources." + k, v) for k, v in e.resources(safe=False).items())
    return {k: np.ascontiguousarray(v).tobytes() for k, v in out.items()}


class Diffs:
    """Per tick, the names in which the new engine and the control differ from the parent's (engines: parent, new, control)."""

    def __init__(self):
        self.ticks, self.new, self.control = 0, [], set()

    def tick(self, engines, label):
        a, b, c = (state(e) for e in engines)
        self.ticks += 1
        self.new += [(label, k) for k in a if a[k] != b[k]]
        self.control |= {k for k in a if a[k] != c[k]}

    def report(self):
        bad = ["%s: %s" % lk for lk in self.new if lk[1] not in self.control]
        text = "DIFFERS in " + "; ".join(bad[:6]) if bad else "byte-equal"
        if self.control:
            text += " (unstable between two engines of the parent: %s)" % ", ".join(sorted(self.control))
        return bool(bad), "%2d ticks: %s" % (self.ticks, text)


def variant_case(engines, seed, variant):
    """test_large_variants_against_oracle's store: its tick, then two writeback ticks on the alternate column
    (the second one speculates when the engine does)."""
    rng = np.random.default_rng(9000 + seed)
    snap = snapshot_with_sizes(rng, large_sizes(rng), hetero=variant == "hetero", edge=variant == "edge",
                               expired_frac=0.0 if variant == "no_expiry" else 0.05,
                               learning_frac=0.5 if variant == "learning" else 0.1)
    rec = variant == "recompute"
    if rec:
        for k in ("agg_count", "agg_sum_has", "agg_sum_wants"):
            snap.pop(k)
    d = Diffs()
    for e in engines:
        e.load(snap)
    for i, kw in enumerate([dict(recompute=rec), dict(writeback=True, wb_columns="alternate", recompute=rec),
                            dict(writeback=True, wb_columns="alternate"), dict(writeback=True)]):
        for e in engines:
            e.apportion(NOW + i * W.NS, **kw)
        d.tick(engines, "tick %d" % i)
    return d


def plan_case(engines):
    """test_speculative_chain_against_the_chain_and_the_oracle's store and plan."""
    rng = np.random.default_rng(8080)
    sizes = np.asarray([4097, 5000, 6000, 8192, 9000, 20000, 65537, 150000, 300, 17, 5], dtype=np.int64)
    snap = snapshot_with_sizes(rng, sizes, kinds=(0, 1, 2, 3), expired_frac=0.01, learning_frac=0.0,
                               parent_expired_frac=0.0)
    snap["kind"][:8] = [3, 3, 2, 3, 2, 3, 1, 3]
    snap["learning_end_ns"][:8] = W.INT64_MIN
    snap["learning_end_ns"][2] = NOW + 3600 * W.NS
    snap["lease_length_s"][:8] = [40, 600, 600, 600, 35, 600, 600, 600]
    so = np.asarray(snap["seg_off"])
    N = len(snap["wants"])
    for e in engines:
        e.load(snap)
    plan = ["same", "same", "same", "same", "release", "same", "same", "wants", "same", "same", "capacity",
            "same", "same", "lapse", "same", "same", "peek", "same", "same"]
    now, capacity, d = NOW, snap["capacity"].copy(), Diffs()
    for i, step in enumerate(plan):
        now += (50 if step == "lapse" else 1) * W.NS
        if step == "release":
            rows = rng.choice(N, 300, replace=False).astype(np.int64)
            for e in engines:
                for r in rows:
                    e.release(np.asarray([r], dtype=np.int64))
        elif step == "wants":
            rows = np.concatenate([np.arange(so[1], so[1] + 700), np.arange(so[4], so[4] + 2000)]).astype(np.int64)
            w = rng.uniform(0.0, 3.0, len(rows)) * np.repeat(snap["capacity"], np.diff(so))[rows] / 1000.0
            for e in engines:
                for k in range(len(rows)):
                    e.update_wants(rows[k:k + 1], w[k:k + 1])
        elif step == "capacity":
            capacity[5] *= 0.5
            c2 = dict(snap)
            c2["capacity"] = capacity
            for e in engines:
                e.load_config(c2)
        for e in engines:
            e.apportion(now, writeback=step != "peek", wb_columns="alternate")
        d.tick(engines, "tick %d (%s)" % (i, step))
    return d


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent", help="the parent commit's libdoorman_hip.so")
    ap.add_argument("--new", default=os.path.join(ROOT, "doorman_amd", "libdoorman_hip.so"))
    a = ap.parse_args()
    failed = 0
    for spec in ("0", "1"):
        for light in ("0", "1", "2"):
            os.environ.update(DM_SPEC_CHAIN=spec, DM_REDO_LIGHT=light)
            engines = [Engine(0, os.path.abspath(lib)) for lib in (a.parent, a.new, a.parent)]  # parent, new, control
            cases = [("%s seed %d" % (v, s), lambda s=s, v=v: variant_case(engines, s, v)) for v in VARIANTS for s in (0, 1)]
            cases.append(("speculative plan", lambda: plan_case(engines)))
            for name, run in cases:
                bad, text = run().report()
                failed += bad
                print("DM_SPEC_CHAIN=%s DM_REDO_LIGHT=%s %-20s %s" % (spec, light, name, text), flush=True)
            for e in engines:
                e.close()
    print("%s" % ("%d cases differ" % failed if failed else "every case byte-equal"))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
