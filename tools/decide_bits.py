"""dm_decide of two library builds, bit for bit, in ONE process (as tools/chain_bits.py).

  python tools/decide_bits.py PARENT.so [--new LIB.so]

For a change that should leave dm_decide's results untouched but moves its host side or its kernels'
arguments: the oracle tolerance of tests/test_server_gpu.py cannot see a reordered sum or a request decided
from a neighbour's area, this can.  It restates that file's rounds -- the stores and requests of
test_decide_matches_sequential_oracle_decides (4 seeds) and test_decide_fast_path_matches_sequential_oracle
(3 seeds), and the three rounds of test_decide_rounds_grow_shrink_and_reuse_their_buffers on one engine --
and decides them on the parent's library and the tree's under DM_DECIDE_FAST = 0 and 1 (read when an engine
is created).  After every round its gets and expiries and read_store() of the two engines are compared byte
for byte: the one-workgroup replay is sequential and the fast path fixes the order of every sum, so they
must be equal.  One line per case; exit status 1 on any difference.
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
from test_server_gpu import NOW, OWNER_KINDS, OWNER_S0, OWNER_SIZES, _fast_round_snapshot, _owner_rounds  # noqa: E402


def sequential_case(seed):
    """test_decide_matches_sequential_oracle_decides' store and round."""
    rng = np.random.default_rng(900 + seed)
    snap = W.random_snapshot(rng, 30, 60, hetero=seed % 2 == 1, edge=seed == 3)
    N = len(snap["wants"])
    free = rng.random(N) < 0.15
    for k, v in (("wants", 0.0), ("has", 0.0), ("subclients", 0), ("expiry_ns", W.RELEASED)):
        snap[k][free] = v
    W.add_store_sums(snap)
    rows = np.flatnonzero(rng.random(N) < 0.4)
    rows = np.concatenate([rows, rng.choice(rows, max(1, len(rows) // 10))])
    rng.shuffle(rows)
    n = len(rows)
    cap_row = np.repeat(snap["capacity"], np.diff(snap["seg_off"]))
    wants = np.where(rng.random(n) < 0.5, snap["wants"][rows], rng.uniform(0, 2, n) * cap_row[rows] / 10)
    sub = np.where(rng.random(n) < 0.8, np.maximum(snap["subclients"][rows], 1), rng.integers(1, 5, n))
    has = rng.uniform(0, 1, n) * cap_row[rows] / 10
    return snap, [(rows, has, wants, sub)]


def fast_case(seed):
    """test_decide_fast_path_matches_sequential_oracle's store and round (decided twice there too)."""
    rng = np.random.default_rng(31 + seed)
    sizes = np.array([3000, 700, 1500, 90, 40, 2600], dtype=np.int64)
    kinds = [W.FAIR_SHARE, W.FAIR_SHARE, W.PROPORTIONAL_SHARE, W.FAIR_SHARE, W.PROPORTIONAL_SHARE, W.FAIR_SHARE]
    s0 = [1, 3, 1, 3, 1, 1]
    snap = _fast_round_snapshot(rng, sizes, kinds, s0)
    so = snap["seg_off"]
    rel = so[5] + rng.choice(sizes[5], sizes[5] // 10, replace=False)
    snap["expiry_ns"][rel] = W.RELEASED
    snap["has"][rel] = 0.0
    snap["wants"][rel] = 0.0
    snap["subclients"][rel] = 0
    W.add_store_sums(snap)
    rows, wants, sub = [], [], []
    for r, n in enumerate(sizes):
        if r % 2 == 0:
            rr = so[r] + rng.permutation(n)
            K = n
        else:
            K = int(n * rng.choice([1.0, 1.5, 2.5]))
            rr = so[r] + rng.integers(0, n, K)
        cw = snap["wants"][rr]
        fresh = rng.uniform(0.0, 3.0, K) * snap["capacity"][r] / n * s0[r]
        w = np.where(rng.random(K) < 0.4, cw, fresh)
        t = rng.random(K) < 0.1
        w[t] = np.round(w[t])
        rows.append(rr)
        wants.append(w)
        sub.append(np.full(K, s0[r], np.int64))
    rows, wants, sub = np.concatenate(rows), np.concatenate(wants), np.concatenate(sub)
    odd = np.flatnonzero((rows >= so[1]) & (rows < so[2]))[5]
    sub[odd] = 2
    order = rng.permutation(len(rows))
    rows, wants, sub = rows[order], wants[order], sub[order]
    has = rng.uniform(0, 1, len(rows))
    return snap, [(rows, has, wants, sub)] * 2


def owner_case():
    rng = np.random.default_rng(77)
    snap = _fast_round_snapshot(rng, OWNER_SIZES, OWNER_KINDS, OWNER_S0)
    return snap, _owner_rounds(rng, snap)


def run(engines, snap, rounds):
    """The names in which the engines differ after some round, with the round's number."""
    for e in engines:
        e.load(snap)
    bad = []
    for i, r in enumerate(rounds):
        outs = []
        for e in engines:
            gets, exp = e.decide(NOW, *r)
            state = {"gets": gets, "expiry": exp}
            state.update(("store." + k, v) for k, v in e.read_store().items())
            outs.append({k: np.ascontiguousarray(v).tobytes() for k, v in state.items()})
        bad += ["round %d: %s" % (i, k) for k in outs[0] if outs[0][k] != outs[1][k]]
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent", help="the parent commit's libdoorman_hip.so")
    ap.add_argument("--new", default=os.path.join(ROOT, "doorman_amd", "libdoorman_hip.so"))
    a = ap.parse_args()
    cases = [("sequential seed %d" % s, lambda s=s: sequential_case(s)) for s in range(4)]
    cases += [("fast path seed %d" % s, lambda s=s: fast_case(s)) for s in range(3)]
    cases.append(("growing rounds", owner_case))
    failed = 0
    for fast in ("0", "1"):
        os.environ["DM_DECIDE_FAST"] = fast
        engines = [Engine(0, os.path.abspath(lib)) for lib in (a.parent, a.new)]
        for name, make in cases:
            snap, rounds = make()
            bad = run(engines, snap, rounds)
            failed += bool(bad)
            print("DM_DECIDE_FAST=%s %-18s %d rounds, %6d requests: %s" % (
                fast, name, len(rounds), sum(len(r[0]) for r in rounds),
                "DIFFERS in " + "; ".join(bad[:6]) if bad else "byte-equal"), flush=True)
        for e in engines:
            e.close()
    print("%s" % ("%d cases differ" % failed if failed else "every case byte-equal"))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
