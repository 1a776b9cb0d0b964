"""The default line's step (C3 with the exchange on, one GPU) under a moving clock, for
several library builds in ONE process, interleaved (the style of tools/ab.py).

  python tools/round_now_ab.py [--dt 1.0] [--rounds 10] [--steps 50] [--warmup 5] LIB_A.so LIB_B.so[@VAR=value+...] ...

bench.py holds `now` still, so a store that the root's round skips because the word in memory
already holds its result (dm_hier_round.h) is skipped there for the rows' expiries too, which a
server never sees: its clock moves.  Here every build gets bench.py's pair (native="local",
pipelined, the leaf C3 and the root of one row per resource) and steps it with `now` advancing
--dt seconds per step (0: bench.py's standing clock).  Timed like bench.py's steps: the warm-up
steps and warm_steps() more, then per round K steps between syncs; per build the median, the
minimum and the maximum over the rounds, and with --values every round.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (one HIP runtime)

from ab import env  # noqa: E402
from bench import C3_R, make_workload, warm_steps  # noqa: E402
from doorman_amd import workloads as W  # noqa: E402
from doorman_amd.engine import Engine  # noqa: E402
from doorman_amd.hierarchy import HierarchicalTick, root_snapshot  # noqa: E402


class Pair:
    def __init__(self, spec, snap, dt_ns):
        path, _, envs = spec.partition("@")
        self.env = dict(kv.partition("=")[::2] for kv in filter(None, envs.split("+")))
        with env(self.env):
            self.leaf, self.root = Engine(0, os.path.abspath(path)), Engine(0, os.path.abspath(path))
        self.leaf.load(snap)
        self.root.load(root_snapshot(C3_R, 1, W.FAIR_SHARE, 1000.0, lease_length_s=20))
        self.ht = HierarchicalTick(torch, self.leaf, self.root, C3_R, 1, 0, None, shard_lo=np.array([0, C3_R]),
                                   pipelined=True, native="local")
        self.now, self.dt = W.NOW_NS, dt_ns
        self.us = []

    def steps(self, n):
        for _ in range(n):
            self.now += self.dt
            self.ht.tick(self.now, asynchronous=True)

    def timed(self, n):
        self.leaf.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.steps(n)
        self.leaf.join()
        self.leaf.sync()
        torch.cuda.synchronize()
        self.us.append((time.perf_counter() - t0) / n * 1e6)

    def close(self):
        self.ht.sync()
        self.ht.check()
        self.leaf.close()
        self.root.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+")
    ap.add_argument("--dt", type=float, default=1.0, help="seconds `now` advances per step (0: a standing clock)")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--values", action="store_true", help="every round's step, us")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    snap = make_workload("c3", 0, 1, "sharded")
    pairs = [Pair(p, snap, int(args.dt * W.NS)) for p in args.libs]
    warm = warm_steps(len(snap["wants"]))
    for p in pairs:
        with env(p.env):
            p.steps(args.warmup)
            p.leaf.sync()
            for i in range(warm):
                p.steps(1)
                if i % 8 == 7:
                    p.leaf.sync()
    for r in range(args.rounds):
        for p in (pairs if r % 2 == 0 else pairs[::-1]):  # the order turns round by round
            with env(p.env):
                p.steps(args.warmup)
                p.timed(args.steps)
    for spec, p in zip(args.libs, pairs):
        rides = p.leaf.plan_info().get("rounds_in_tick", 0)
        print(f"{os.path.basename(spec):40s} dt {args.dt:g} s: step med {statistics.median(p.us):7.2f} us  "
              f"min {min(p.us):7.2f}  max {max(p.us):7.2f}  ({len(p.us)} rounds of {args.steps} steps; "
              f"{rides} rounds rode in a leaf launch)")
        if args.values:
            print("    per round: " + " ".join(f"{v:.2f}" for v in p.us))
    for p in pairs:
        p.close()


if __name__ == "__main__":
    main()
