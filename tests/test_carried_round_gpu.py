"""The carried root round (dm_carry_rule.h, dm_hier_host.cpp, k_block_fused's ROOT build in
dm_tick_fused_root.hip): dm_hier_step keeps the root's round of step t - 1
and runs it inside step t's one fused leaf launch, or ahead of a tick that is not one launch,
and every other call on either context launches it first.

Nothing a caller can read may depend on it: engine pair A (DM_CARRY_ROUND=0: a launch of its
own behind every tick) and pair B (the default) hold identical bits after every burst of
asynchronous steps: leases, templates, the leaf and root stores, the root's sums, its verdict
and the published blocks.  dm_plan_info's "rounds_in_tick" says how many rounds rode.

The pairs are test_fused_tick_gpu.test_through_the_pipelined_exchange's: native="local", one
server, the root's kinds mixed over all four algorithms with NaN and set safe capacities and
lease lengths 20 and 60, some resources learning at the root and some at the leaf, `now` moving
by uneven amounts every step (so that a round decided with the wrong step's time shows in the
templates' parent expiries).  Both pairs run DM_FUSED=2 (fused wherever the rule allows,
whatever count was told), as that test's B does: the leaves' random wants leave many resources
oversubscribed, and only the carry may differ between A and B.

What a flush is seen by: the round's writes live in memory the library owns, so each flush point
is followed by library reads, which must equal A's (where the round ran long before); that B
really held a round at each point shows in rounds_in_tick, which grows over the sequence."""
import ctypes

import numpy as np
import pytest

from doorman_amd import _lib
from doorman_amd import workloads as W
import hier_model as M

pytestmark = pytest.mark.gpu

NOW = W.NOW_NS
BURSTS = (1, 2, 3, 5)
DT = (0.5, 1.25, 0.25, 2.75, 1.0)  # seconds between steps, in turn


def pairs(monkeypatch, alternate=False):
    """(leaf, root) A with DM_CARRY_ROUND=0 and B with the default; both DM_FUSED=2."""
    from doorman_amd.engine import Engine
    for k in ("DM_FIXED", "DM_SWEEP", "DM_STEADY", "DM_CYCLE", "DM_CYCLE_BYTES", "DM_CARRY_ROUND"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DM_FUSED", "2")
    if alternate:
        monkeypatch.setenv("DM_CYCLE_BYTES", "0")
    try:
        monkeypatch.setenv("DM_CARRY_ROUND", "0")
        a = (Engine(0), Engine(0))
        monkeypatch.delenv("DM_CARRY_ROUND")
        b = (Engine(0), Engine(0))
        return a, b
    finally:
        for k in ("DM_FUSED", "DM_CYCLE_BYTES", "DM_CARRY_ROUND"):
            monkeypatch.delenv(k, raising=False)


def root_config(R, rng):
    cfg = {"kind": rng.choice([W.FAIR_SHARE, W.PROPORTIONAL_SHARE, W.STATIC, W.NO_ALGORITHM], R).astype(np.int32),
           "capacity": rng.choice([100.0, 1000.0, 2500.5], R),
           "lease_length_s": rng.choice([20, 60], R).astype(np.int64),
           "refresh_interval_s": rng.choice([1, 5], R).astype(np.int64),
           "learning_end_ns": np.full(R, W.INT64_MIN, np.int64),
           "parent_expiry_ns": np.full(R, W.INT64_MAX, np.int64),
           "safe_capacity": np.where(rng.random(R) < 0.5, np.nan, rng.uniform(1, 9, R))}
    cfg["learning_end_ns"][rng.random(R) < 0.1] = NOW + 6 * W.NS  # learning until some step of the run
    return cfg


def leaf_snapshot(sizes, rng, subclients=1):
    sizes = np.asarray(sizes, np.int64)
    N = int(sizes.sum())
    full = W.make_snapshot(sizes, rng.uniform(0.2, 3.0, N) * 1000.0 / np.repeat(sizes, sizes), 0.0, subclients,
                           NOW + 600 * W.NS, W.FAIR_SHARE, 1000.0)
    learn = np.where(rng.random(len(sizes)) < 0.1, NOW + 4 * W.NS, W.INT64_MIN)
    return M.with_config(full, M.default_config(len(sizes), learn))


class Run:
    """One attached pair stepping through the pipelined exchange."""

    def __init__(self, leaf, root, snap, rcfg):
        import torch
        from doorman_amd.hierarchy import HierarchicalTick, root_snapshot
        torch.cuda.set_device(0)
        self.torch, self.leaf, self.root, self.rcfg = torch, leaf, root, rcfg
        self.R = R = len(snap["seg_off"]) - 1
        leaf.load(snap)
        root.load(M.with_config(root_snapshot(R, 1, W.FAIR_SHARE, 1.0), rcfg))
        self.ht = HierarchicalTick(torch, leaf, root, R, 1, 0, None, shard_lo=np.array([0, R]), pipelined=True,
                                   native="local")
        self.t = 0
        self.now = NOW

    def steps(self, n, before=None):
        for _ in range(n):
            if before is not None:
                before(self, self.t)
            self.now += int(DT[self.t % len(DT)] * W.NS)
            self.ht.tick(self.now, asynchronous=True)
            self.t += 1

    def observe(self):
        leases, cfg = self.leaf.leases(), self.leaf.config()
        out = {"gets": leases[0], "expiry": leases[1], "status": self.ht.status()}
        out.update({"template " + k: cfg[k] for k in W.CFG_FIELDS})
        for who, e in (("leaf", self.leaf), ("root", self.root)):
            out.update({f"{who} {k}": v for k, v in e.read_store().items()})
            out.update({f"{who} sums {k}": v for k, v in e.resources().items()})
        out["published"] = self.torch.stack(self.ht.totals).cpu().numpy()
        return out

    def rides(self):
        return self.leaf.plan_info()["rounds_in_tick"], self.root.plan_info()["rounds_in_tick"]


def same(a, b, label):
    assert a.keys() == b.keys(), label
    for k in a:
        if k == "rides":  # (rounds_in_tick so far: A's is 0 by design)
            continue
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), f"{label}: {k}"


def drive(monkeypatch, sizes, script, alternate=False, seed=21, subclients=1, snap_edit=None):
    """script(run) -> a list of (label, observation); run on A, then on B; -> (A's, B's, rides)."""
    (la, ra), (lb, rb) = pairs(monkeypatch, alternate)
    try:
        outs, rides = [], []
        for leaf, root in ((la, ra), (lb, rb)):
            rng = np.random.default_rng(seed)
            snap = leaf_snapshot(sizes, rng, subclients)
            if snap_edit is not None:
                snap_edit(snap)
            run = Run(leaf, root, snap, root_config(len(sizes), rng))
            outs.append(script(run))
            rides.append(run.rides())
        assert [x[0] for x in outs[0]] == [x[0] for x in outs[1]]
        for (label, a), (_, b) in zip(*outs):
            same(a, b, label)
        return outs[0], outs[1], rides
    finally:
        for e in (la, ra, lb, rb):
            e.close()


def halve_and_restore(halve_at, restore_at):
    def before(run, t):
        if t == halve_at:
            halved = {k: np.array(v) for k, v in run.rcfg.items()}
            halved["capacity"] *= 0.5
            run.root.load_config(halved)
        if t == restore_at:
            run.root.load_config(run.rcfg)
    return before


def bursts_script(run):
    seen = []
    before = halve_and_restore(22, 24)
    for i in range(12):  # 33 steps: bursts of 1, 2, 3, 5, three times over
        run.steps(BURSTS[i % 4], before)
        seen.append((f"after step {run.t}", run.observe()))
    return seen


# one bin each: 128 x 4, 128 x 8, 256 x 8, and bin 6 (512 x 8: it holds every row) with filler of its own bin
ONE_BIN = {"300x257": [257] * 300, "150x600": [600] * 150, "40x1100": [1100] * 40,
           "6x4096": [4096] * 6 + [2049, 3000, 2500, 4000, 3333]}


@pytest.mark.parametrize("column", ["inplace", "alternate"])
@pytest.mark.parametrize("shape", list(ONE_BIN))
def test_one_bin_leaves_carry_the_round(monkeypatch, shape, column):
    """Bursts of 1, 2, 3 and 5 asynchronous steps between reads; the root halves every capacity
    before step 22 (dm_config_load: a flush, and a new root configuration for the carried
    rounds after it) and restores it two steps later, inside a burst."""
    a, b, (ra, rb) = drive(monkeypatch, ONE_BIN[shape], bursts_script, alternate=column == "alternate")
    assert ra == (0, 0), ra
    assert rb[0] > 0 and rb[0] == rb[1], rb
    # the run is no fixed point: the halved capacities moved the root's grants (round 22, read after step 23)
    assert a[7][1]["root has"].tobytes() != a[8][1]["root has"].tobytes()


def test_a_leaf_with_several_bins_keeps_two_launches(monkeypatch):
    """test_through_the_pipelined_exchange's sizes, three bins: every tick is several launches,
    so every carried round runs ahead of its tick, where it ran before."""
    rng = np.random.default_rng(21)
    sizes = np.concatenate([rng.integers(257, 513, 140), rng.integers(513, 1100, 30), rng.integers(1025, 4097, 6)])
    _, _, (ra, rb) = drive(monkeypatch, sizes, bursts_script, alternate=True)
    assert ra == (0, 0) and rb == (0, 0), (ra, rb)


def test_listed_and_rest_items_inside_a_riding_launch(monkeypatch):
    """As test_fused_tick_gpu.test_rest_items_inside_a_fused_tick: under dm_keep_keys mode 3 a
    row is released in three resources and one of them refilled by an upsert, which leaves
    items with a stale hint, a mask bit or an arrival bit: rest items of the fused ticks that
    follow, beside the listed items the oversubscribed resources are.  The release and the
    upsert flush; the steps after them ride, and the root's round runs for those lanes too:
    the root rows of those resources move with the others, bit for bit as in A."""
    picked = (3, 130, 299)

    def script(run):
        seen = []
        run.leaf.keep_keys(3)
        run.steps(10)
        seen.append(("settled", run.observe()))
        off = run.leaf.seg_off
        rows = np.array([int(off[r]) + 70 for r in picked], np.int64)
        run.leaf.release(rows)
        r0 = run.rides()[0]
        run.steps(3)
        seen.append(("after the release", run.observe()))
        seen.append(("rides", {"n": np.array([run.rides()[0] - r0], np.int64)}))
        run.leaf.upsert(rows[:1], np.zeros(1), np.full(1, 0.125), np.ones(1, np.int64),
                        np.full(1, run.now + 200 * W.NS))
        run.steps(5)
        seen.append(("after the upsert", run.observe()))
        return seen

    # (the rides entry differs between A and B by design: compare the rest, then the counts)
    (la, ra), (lb, rb) = pairs(monkeypatch)
    try:
        outs, rides = [], []
        for leaf, root in ((la, ra), (lb, rb)):
            rng = np.random.default_rng(9)
            run = Run(leaf, root, leaf_snapshot([257] * 300, rng), root_config(300, rng))
            outs.append(script(run))
            rides.append(run.rides()[0])
        for (label, a), (_, b) in zip(*outs):
            if label != "rides":
                same(a, b, label)
        assert rides[0] == 0
        assert int(outs[1][2][1]["n"][0]) >= 1, outs[1][2]  # three steps after the flush: rounds rode in fused ticks
        before, after = outs[1][0][1], outs[1][1][1]
        for r in picked:  # one root row per resource: the round reached these lanes
            assert before["root wants"][r] != after["root wants"][r], r
    finally:
        for e in (la, ra, lb, rb):
            e.close()


def test_a_request_the_root_rejects(monkeypatch):
    """Which way the form admits it: not by the leaf's own tick.  A band with Count < 1 needs rows
    with zero subclients, and a resource holding them is never dense, so its part never runs a
    steady form and no tick of that leaf is one launch (tried: no round rides); a Count beyond
    2^31 is out of reach of a dense resource's 4,096 rows of at most 254 subclients.  So the
    test raises the flag itself, as a rejected server's block carries it: a torch write of
    record 0 of the block the last tick published, on the pair's stream, between the step that
    carries the round and the step it rides in (no library call, so nothing flushes), and once
    more for the round the final read flushes.

    B: step a (round a carried), step b (round a rides; b carried), flag block b, step c (round
    b rides, rejected; c carried), flag block c, read (round c launched, rejected).  As
    test_hierarchy_gpu.test_rejected_server_keeps_its_templates_and_root_rows expects, the
    status is the flag, the root's rows and sums are what round a left, and the templates the
    leaf takes next are round a's.  What round a left is read from A, which stops after it."""
    import torch
    SETTLE = 16

    def flag_last_block(run):
        blk = run.ht.totals[(run.t - 1) % 3]
        with torch.cuda.stream(run.ht.stream):
            blk.view(torch.int64)[0, 0] = int(_lib.DM_HIER_INVALID)

    (la, ra), (lb, rb) = pairs(monkeypatch)
    try:
        runs = []
        for leaf, root in ((la, ra), (lb, rb)):
            rng = np.random.default_rng(33)
            runs.append(Run(leaf, root, leaf_snapshot([257] * 300, rng), root_config(300, rng)))
        A, B = runs
        A.steps(SETTLE + 1)  # ... step a
        after_a = A.observe()
        A.steps(2)
        templates_a = A.leaf.config()  # tick a + 2 took round a's (lag 1: TemplateQueue::take)
        B.steps(SETTLE)
        B.leaf.sync()
        r0 = B.rides()[0]
        B.steps(2)
        flag_last_block(B)
        B.steps(1)
        flag_last_block(B)
        got = B.observe()
        rode = B.rides()[0] - r0
        print("rounds that rode in steps b and c:", rode)
        assert rode == 2, rode  # round a in step b, the rejected round b in step c
        assert got["status"][0] == _lib.DM_HIER_INVALID
        for k in got:
            if k.startswith("root "):
                assert np.asarray(got[k]).tobytes() == np.asarray(after_a[k]).tobytes(), k
        assert after_a["status"][0] == 0 and after_a["root has"].any()
        B.steps(2)  # tick c + 2 takes the rejected round c's templates: a copy of b's copy of round a's
        cfg = B.leaf.config()
        for k in W.CFG_FIELDS:
            assert np.asarray(cfg[k]).tobytes() == np.asarray(templates_a[k]).tobytes(), k
        assert A.rides() == (0, 0)
    finally:
        for e in (la, ra, lb, rb):
            e.close()


def test_every_flush_point_observes_the_round(monkeypatch):
    """A burst of asynchronous steps, then one call that must launch the carried round first,
    then reads; at the end the leaf is closed and the root read."""
    def script(run):
        torch, leaf, root, ht = run.torch, run.leaf, run.root, run.ht
        L = leaf._L
        seen = []
        counts = []

        def point(label, call):
            run.steps(3)
            counts.append(run.rides()[0])
            extra = call()
            obs = run.observe()
            if extra is not None:
                obs["extra"] = extra
            seen.append((label, obs))

        leaf.keep_keys(1)  # (the wants refresh below keeps the row epoch, and the ticks their form)
        run.steps(12)
        point("sync", leaf.sync)

        def join_then_torch():
            leaf.join()
            with torch.cuda.stream(ht.stream):  # a torch read on the pair's stream, behind the flushed round
                return torch.stack(ht.totals).clone().cpu().numpy()
        point("join", join_then_torch)
        point("root.read_store", lambda: root.read_store()["has"])
        point("leaf.config", lambda: leaf.config()["capacity"])
        point("status", ht.status)
        point("plain apportion", lambda: leaf.apportion(run.now, writeback=True, asynchronous=True))
        off = leaf.seg_off
        rows = np.array([int(off[5]) + 3, int(off[200]) + 9], np.int64)

        def refresh():  # (a refresh ends the tick's result: a step follows it before the reads)
            leaf.update_wants(rows, np.array([0.25, 0.75]))
            run.steps(1)
        point("wants refresh", refresh)

        def foreign():
            xs = torch.cuda.Stream()
            leaf.stream_wait(xs.cuda_stream)
            with torch.cuda.stream(xs):
                has = root.read_store_device(columns=("has",))["has"]
                shot = has.clone()
            xs.synchronize()
            return shot.cpu().numpy()
        point("stream_wait", foreign)

        def unpipe():
            _lib.check(L.dm_hier_pipeline(leaf._ctx, 0), leaf._ctx, L)  # takes the newest staged templates now
            cfg = leaf.config()
            _lib.check(L.dm_hier_pipeline(leaf._ctx, 1), leaf._ctx, L)
            return np.concatenate([np.asarray(cfg[k], np.float64) for k in ("capacity", "lease_length_s")])
        point("dm_hier_pipeline(0)", unpipe)

        run.steps(3)
        counts.append(run.rides()[0])
        leaf.close()  # the round it leaves is launched; the root store holds it
        fin = {f"root {k}": v for k, v in root.read_store().items()}
        fin.update({f"root sums {k}": v for k, v in root.resources().items()})
        seen.append(("leaf closed", fin))
        seen.append(("counts", {"n": np.array(counts, np.int64)}))
        return seen

    (la, ra), (lb, rb) = pairs(monkeypatch)
    try:
        outs = []
        for leaf, root in ((la, ra), (lb, rb)):
            rng = np.random.default_rng(4)
            run = Run(leaf, root, leaf_snapshot([257] * 300, rng), root_config(300, rng))
            outs.append(script(run))
        for (label, a), (_, b) in zip(*outs):
            if label != "counts":
                same(a, b, label)
        ca, cb = outs[0][-1][1]["n"], outs[1][-1][1]["n"]
        assert not ca.any(), ca
        print("rounds_in_tick before each flush point:", cb)
        assert (np.diff(cb) >= 1).all() and cb[0] > 0, cb  # every burst behind a flush held rounds that rode
    finally:
        for e in (la, ra, lb, rb):
            e.close()


def test_plan_info_names_the_counter():
    from doorman_amd import engine
    assert engine._PLAN_NAMES[29] == "rounds_in_tick"
