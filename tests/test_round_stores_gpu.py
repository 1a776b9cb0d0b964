"""The root's round stores a word only where its bits differ from what the lane loaded there
(dm_hier_round.h hier_round_decide, both forms: k_hier_tick and k_block_fused's ROOT build;
DESIGN.md section 6).  DM_ROUND_STORES=0 stores every word, as the round did before.

Nothing a caller can read may depend on it: engine pair A (DM_ROUND_STORES=0) and pair B (the
default), both DM_FUSED=2 as test_carried_round_gpu's pairs are, hold identical bits after every
burst: leases, templates, the leaf and root stores, the root's sums, its verdict and the
published blocks (test_carried_round_gpu.same).  Whether a store was in fact skipped does not
show in results; WRITE_SIZE shows it (profiles/round_stores_ab.md).

Shapes: [257] * 300 (three workgroups of 128 lanes in the fused launch, the last with 44) and
[600] * 150 (the 128 x 8 bin)."""
import numpy as np
import pytest

from doorman_amd import _lib
from doorman_amd import workloads as W
import hier_model as M
from test_carried_round_gpu import DT, Run, leaf_snapshot, root_config, same
import test_hierarchy_gpu as H

pytestmark = pytest.mark.gpu

NOW = W.NOW_NS
SHAPES = {"300x257": [257] * 300, "150x600": [600] * 150}
STILL = (0.0,)
NEG0 = np.int64(np.iinfo(np.int64).min)  # the bits of -0.0; +0.0's are 0


def pairs(monkeypatch, carry=True):
    """(leaf, root) A with DM_ROUND_STORES=0 and B with the default; both DM_FUSED=2."""
    from doorman_amd.engine import Engine
    for k in ("DM_FIXED", "DM_SWEEP", "DM_STEADY", "DM_CYCLE", "DM_CYCLE_BYTES", "DM_CARRY_ROUND", "DM_ROUND_STORES"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DM_FUSED", "2")
    if not carry:
        monkeypatch.setenv("DM_CARRY_ROUND", "0")
    try:
        monkeypatch.setenv("DM_ROUND_STORES", "0")
        a = (Engine(0), Engine(0))
        monkeypatch.delenv("DM_ROUND_STORES")
        b = (Engine(0), Engine(0))
        return a, b
    finally:
        for k in ("DM_FUSED", "DM_CARRY_ROUND", "DM_ROUND_STORES"):
            monkeypatch.delenv(k, raising=False)


class Clocked(Run):
    """test_carried_round_gpu.Run with the clock's steps and the root's snapshot as arguments."""

    def __init__(self, leaf, root, snap, rcfg, dt=DT, root_snap=None):
        import torch
        from doorman_amd.hierarchy import HierarchicalTick, root_snapshot
        torch.cuda.set_device(0)
        self.torch, self.leaf, self.root, self.rcfg = torch, leaf, root, rcfg
        self.R = R = len(snap["seg_off"]) - 1
        leaf.load(snap)
        root.load(M.with_config(root_snapshot(R, 1, W.FAIR_SHARE, 1.0) if root_snap is None else root_snap, rcfg))
        self.ht = HierarchicalTick(torch, leaf, root, R, 1, 0, None, shard_lo=np.array([0, R]), pipelined=True,
                                   native="local")
        self.t = 0
        self.now = NOW
        self.dt = dt

    def steps(self, n, before=None):
        for _ in range(n):
            if before is not None:
                before(self, self.t)
            self.now += int(self.dt[self.t % len(self.dt)] * W.NS)
            self.ht.tick(self.now, asynchronous=True)
            self.t += 1


def drive(monkeypatch, sizes, script, carry=True, seed=21, dt=DT, snap_edit=None, rcfg_edit=None, root_snap=None):
    """script(run) -> a list of (label, observation); run on A, then on B; A's and B's must be
    equal; -> (A's, B's, (A's rides, B's rides))."""
    (la, ra), (lb, rb) = pairs(monkeypatch, carry)
    try:
        outs, rides = [], []
        for leaf, root in ((la, ra), (lb, rb)):
            rng = np.random.default_rng(seed)
            snap = leaf_snapshot(sizes, rng)
            if snap_edit is not None:
                snap_edit(snap)
            rcfg = root_config(len(sizes), rng)
            if rcfg_edit is not None:
                rcfg_edit(rcfg)
            run = Clocked(leaf, root, snap, rcfg, dt, None if root_snap is None else root_snap(len(sizes)))
            outs.append(script(run))
            rides.append(run.rides()[0])
        assert [x[0] for x in outs[0]] == [x[0] for x in outs[1]]
        for (label, a), (_, b) in zip(*outs):
            same(a, b, label)
        return outs[0], outs[1], rides
    finally:
        for e in (la, ra, lb, rb):
            e.close()


def settle_halve_restore_refresh(run):
    """12 steps (with a standing clock every skippable store is skipped once the exchange has
    settled), the root's capacities halved for two steps and restored, a wants refresh on two
    rows of the leaf; an observation after each."""
    seen = []
    run.steps(12)
    seen.append(("settled", run.observe()))
    halved = {k: np.array(v) for k, v in run.rcfg.items()}
    halved["capacity"] *= 0.5
    run.root.load_config(halved)
    run.steps(2)
    seen.append(("halved", run.observe()))
    run.root.load_config(run.rcfg)
    run.steps(2)
    seen.append(("restored", run.observe()))
    off = run.leaf.seg_off
    rows = np.array([int(off[5]) + 3, int(off[200 % run.R]) + 9], np.int64)
    run.leaf.update_wants(rows, np.array([0.25, 0.75]))
    run.steps(2)  # (a refresh ends the tick's result: steps follow it before the reads)
    seen.append(("refreshed", run.observe()))
    return seen


@pytest.mark.parametrize("carry", [True, False], ids=["riding", "own_launch"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_standing_clock(monkeypatch, shape, carry):
    """`now` constant: once settled the round stores nothing but the staged templates.  A change
    after the long run of skipped stores still lands: the halved capacities move the root's
    grants.  Riding (k_block_fused's ROOT build) and with DM_CARRY_ROUND=0 (k_hier_tick, K = 1)."""
    a, _, (ra, rb) = drive(monkeypatch, SHAPES[shape], settle_halve_restore_refresh, carry=carry, dt=STILL)
    assert a[0][1]["root has"].tobytes() != a[1][1]["root has"].tobytes()
    if carry:
        assert ra > 0 and rb > 0, (ra, rb)
    else:
        assert (ra, rb) == (0, 0), (ra, rb)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_moving_clock(monkeypatch, shape):
    """The same script with uneven steps of `now`: the rows' expiries move every round, so
    only they and the templates are stored."""
    a, _, (ra, rb) = drive(monkeypatch, SHAPES[shape], settle_halve_restore_refresh)
    assert a[0][1]["root has"].tobytes() != a[1][1]["root has"].tobytes()
    assert a[0][1]["root expiry_ns"].tobytes() != a[1][1]["root expiry_ns"].tobytes()
    assert ra > 0 and rb > 0, (ra, rb)


def minus_zero_root(R):
    """One live row per resource; every third holds has = -0.0 and the sum of it, -0.0."""
    third = np.arange(R) % 3 == 0
    has = np.where(third, -0.0, 0.0)
    snap = W.make_snapshot(np.ones(R, np.int64), np.where(third, 5.0, 0.0), has, np.where(third, 1, 0).astype(np.int64),
                           np.where(third, NOW + 1000 * W.NS, W.RELEASED), W.FAIR_SHARE, 1.0)
    snap["agg_sum_has"] = has.copy()
    return snap


def learning_thirds(rcfg):
    rcfg["learning_end_ns"][np.arange(len(rcfg["kind"])) % 3 == 0] = NOW + 1000 * W.NS


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def test_signed_zero_is_replaced(monkeypatch):
    """Every third root row holds has = -0.0 (and its resource sum_has = -0.0) and is in learning
    mode at the root, so the round's grant is the request's Has, +0.0: equal to the word in
    memory by ==, different in bits.  The store must happen."""
    import bench
    R = 300
    third = np.arange(R) % 3 == 0
    # the expected value, on the CPU: the model's grant for such a row, and the Assign's sum
    cfg = (W.FAIR_SHARE, 1000.0, 20, 5, NOW + 1000 * W.NS, W.INT64_MAX, np.nan)
    _, gets = bench.root_round_one(NOW + W.NS, cfg, (5.0, -0.0, 1, NOW + 1000 * W.NS), (1, -0.0, 5.0), 0, 321.0, 257)
    assert bits([gets])[0] == 0
    assert bits([np.float64(-0.0) + (np.float64(gets) - np.float64(-0.0))])[0] == 0

    def script(run):
        before = {"has": run.root.read_store()["has"], "sum_has": run.root.resources(safe=False)["sum_has"]}
        run.steps(1)
        return [("loaded", before), ("one step", run.observe())]

    a, b, _ = drive(monkeypatch, SHAPES["300x257"], script, rcfg_edit=learning_thirds, root_snap=minus_zero_root)
    for outs in (a, b):
        loaded, after = outs[0][1], outs[1][1]
        assert (bits(loaded["has"])[third] == NEG0).all()  # the load kept the sign
        assert (bits(loaded["sum_has"])[third] == NEG0).all()
        assert (bits(after["root has"])[third] == 0).all()
        assert (bits(after["root sums sum_has"])[third] == 0).all()
        assert (after["root subclients"][third] == 257).all()  # the round did decide those rows


def test_signed_zero_in_a_riding_round(monkeypatch):
    """The same inside a leaf launch: after the exchange has settled, an upsert puts has = -0.0
    into every third root row (learning at the root: +0.0 was there); the next round rides."""
    R = 300
    third = np.flatnonzero(np.arange(R) % 3 == 0)

    def script(run):
        run.steps(16)
        st = run.root.read_store()
        run.root.upsert(third, np.full(len(third), -0.0), st["wants"][third], st["subclients"][third],
                        st["expiry_ns"][third])
        put = run.root.read_store()["has"]
        r0 = run.rides()[0]
        run.steps(3)  # the round of the first is carried and rides in the second, the second's in the third
        rode = run.rides()[0] - r0
        return [("upserted", {"has": put}), ("three steps", run.observe()), ("rides", {"n": np.array([rode])})]

    (la, ra), (lb, rb) = pairs(monkeypatch)
    try:
        outs = []
        for leaf, root in ((la, ra), (lb, rb)):
            rng = np.random.default_rng(21)
            snap = leaf_snapshot(SHAPES["300x257"], rng)
            rcfg = root_config(R, rng)
            learning_thirds(rcfg)
            outs.append(script(Clocked(leaf, root, snap, rcfg)))
        for (label, a), (_, b) in zip(*outs):
            if label != "rides":
                same(a, b, label)
        for o in outs:
            assert (bits(o[0][1]["has"])[third] == NEG0).all()
            assert (bits(o[1][1]["root has"])[third] == 0).all()
            assert int(o[2][1]["n"][0]) == 2, o[2]  # the first round after the upsert rode
    finally:
        for e in (la, ra, lb, rb):
            e.close()


def test_lapsed_root_rows(monkeypatch):
    """Root rows with an explicit expiry before `now` (and some that lapse 14 s into the run, in
    a riding round), on resources whose leaf publishes no request (all wants 0): the round's
    Clean releases them, and the next round writes nothing for them."""
    R = 300
    early = np.arange(R) % 7 == 2
    late = np.arange(R) % 7 == 4
    quiet = early | late

    def no_wants(snap):
        so = snap["seg_off"]
        for r in np.flatnonzero(quiet):
            snap["wants"][so[r]:so[r + 1]] = 0.0
        W.add_store_sums(snap)

    def root_snap(n):
        exp = np.where(early, NOW - 5 * W.NS, np.where(late, NOW + 14 * W.NS, W.RELEASED))
        return W.make_snapshot(np.ones(n, np.int64), np.where(quiet, 9.0, 0.0), np.where(quiet, 7.5, 0.0),
                               np.where(quiet, 3, 0).astype(np.int64), exp, W.FAIR_SHARE, 1.0)

    def script(run):
        seen = []
        for i in range(3):
            run.steps(1)
            seen.append((f"step {i + 1}", run.observe()))
        run.steps(14)  # 19 s into the run
        seen.append(("step 17", run.observe()))
        return seen

    a, _, (ra, rb) = drive(monkeypatch, SHAPES["300x257"], script, snap_edit=no_wants, root_snap=root_snap)
    first, last = a[0][1], a[3][1]
    assert (first["root expiry_ns"][early] == W.RELEASED).all() and (first["root has"][early] == 0.0).all()
    assert (first["root expiry_ns"][late] == NOW + 14 * W.NS).all() and (first["root has"][late] == 7.5).all()
    assert (last["root expiry_ns"][late] == W.RELEASED).all() and (last["root sums count"][late] == 0).all()
    assert ra > 0 and rb > 0, (ra, rb)


def test_general_form_three_servers(monkeypatch):
    """k_hier_tick with K = G = 3 rows per resource (the replicated layout on one GPU, as
    test_hierarchy_gpu builds it): R = 50, the root's kinds mixed, the servers' blocks built on
    the host.  Five rounds with a standing clock and the same requests (from the second on,
    every in-place store is skippable), then five with a moving clock, new requests, and a
    server that stops asking for a quarter of the resources (their rows lapse: Clean)."""
    import torch
    from doorman_amd.engine import Engine
    torch.cuda.set_device(0)
    L = _lib.lib()
    R, G = 50, 3
    seen = []
    for stores in ("0", None):
        monkeypatch.delenv("DM_ROUND_STORES", raising=False)
        if stores is not None:
            monkeypatch.setenv("DM_ROUND_STORES", stores)
        rng = np.random.default_rng(17)
        rcfg = H.root_config(R, rng)
        root = H.root_engine(rcfg, G)
        leaf = Engine(0)
        monkeypatch.delenv("DM_ROUND_STORES", raising=False)
        try:
            leaf.load(M.with_config(W.uniform(R, 40, kind=W.FAIR_SHARE, seed=5, capacity=1000.0), M.default_config(R)))
            sw = rng.uniform(10.0, 900.0, (G, R))
            sw[rng.random((G, R)) < 0.15] = 0.0  # no band: the server does not ask
            cnt = rng.integers(1, 40, (G, R)).astype(np.int64)
            now, obs = NOW, []
            for t in range(10):
                if t >= 5:
                    now += (3 + t % 2) * W.NS
                if t == 5:
                    sw = sw * rng.uniform(0.5, 1.5, (G, R))
                    sw[1, :R // 4] = 0.0
                gathered = torch.from_numpy(H.blocks(sw, cnt)).to("cuda")
                torch.cuda.synchronize()
                _lib.check(L.dm_hier_root_tick(root._ctx, gathered.data_ptr(), G, now, leaf._ctx, 0), root._ctx)
                root.sync()
                leaf.sync()
                o = {f"root {k}": v for k, v in root.read_store().items()}
                o.update({f"sums {k}": v for k, v in root.resources(safe=False).items()})
                o.update({f"template {k}": v for k, v in leaf.config().items()})
                obs.append((f"round {t}", o))
            seen.append(obs)
        finally:
            root.close()
            leaf.close()
    for (label, a), (_, b) in zip(*seen):
        same(a, b, label)
    a = seen[0]
    assert a[0][1]["root has"].any()
    assert a[4][1]["root has"].tobytes() == a[1][1]["root has"].tobytes()  # the standing rounds repeat themselves
    assert (a[9][1]["root expiry_ns"] == W.RELEASED).sum() > (a[4][1]["root expiry_ns"] == W.RELEASED).sum()  # lapsed


def test_listed_and_rest_items_beside_the_round(monkeypatch):
    """test_carried_round_gpu.test_listed_and_rest_items_inside_a_riding_launch's script (released
    rows and an upsert under dm_keep_keys mode 3: rest items and listed items beside done ones)
    under this switch: the round runs, and skips what it may, in the lanes of those items too."""
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
        rode = run.rides()[0] - r0
        run.leaf.upsert(rows[:1], np.zeros(1), np.full(1, 0.125), np.ones(1, np.int64),
                        np.full(1, run.now + 200 * W.NS))
        run.steps(5)
        seen.append(("after the upsert", run.observe()))
        seen.append(("rode", {"n": np.array([rode], np.int64)}))
        return seen

    a, b, _ = drive(monkeypatch, SHAPES["300x257"], script, seed=9)
    for outs in (a, b):
        assert int(outs[3][1]["n"][0]) >= 1, outs[3]
        for r in picked:  # one root row per resource: the round reached these lanes
            assert outs[0][1]["root wants"][r] != outs[1][1]["root wants"][r], r
