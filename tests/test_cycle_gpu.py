"""The cycle form of the dense tick (dm_tick_steady.h: the cycle builds of k_sweep / k_block_list,
dm_device.h CycAux): a steady writeback tick on the alternate column
moves no row of a resource whose tick provably reproduces its state of two ticks ago, which
the destination column still holds; only its record alternates.

Nothing a caller can read may depend on it: engine A (DM_CYCLE=0: the plain builds on the
alternate column, as before) and engine B (the default) hold identical bits after every tick
(leases, rows, records, configuration), and B matches the oracle at the suite's tolerance.

The stores are workloads.uniform_range(48, n, 0, 48, seed=3): oversubscribed FairShare
resources, of which some wobble with period two (C - SumHas is a rounding residue whose sign
flips each tick).  That is a condition of the device's own summation order, so every case
first asserts it on the control engine's rows and sums after ticks 6, 7 and 8.
"""
import numpy as np
import pytest

from doorman_amd import _lib
from doorman_amd import workloads as W
import test_fixed_point_gpu as FP
from test_skip_unchanged_gpu import copy_of

pytestmark = pytest.mark.gpu

NOW = W.NOW_NS
SIZES = (257, 1000, 1025, 4096)  # one per dense instance


def cycle_engines(monkeypatch, n=1):
    """n engines with DM_CYCLE=0 and n with the default (read when the context is created)."""
    from doorman_amd.engine import Engine
    for k in ("DM_FIXED", "DM_SWEEP", "DM_STEADY"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DM_CYCLE", "0")
    a = [Engine(0) for _ in range(n)]
    monkeypatch.delenv("DM_CYCLE")
    return a, [Engine(0) for _ in range(n)]


class CyclePair(FP.Pair):
    """test_fixed_point_gpu.Pair with A = DM_CYCLE=0 and B = the default; a tick writes the
    alternate column unless told otherwise."""

    def __init__(self, monkeypatch, snap):
        monkeypatch.setattr(FP, "engines", cycle_engines)
        super().__init__(monkeypatch, snap)
        self.t = -2  # (the first tick at NOW: the loaded leases' expiries begin at NOW + 1 s)

    def counts(self, label):
        """B's (cycle_parts, fixed_items, cycling_items); A never runs the form."""
        a = self.A.plan_info()
        assert a["cycle_parts"] == 0 and self.A.store_stats()["cycling_items"] == 0, label
        s = self.B.store_stats()
        return self.B.plan_info()["cycle_parts"], s["fixed_items"], s["cycling_items"]

    def tick(self, label, dt=None, oracle=True, **kw):
        kw.setdefault("wb_columns", "alternate" if kw.get("writeback", True) else "auto")
        if dt is None:
            self.t += 2
            dt = self.t
        else:
            self.t = dt
        return super().tick(label, dt, oracle=oracle, **kw)

    def more(self, label, n=4, engaged=True):
        """n more ticks; the last must run the form with the keys in use again (engaged)."""
        for i in range(n):
            out = self.tick(f"{label}: tick {i + 1} after")
        assert not engaged or out[0] > 0, (label, out)
        return out

    def state(self, e):
        return e.read_store()["has"].view(np.int64).copy(), e.resources()["sum_has"].view(np.int64).copy()


def per_resource(off, same_rows):
    return np.array([same_rows[off[r]:off[r + 1]].all() for r in range(len(off) - 1)])


def settle(P, big):
    """Eight ticks.  On the control engine's own rows and sums after ticks 6, 7 and 8: at least
    4 resources are in a cycle of period two that is no fixed point.  B ran the form, and
    exactly the workgroup-bin resources whose state repeats after two ticks hold valid keys,
    those of them whose sums alternate counted as cycling."""
    st = {}
    for t in range(1, 9):
        out = P.tick(f"tick {t}", oracle=t in (1, 2, 3, 8))
        if t >= 6:
            st[t] = P.state(P.A)
    off = P.off
    same = lambda a, b: per_resource(off, st[a][0] == st[b][0]) & (st[a][1] == st[b][1])
    back, still = same(6, 8), same(6, 7) & same(7, 8)
    cyc = back & ~still
    print(f"two-cycles {int(cyc.sum())}, fixed {int(still.sum())}, neither {int((~back).sum())} of {len(back)}")
    assert cyc[big].sum() >= 4, (int(cyc[big].sum()), "resources in a two-cycle that is no fixed point")
    parts, items, cycling = out
    assert parts > 0, out
    assert items == int(back[big].sum()), (out, int(back[big].sum()))
    assert cycling == int((back & (st[7][1] != st[8][1]))[big].sum()), out
    return cyc, still


def uniform_store(n):
    return W.uniform_range(48, n, 0, 48, seed=3)


def mixed_store():
    """All four sizes (12 resources each), a ProportionalShare resource of 300 rows and a
    sub-wave resource of 40."""
    parts = [W.uniform_range(12, n, 0, 12, seed=3) for n in SIZES]
    parts.append(W.uniform_range(1, 300, 0, 1, kind=W.PROPORTIONAL_SHARE, seed=4))
    parts.append(W.uniform_range(1, 40, 0, 1, seed=5))
    sizes = np.concatenate([np.diff(p["seg_off"]) for p in parts])
    cat = lambda k: np.concatenate([np.asarray(p[k]) for p in parts])
    return W.make_snapshot(sizes, cat("wants"), cat("has"), cat("subclients"), cat("expiry_ns"), cat("kind"),
                           cat("capacity"), lease_length_s=cat("lease_length_s"),
                           refresh_interval_s=cat("refresh_interval_s"))


def big_of(snap):
    return np.diff(np.asarray(snap["seg_off"])) >= 257


@pytest.mark.parametrize("n", SIZES)
def test_every_dense_instance_settles_into_the_form(monkeypatch, n):
    snap = uniform_store(n)
    P = CyclePair(monkeypatch, snap)
    try:
        settle(P, big_of(snap))
        P.more("steady")
    finally:
        P.close()


def pick(snap, group, n=None):
    off = np.asarray(snap["seg_off"])
    return int(next(r for r in np.flatnonzero(group) if n is None or off[r + 1] - off[r] == n))


def test_ticks_and_times_that_end_a_cycle_without_a_row_write(monkeypatch):
    """The mixed store through what ends or refutes a key with no row written by a call: the
    capacity halved and restored and the kind changed (dm_config_load), learning mode begun
    and ended by time alone, a parent expiry passing, one non-writeback, one in-place and one
    recompute tick, and the followers lapsing.  Four more ticks after each."""
    snap = mixed_store()
    big = big_of(snap)
    R = len(big)
    P = CyclePair(monkeypatch, snap)
    try:
        cyc, still = settle(P, big)
        c, f = pick(snap, cyc & big), pick(snap, still & big) if (still & big).any() else pick(snap, cyc & big)
        cfg = {k: np.array(P.host[k]) for k in W.CFG_FIELDS}

        def load(label, **ch):
            for k, (r, v) in ch.items():
                cfg[k][r] = v
                P.host[k] = cfg[k].copy()
            P.both(lambda e: e.load_config(P.host))
            P.more(label)

        cap = cfg["capacity"][c]
        load("capacity halved", capacity=(c, cap * 0.5))
        load("capacity restored", capacity=(c, cap))
        load("kind changed", kind=(c, W.PROPORTIONAL_SHARE))
        load("kind restored", kind=(c, W.FAIR_SHARE))
        # learning mode from P.t + 3 s to P.t + 9 s, and a parent expiry at P.t + 13 s: by time alone
        t0 = P.t
        cfg["learning_end_ns"][f] = NOW + (t0 + 9) * W.NS
        cfg["parent_expiry_ns"][c] = NOW + (t0 + 13) * W.NS
        P.host["learning_end_ns"], P.host["parent_expiry_ns"] = cfg["learning_end_ns"].copy(), cfg["parent_expiry_ns"].copy()
        P.both(lambda e: e.load_config(P.host))
        P.more("learning mode ends and the parent expiry passes", 10)
        for what, kw in (("no writeback", {"writeback": False}), ("in place", {"wb_columns": "inplace"}),
                         ("recompute", {"recompute": True})):
            assert P.tick(f"{what} tick", **kw)[0] == 0
            assert P.tick(f"first tick after the {what} tick")[0] == 0  # every key rewritten, none trusted
            P.more(what)
        P.tick("lapse", P.t + 400)
        gets, exp = P.B.leases()
        assert not gets.any() and (exp == W.RELEASED).all()
        P.more("lapse", engaged=False)  # (a store of released rows runs no steady build)
    finally:
        P.close()


@pytest.mark.parametrize("mode", [0, 1, 3])
def test_row_writes_under_the_keep_modes(monkeypatch, mode):
    """A wants refresh, a release and an upsert of one row in a cycling and in a fixed (or a
    second cycling) resource under dm_keep_keys 0, 1 and 3, then dm_store_relayout and a
    reload.  Four more ticks after each: a kept key-clearing update leaves state 0, and the
    next tick rewrites that resource's destination rows."""
    snap = mixed_store()
    big = big_of(snap)
    P = CyclePair(monkeypatch, snap)
    try:
        P.both(lambda e: e.keep_keys(mode))
        cyc, still = settle(P, big)
        c = pick(snap, cyc & big)
        others = (still if (still & big).any() else cyc) & big
        others[c] = False
        f = pick(snap, others)
        for r in (c, f):
            row = np.array([P.row(r, 70)], np.int64)
            P.set_wants(row, [P.host["wants"][row[0]] * 0.5 + 1.0 / 1024])
            P.more(f"wants refresh in {r}")
            P.both(lambda e: e.release(row))
            P.host["has"][row], P.host["wants"][row], P.host["subclients"][row] = 0.0, 0.0, 0
            P.host["expiry_ns"][row] = W.RELEASED
            W.add_store_sums(P.host)
            P.more(f"release in {r}", engaged=False)  # (a released row: steady only under DM_KEEP_UPDATES)
            ne = NOW + (P.t + 200) * W.NS
            P.both(lambda e: e.upsert(row, np.zeros(1), np.full(1, 0.125), np.ones(1, np.int64), np.full(1, ne)))
            P.host["has"][row], P.host["wants"][row], P.host["subclients"][row] = 0.0, 0.125, 1
            P.host["expiry_ns"][row] = ne
            W.add_store_sums(P.host)
            P.more(f"upsert in {r}", 5)
        off = np.asarray(snap["seg_off"])
        P.both(lambda e: e.relayout(off))
        P.more("relayout")
        again = P.A.read_store()
        reload = copy_of(P.host)
        for k in ("has", "wants", "subclients", "expiry_ns"):
            reload[k] = again[k]
        W.add_store_sums(reload)
        P.both(lambda e: e.load(reload))
        P.host = copy_of(reload)
        P.more("reload", 6)
    finally:
        P.close()


def test_a_worklist_longer_than_the_grid_and_an_empty_one(monkeypatch):
    """1,100 resources of 257 rows under capacity (every one at a fixed point: the worklist is
    empty and the told count 0), 600 of which share a parent expiry that passes between two
    ticks with no call: the next tick's row kernel strides over 600 refuted keys from a grid
    of 16 workgroups."""
    import test_fixed_sweep_gpu as FS
    K, hit = 1100, np.arange(250, 850)
    snap = FS.bin_store(K, set(), None, seed=9)
    snap["parent_expiry_ns"] = np.where(np.isin(np.arange(K), hit), NOW + 13 * W.NS, W.INT64_MAX).astype(np.int64)
    P = CyclePair(monkeypatch, snap)
    try:
        for t in range(6):
            parts, items, cycling = P.tick(f"tick {t + 1}", oracle=t == 5)
        assert parts > 0 and items == K and cycling == 0, (parts, items, cycling)  # an empty worklist
        parts, items, _ = P.tick("the tick after the time", 14)
        assert parts > 0 and items <= K - len(hit), (parts, items)
        parts, items, _ = P.more("the time")
        assert items == K, items
    finally:
        P.close()


def test_the_form_never_runs_in_place_or_with_dm_cycle_0(monkeypatch):
    """DM_WB_INPLACE keeps FIXED: no tick of a store told to tick in place runs the form."""
    snap = uniform_store(257)
    (a,), (b,) = cycle_engines(monkeypatch)
    try:
        for e in (a, b):
            e.load(snap)
            for t in range(5):
                e.apportion(NOW + 2 * t * W.NS, writeback=True, wb_columns="inplace")
                assert e.plan_info()["cycle_parts"] == 0
            assert e.plan_info()["fixed_parts"] > 0
        FP.assert_same_state(a, b, "in place")
    finally:
        a.close()
        b.close()


def auto_engines(monkeypatch, n=1):
    """cycle_engines with DM_CYCLE_BYTES=0 (the test hook): a store of any size may ask for the
    alternate column by itself, as a store above 1 GiB does."""
    monkeypatch.setenv("DM_CYCLE_BYTES", "0")
    try:
        return cycle_engines(monkeypatch, n)
    finally:
        monkeypatch.delenv("DM_CYCLE_BYTES")


def test_a_store_engages_by_itself_and_a_fixed_store_never_does(monkeypatch):
    """No column flag on any tick.  The 1,000-row store has resources that are never at a fixed
    point: after the in-place sweep has told a non-empty list on 8 consecutive ticks B goes to
    the alternate column (dm_plan_info wb_inplace 0) and runs the form, is judged by the stamped
    count of its 8th cycle-form tick and stays; A (DM_CYCLE=0) stays in place.  Identical bits
    after every tick, the oracle on the last.  A store of resources under capacity (every one
    at its fixed point: an empty list) never leaves in place."""
    import test_fixed_sweep_gpu as FS
    monkeypatch.setattr(FP, "engines", auto_engines)
    for snap, engages in ((uniform_store(1000), True), (FS.bin_store(70, set(), None, seed=9), False)):
        P = FP.Pair.__new__(CyclePair)
        FP.Pair.__init__(P, monkeypatch, snap)
        P.t = -2
        try:
            went = []
            for t in range(40):
                parts, items, cycling = P.tick(f"tick {t + 1}", oracle=t == 39, wb_columns="auto")
                a, b = P.A.plan_info(), P.B.plan_info()
                assert a["wb_inplace"] == 1 and a["cycle_parts"] == 0, t
                went.append((b["wb_inplace"], parts, items, cycling))
            print(went)
            if not engages:
                assert all(w[0] == 1 and w[1] == 0 for w in went), went
                continue
            first = next(i for i, w in enumerate(went) if w[0] == 0)
            assert 10 <= first <= 14, (first, went)  # hints, keys, then 8 told sweeps
            assert all(w[0] == 0 for w in went[first:]), went  # judged and stayed
            assert went[-1][1] > 0 and went[-1][2] == 48 and went[-1][3] >= 4, went[-1]
        finally:
            P.close()


def test_capacity_halved_and_restored_through_the_pipelined_exchange(monkeypatch):
    """test_fixed_sweep_gpu's leaf under the pipelined exchange (its templates are rewritten on
    the device every step), with A = DM_CYCLE=0 and B = the default, both free to ask for the
    alternate column by themselves (DM_CYCLE_BYTES=0): B engages as bench.py's default line
    does.  Then the root halves the capacity of a resource whose key holds and restores it two
    steps later; four more steps.  After every step, bit for bit: leases, templates (capacity
    and kind among them), leaf and root stores, the published blocks (the ring of three) and the
    root's verdict.  B runs the form with valid keys before the halving and at the end, and the
    halved resource's leases move."""
    import torch
    import hier_model as M
    from doorman_amd.hierarchy import HierarchicalTick, root_snapshot
    torch.cuda.set_device(0)
    rng = np.random.default_rng(21)
    sizes = np.concatenate([rng.integers(257, 513, 140), rng.integers(513, 1100, 30), rng.integers(1025, 4097, 6)])
    R = len(sizes)
    rcfg = {"kind": rng.choice([W.FAIR_SHARE, W.PROPORTIONAL_SHARE, W.STATIC, W.NO_ALGORITHM], R).astype(np.int32),
            "capacity": rng.choice([100.0, 1000.0, 2500.5], R),
            "lease_length_s": rng.choice([20, 60], R).astype(np.int64),
            "refresh_interval_s": rng.choice([1, 5], R).astype(np.int64),
            "learning_end_ns": np.full(R, W.INT64_MIN, np.int64),
            "parent_expiry_ns": np.full(R, W.INT64_MAX, np.int64),
            "safe_capacity": np.where(rng.random(R) < 0.5, np.nan, rng.uniform(1, 9, R))}
    full = W.make_snapshot(sizes, rng.uniform(0.2, 3.0, int(sizes.sum())) * 1000.0 / np.repeat(sizes, sizes),
                           0.0, 1, NOW + 60 * W.NS, W.FAIR_SHARE, 1000.0)
    off = np.concatenate([[0], np.cumsum(sizes)])
    shared = rcfg["kind"] >= W.PROPORTIONAL_SHARE  # the kinds whose gets depend on the capacity
    HALVE, RESTORE, STEPS = 30, 32, 37
    (la, ra), (lb, rb) = auto_engines(monkeypatch, 2)
    try:
        runs = []
        for leaf, root in ((la, ra), (lb, rb)):
            leaf.load(M.with_config(full, M.default_config(R)))
            root.load(M.with_config(root_snapshot(R, 1, W.FAIR_SHARE, 1.0), rcfg))
            ht = HierarchicalTick(torch, leaf, root, R, 1, 0, None, shard_lo=np.array([0, R]), pipelined=True,
                                  native="local")
            out, info, target = [], [], None
            for t in range(STEPS):
                now = NOW + t * W.NS // 2
                if t == HALVE:  # a capacity-dependent resource whose leases repeat after two steps
                    g1, g3 = out[-1][0][0], out[-3][0][0]
                    target = next(r for r in range(R) if shared[r] and g1[off[r]:off[r + 1]].any() and
                                  g1[off[r]:off[r + 1]].tobytes() == g3[off[r]:off[r + 1]].tobytes())
                    halved = {k: np.array(v) for k, v in rcfg.items()}
                    halved["capacity"][target] *= 0.5
                    root.load_config(halved)
                if t == RESTORE:
                    root.load_config(rcfg)
                ht.tick(now)
                leases, cfg = leaf.leases(), leaf.config()
                pub = torch.stack(ht.totals).cpu().numpy().tobytes()
                pi, ss = leaf.plan_info(), leaf.store_stats()
                info.append((pi["wb_inplace"], pi["cycle_parts"], ss["fixed_items"], ss["cycling_items"]))
                out.append((leases, cfg, leaf.read_store(), root.read_store(), ht.status(), pub))
            runs.append((out, info, target))
        (oa, ia, ta), (ob, ib, tb) = runs
        print(ib)
        assert all(w[0] == 1 and w[1] == 0 and w[3] == 0 for w in ia), ia
        assert ta == tb
        for w in (ib[HALVE - 1], ib[-1]):  # the alternate column, the form in every bin's part, valid keys, cycles among them
            assert w[0] == 0 and w[1] > 0 and w[2] > 0 and w[3] > 0, w
        gets = [o[0][0][off[tb]:off[tb + 1]] for o in ob]
        assert any(not np.array_equal(gets[t], gets[t - 2]) for t in range(HALVE, RESTORE + 3)), tb
        for t, (a, b) in enumerate(zip(oa, ob)):
            for x, y in zip(a[0], b[0]):
                assert x.tobytes() == y.tobytes(), f"step {t}: leases"
            for k in W.CFG_FIELDS:
                assert a[1][k].tobytes() == b[1][k].tobytes(), f"step {t}: template {k}"
            for k in ("has", "wants", "subclients", "expiry_ns"):
                assert a[2][k].tobytes() == b[2][k].tobytes(), f"step {t}: leaf {k}"
                assert a[3][k].tobytes() == b[3][k].tobytes(), f"step {t}: root {k}"
            assert a[4].tobytes() == b[4].tobytes(), f"step {t}: the root's verdict on the request"
            assert a[5] == b[5], f"step {t}: the published blocks"
    finally:
        for e in (la, ra, lb, rb):
            e.close()
