"""The FIXED build of the dense tick kernel (dm_tick_group.hip group_segment):
a part that runs a steady build on a writeback tick in place keeps a key per resource, set
when the resource's tick stored no gets, reduced a delta of +0.0 and wrote back the record it
read; while the key matches the resource's effective capacity and kind, and nothing but
such builds has touched its rows, running sums or state (the host's fix_live), the next
tick loads no row of it and writes the record it would have written.

Nothing a caller can read may depend on it: engine A (DM_FIXED=0, the steady builds as
they were) and engine B (the default) hold identical bits after every tick, through every
way a key can stop being true: row writes (a wants refresh, a release, an arrival, a NaN
wants), a capacity change by a call (load_config) and with no call at all (a parent expiry
that passes, learning mode that ends, a template the exchange rewrites on the device), ticks
that are not FIXED between ticks that are (non-writeback, recompute, alternate column), a
lapse of every follower, a re-layout and a reload.  dm_plan_info's "fixed_parts" says
whether the last tick ran with keys in use, dm_store_stats' "fixed_items" how many keys are
valid and in use right now (none after a call that wrote rows).

The store is test_skip_unchanged_gpu.make_store's (two resources at each first and last row
count of every dense instance, one under capacity and one over with dyadic wants), with a
few of the under-capacity resources given kinds 0 and 1, one learning until NOW + 9 s and one
whose parent expiry passes at NOW + 13 s.  The oracle alone confirms that every
under-capacity resource outside learning mode is a fixed point from tick 2 on (a condition
of the data, not a device result)."""
import numpy as np
import pytest

from doorman_amd import workloads as W
from oracle import oracle as O
import hier_model as M
from parity_util import assert_leases_match
from test_skip_unchanged_gpu import copy_of, host_tick, make_store
from test_steady_dense_gpu import assert_same_state

pytestmark = pytest.mark.gpu

NOW = W.NOW_NS
COLS = ("has", "wants", "subclients", "expiry_ns")


def fixed_store():
    """(snapshot, under, over, learning resource, parent-expiry resource)"""
    snap, under, over = make_store()
    off = np.asarray(snap["seg_off"])
    size = lambda r: int(off[r + 1] - off[r])
    by_size = lambda n: next(r for r in under if size(r) == n)
    for k in ("kind", "learning_end_ns", "parent_expiry_ns"):
        snap[k] = np.array(snap[k])
    snap["kind"][by_size(257)] = W.NO_ALGORITHM
    snap["kind"][by_size(2048)] = W.STATIC
    snap["kind"][by_size(4096)] = W.STATIC
    learn, pexp = by_size(513), by_size(1025)
    snap["learning_end_ns"][learn] = NOW + 9 * W.NS
    snap["parent_expiry_ns"][pexp] = NOW + 13 * W.NS
    return snap, under, over, learn, pexp


def unchanged_by_tick(host, now):
    """Per resource: the oracle's writeback tick at `now` leaves every row's has bit for bit
    unchanged (advances host)."""
    off = host["seg_off"]
    before = host["has"].copy()
    host_tick(host, now)
    same = before.view(np.int64) == host["has"].view(np.int64)
    return np.array([same[off[r]:off[r + 1]].all() for r in range(len(off) - 1)])


@pytest.fixture(scope="module")
def store():
    snap, under, over, learn, pexp = fixed_store()
    host = copy_of(snap)
    host_tick(host, NOW)
    for t in (1, 2):  # the data's condition: ticks 2 and 3 leave the under-capacity resources as they are
        same = unchanged_by_tick(host, NOW + 2 * t * W.NS)
        assert same[under].all(), f"tick {t + 1}: {np.asarray(under)[~same[under]]}"
    return snap, under, over, learn, pexp


def engines(monkeypatch, n=1):
    """n engines with DM_FIXED=0 and n with the default (read when the context is created)."""
    from doorman_amd.engine import Engine
    monkeypatch.setenv("DM_FIXED", "0")
    a = [Engine(0) for _ in range(n)]
    monkeypatch.delenv("DM_FIXED")
    return a, [Engine(0) for _ in range(n)]


class Pair:
    """Engine A (DM_FIXED=0) and engine B (the default) on the same store, and the oracle's
    host copy of it."""

    def __init__(self, monkeypatch, snap):
        (self.A,), (self.B,) = engines(monkeypatch)
        self.host = copy_of(snap)
        self.off = np.asarray(snap["seg_off"])
        try:
            self.both(lambda e: e.load(snap))
        except Exception:
            self.close()
            raise

    def close(self):
        self.A.close()
        self.B.close()

    def both(self, fn):
        fn(self.A)
        fn(self.B)

    def counts(self, label):
        """B's (fixed_parts, fixed_items); A's are 0 throughout."""
        assert self.A.plan_info()["fixed_parts"] == 0 and self.A.store_stats()["fixed_items"] == 0, label
        return self.B.plan_info()["fixed_parts"], self.B.store_stats()["fixed_items"]

    def tick(self, label, dt, oracle=False, **kw):
        """One tick of both engines at NOW + dt s (writeback unless said otherwise); identical
        bits after it; with oracle, B's leases against the oracle's on the host copy.  A
        writeback tick advances the host copy.  Returns B's (fixed_parts, fixed_items)."""
        now = NOW + dt * W.NS
        kw.setdefault("writeback", True)
        self.both(lambda e: e.apportion(now, **kw))
        assert_same_state(self.A, self.B, label)
        if oracle:
            assert_leases_match(self.host, *self.B.leases(), O.apportion(self.host, now), label)
        if kw["writeback"]:
            host_tick(self.host, now)
        return self.counts(label)

    def set_wants(self, rows, nw):
        rows, nw = np.asarray(rows, np.int64), np.asarray(nw, np.float64)
        self.both(lambda e: e.update_wants(rows, nw))
        self.host["wants"][rows] = nw
        W.add_store_sums(self.host)

    def row(self, r, i):
        return int(self.off[r] + i)


def by_size(snap, group, n):
    off = snap["seg_off"]
    return next(r for r in group if off[r + 1] - off[r] == n)


def test_keys_engage_and_row_writes_end_them(monkeypatch, store):
    """Three writeback ticks engage the keys (the first sets the hints, the second runs the
    FIXED build and writes every key, the third uses them): fixed_parts > 0 and at least
    the under-capacity resources outside learning mode hold a valid key.  Then the calls
    that write rows, each starting a row epoch in which no key is trusted until a FIXED
    launch has rewritten them: a wants refresh of one row of a fixed resource, a release in
    another and an arrival into the freed slot, load_config halving a fixed resource's
    capacity, a NaN wants in a FairShare resource (k_general) and its repair.  Identical
    bits after every tick; B matches the oracle after the keys engage and after each event."""
    snap, under, over, learn, pexp = store
    n_under = len(under) - 1  # (one is learning until NOW + 9 s)
    P = Pair(monkeypatch, snap)
    try:
        assert P.counts("loaded") == (0, 0)
        assert P.tick("tick 1", 0) == (0, 0)  # no hints before the first writeback tick
        parts, _ = P.tick("tick 2", 2)  # the first FIXED launch: every key rewritten, none trusted
        assert parts == 0
        parts, items = P.tick("tick 3", 4, oracle=True)
        assert parts > 0 and items >= n_under, (parts, items)

        r = by_size(snap, under, 1000)  # a fixed resource: one row of its second wave
        P.set_wants([P.row(r, 70)], [P.host["wants"][P.row(r, 70)] * 0.5 + 1.0 / 1024])
        assert P.counts("wants refresh")[1] == 0  # a new row epoch: no key is in use
        assert P.tick("tick 4 (wants refresh)", 6, oracle=True)[0] == 0
        assert P.tick("tick 5", 8)[0] == 0  # keys rewritten ...
        parts, items = P.tick("tick 6", 10, oracle=True)  # ... and used (learning ended at NOW + 9 s)
        assert parts > 0 and items >= n_under, (parts, items)

        r = by_size(snap, under, 1024)
        freed = np.array([P.row(r, 700)], np.int64)
        P.both(lambda e: e.release(freed))
        P.host["has"][freed], P.host["wants"][freed], P.host["subclients"][freed] = 0.0, 0.0, 0
        P.host["expiry_ns"][freed] = W.RELEASED
        W.add_store_sums(P.host)
        assert P.counts("release")[1] == 0
        P.tick("tick 7 (release)", 12, oracle=True)
        ne = NOW + 112 * W.NS
        P.both(lambda e: e.upsert(freed, np.zeros(1), np.full(1, 0.125), np.ones(1, np.int64), np.full(1, ne)))
        P.host["has"][freed], P.host["wants"][freed], P.host["subclients"][freed] = 0.0, 0.125, 1
        P.host["expiry_ns"][freed] = ne
        W.add_store_sums(P.host)
        P.tick("tick 8 (arrival)", 14, oracle=True)  # (the parent expiry of one resource has passed too)
        P.tick("tick 9", 16)
        P.tick("tick 10", 18)
        parts, items = P.tick("tick 11", 20, oracle=True)
        assert parts > 0 and items >= n_under - 1, (parts, items)

        r = by_size(snap, over, 1024)  # a fixed point of the data (test_skip_unchanged_gpu.store)
        P.host["capacity"] = P.host["capacity"].copy()
        P.host["capacity"][r] *= 0.5
        P.both(lambda e: e.load_config(P.host))
        assert P.counts("load_config")[1] == 0
        P.tick("tick 12 (capacity halved)", 22, oracle=True)
        P.tick("tick 13", 24)
        parts, items = P.tick("tick 14", 26, oracle=True)
        assert parts > 0, parts

        r = next(x for x in under if snap["kind"][x] == W.FAIR_SHARE and x not in (learn, pexp))
        keep = P.host["wants"][P.row(r, 5)]
        P.set_wants([P.row(r, 5)], [np.nan])
        P.tick("tick 15 (NaN wants)", 28)
        P.tick("tick 16", 30)
        P.set_wants([P.row(r, 5)], [keep])
        P.tick("tick 17 (repaired)", 32)
        P.tick("tick 18", 34)
        P.tick("tick 19", 36)
        parts, items = P.tick("tick 20", 38)
        assert parts > 0 and items > 0, (parts, items)
    finally:
        P.close()


def test_ticks_and_times_that_end_a_fixed_point_without_a_call(monkeypatch, store):
    """No call writes a row here.  Learning mode ends (NOW + 9 s: the learning resource's
    rows kept their has until then and take their wants after) and a parent expiry passes
    (NOW + 13 s: C goes to 0) between two FIXED ticks with keys in use; a non-writeback
    tick, a recompute tick and an alternate-column tick run between in-place ticks (each
    clears fix_live: the next FIXED launch rewrites the keys); a tick 25 s later finds every
    follower of the 20-s leases lapsed (the queueing path clears the keys) and the tick after
    it decides a store of released rows.  Identical bits after every tick, and B matches
    the oracle across the two times and the lapse."""
    snap, under, over, learn, pexp = store
    P = Pair(monkeypatch, snap)
    try:
        P.tick("tick 1", 0)
        P.tick("tick 2", 2)
        parts, items = P.tick("tick 3", 4)
        assert parts > 0 and items >= len(under) - 1, (parts, items)
        lo, hi = P.off[learn], P.off[learn + 1]
        assert not np.array_equal(P.host["has"][lo:hi], P.host["wants"][lo:hi])  # learning: has kept
        P.tick("tick 4", 6)
        parts, before = P.tick("tick 5", 8, oracle=True)
        assert parts > 0
        parts, _ = P.tick("tick 6 (learning ended)", 10, oracle=True)
        assert parts > 0
        np.testing.assert_array_equal(P.B.read_store()["has"][lo:hi], P.host["wants"][lo:hi])
        parts, _ = P.tick("tick 7", 12, oracle=True)
        assert parts > 0
        lo, hi = P.off[pexp], P.off[pexp + 1]
        before = P.B.read_store()["has"][lo:hi]
        np.testing.assert_array_equal(before, P.host["wants"][lo:hi])  # under capacity: gets == wants
        parts, _ = P.tick("tick 8 (parent expiry passed)", 14, oracle=True)  # its key must not match: C is 0 now
        assert parts > 0
        assert (P.B.read_store()["has"][lo:hi] < before).all()  # nothing is available any more
        parts, items = P.tick("tick 9", 16, oracle=True)
        # (fixed again but for the resource without capacity, which need not settle)
        assert parts > 0 and items >= len(under) - 1, (parts, items)

        for k, (what, kw) in enumerate([("no writeback", {"writeback": False}), ("recompute", {"recompute": True}),
                                        ("alternate column", {"wb_columns": "alternate"})]):
            dt = 18 + 6 * k
            assert P.tick(f"{what} tick", dt, oracle=True, **kw) == (0, 0)
            assert P.tick(f"first tick after the {what} tick", dt + 2)[0] == 0  # keys rewritten, not trusted
            parts, items = P.tick(f"second tick after the {what} tick", dt + 4, oracle=True)
            assert parts > 0 and items >= len(under) - 1, (what, parts, items)

        P.tick("lapse", 34 + 25, oracle=True)
        gets, exp = P.B.leases()
        assert not gets.any() and (exp == W.RELEASED).all()  # every follower lapsed
        P.tick("after the lapse", 34 + 27, oracle=True)
        P.tick("and again", 34 + 29)
    finally:
        P.close()


def test_capacity_there_and_back_under_the_exchange(monkeypatch):
    """A leaf under the pipelined exchange (test_steady_dense_gpu's: its templates change on
    the device from step to step, lease lengths and kinds included, with no row epoch on the
    leaf).  Between two steps the root halves the capacity of a resource at its fixed point
    (root.load_config), and restores it a step later: the leaf's rows changed in between,
    so the old key must not match.  While it is halved the leaf also runs a recompute tick of
    its own between two steps (not a FIXED launch: fix_live).  Leases, templates, leaf and
    root stores and the root's verdict are the same bits as with DM_FIXED=0 at every step,
    and the leaf's keys are in use before and after."""
    import torch
    from doorman_amd.hierarchy import HierarchicalTick, root_snapshot
    torch.cuda.set_device(0)
    rng = np.random.default_rng(21)
    sizes = np.concatenate([rng.integers(257, 1100, 60), rng.integers(1025, 4097, 6)])
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
    HALVE, EXTRA, RESTORE, STEPS = 9, 10, 11, 18
    (la, ra), (lb, rb) = engines(monkeypatch, 2)
    try:
        runs = []
        for leaf, root in ((la, ra), (lb, rb)):
            leaf.load(M.with_config(full, M.default_config(R)))
            root.load(M.with_config(root_snapshot(R, 1, W.FAIR_SHARE, 1.0), rcfg))
            ht = HierarchicalTick(torch, leaf, root, R, 1, 0, None, shard_lo=np.array([0, R]), pipelined=True,
                                  native="local")
            out, parts, items, target = [], [], [], None
            for t in range(STEPS):
                now = NOW + 2 * t * W.NS
                if t == HALVE:
                    # a resource the last step left bit for bit as it was (the same one in both
                    # runs, their leases being the same bits), of a kind that shares its capacity
                    g1, g2 = out[-1][0][0], out[-2][0][0]
                    target = next(r for r in range(R) if shared[r] and g1[off[r]:off[r + 1]].any() and
                                  g1[off[r]:off[r + 1]].tobytes() == g2[off[r]:off[r + 1]].tobytes())
                    halved = {k: np.array(v) for k, v in rcfg.items()}
                    halved["capacity"][target] *= 0.5
                    root.load_config(halved)
                if t == RESTORE:
                    root.load_config(rcfg)
                if t == EXTRA:
                    leaf.apportion(now - W.NS, writeback=True, recompute=True)
                ht.tick(now)
                parts.append(leaf.plan_info()["fixed_parts"])
                items.append(leaf.store_stats()["fixed_items"])
                out.append((leaf.leases(), leaf.config(), leaf.read_store(), root.read_store(), ht.status()))
            runs.append((out, parts, items, target))
        (oa, pa, ia, ta), (ob, pb, ib, tb) = runs
        assert not any(pa) and not any(ia), (pa, ia)
        assert pb[HALVE - 1] > 0 and ib[HALVE - 1] > 0 and pb[-1] > 0 and ib[-1] > 0, (pb, ib)
        assert ta == tb
        gets = [o[0][0][off[tb]:off[tb + 1]] for o in ob]
        # the halving moved the target's leases off their fixed point (so the key set before it
        # must not serve after the capacity is back)
        assert any(not np.array_equal(gets[t], gets[HALVE - 1]) for t in range(HALVE, RESTORE + 3)), tb
        for t, (a, b) in enumerate(zip(oa, ob)):
            for x, y in zip(a[0], b[0]):
                assert x.tobytes() == y.tobytes(), f"step {t}: leases"
            for k in W.CFG_FIELDS:
                assert a[1][k].tobytes() == b[1][k].tobytes(), f"step {t}: template {k}"
            for k in COLS:
                assert a[2][k].tobytes() == b[2][k].tobytes(), f"step {t}: leaf {k}"
                assert a[3][k].tobytes() == b[3][k].tobytes(), f"step {t}: root {k}"
            assert a[4].tobytes() == b[4].tobytes(), f"step {t}: the root's verdict on the request"
    finally:
        for e in (la, ra, lb, rb):
            e.close()


def test_relayout_and_reload_start_without_keys(monkeypatch, store):
    """A store whose keys are valid is re-laid out (one resource grows by 64 rows: new work
    items), then replaced by another store of the same shape (other wants: a key kept from
    the old store would name rows that are no longer there).  Each time no key is valid or in
    use until a FIXED launch has rewritten them, and the two engines hold identical bits."""
    snap, under, over, learn, pexp = store
    P = Pair(monkeypatch, snap)
    try:
        for t in range(3):
            parts, items = P.tick(f"tick {t + 1}", 2 * t)
        assert parts > 0 and items >= len(under) - 1, (parts, items)

        sizes = np.diff(P.off)
        sizes[by_size(snap, under, 1000)] += 64
        new_off = np.concatenate([[0], np.cumsum(sizes)])
        P.both(lambda e: e.relayout(new_off))
        assert P.counts("re-layout")[1] == 0
        for t in range(3):
            now = NOW + (6 + 2 * t) * W.NS
            P.both(lambda e: e.apportion(now, writeback=True))
            assert_same_state(P.A, P.B, f"tick {t + 1} after the re-layout")
            got = P.counts(f"tick {t + 1} after the re-layout")
            assert (got[0] > 0) == (t == 2), (t, got)

        other, _, _ = make_store(seed=2)
        P.both(lambda e: e.load(other))
        assert P.counts("reload")[1] == 0
        P.host = copy_of(other)
        for t in range(3):
            got = P.tick(f"tick {t + 1} after the reload", 12 + 2 * t, oracle=t == 2)
            assert (got[0] > 0) == (t == 2), (t, got)
    finally:
        P.close()
