"""dm_keep_keys: with the mode on, a wants refresh without NaN starts no row
epoch; the refresh kernels' key-clearing builds (dm_update.hip) store an invalid key for
exactly the workgroup-bin resources in which a row changed its wants bits, every other key
stays in use, the density verification stays valid and the next tick stays in place.

Nothing a caller can read may depend on it.  Engine A runs with the mode off, engine B with
keep_keys(1): identical bits after every call and every tick, B against the oracle at each
event.  What differs is what the introspection calls say: dm_store_stats' "fixed_items" (the
valid keys in use: 0 in A after any refresh, down in B by the resources the refresh changed),
dm_plan_info's "fixed_parts" / "sweep_parts" (the form of the last tick) and
"kept_refreshes".

The store: a 40-row resource (small tiles) with three released rows and a 5,000-row resource
(the large chain), neither with a key; then two resources at each of 257, 512, 513, 1000,
1024, 1025, 2048, 2049 and 4096 rows, one under capacity (sum of wants <= C / 2: gets ==
wants in any order) and one over it with wants multiples of 2^-10 and C = 2^12 (every sum
exact).  So that the order of the refresh kernels' atomics cannot show, a refresh changes at
most one row per under-capacity resource and uses multiples of 2^-10 on the others.  The
oracle alone confirms that every under-capacity resource is a fixed point from tick 2 on (a
condition of the data): those hold a valid key once the keys engage.  An over-capacity one
may move by a rounding step per tick, and whether it does depends on the rounding of its
running sums, which the device keeps from tick to tick and the oracle's host copy adds up
anew.  So the resources that hold a valid key are read off engine A, the control: those of
the workgroup bins whose rows' has and whose sums A's last tick left bit for bit as they
were, which is what a key says (dm_device.h FixKey).  Every count of keys is exact against
that set."""
import numpy as np
import pytest

from doorman_amd import _lib
from doorman_amd import workloads as W
from oracle import oracle as O
from parity_util import assert_leases_match
from test_skip_unchanged_gpu import assert_same_state, copy_of, host_tick

pytestmark = pytest.mark.gpu

NOW = W.NOW_NS
EDGES = [257, 512, 513, 1000, 1024, 1025, 2048, 2049, 4096]
R_SMALL, R_LARGE = 0, 1
RELEASED_ROWS = (3, 17, 18)  # of the 40-row resource
COLS = ("has", "wants", "subclients", "expiry_ns")


def make_store(seed=5):
    """(snapshot, under-capacity resources, over-capacity resources)"""
    rng = np.random.default_rng(seed)
    sizes, kinds, caps, wants, under, over = [40, 5000], [3, 3], [100.0, 4096.0], [], [], []
    wants.append(rng.uniform(0.0, 1.0, 40) * (0.5 * 100.0 / 40))
    wants.append(np.round(rng.uniform(0.0, 4.0, 5000) * (4096.0 / 5000) * 1024.0) / 1024.0)
    for i, n in enumerate(EDGES):
        for j in range(2):
            r = len(sizes)
            sizes.append(n)
            kinds.append(2 + (i + j) % 2)
            if j == 0:
                C = 1000.0
                w = rng.uniform(0.0, 1.0, n) * (0.5 * C / n)
                under.append(r)
            else:
                C = 4096.0
                w = np.round(rng.uniform(0.0, 4.0, n) * (C / n) * 1024.0) / 1024.0
                over.append(r)
            caps.append(C)
            wants.append(w)
    wants = np.concatenate(wants)
    N = len(wants)
    cap_row = np.repeat(np.asarray(caps), sizes) / np.repeat(np.asarray(sizes, np.float64), sizes)
    has = rng.uniform(0.0, 0.4, N) * cap_row
    exp = NOW + rng.integers(30, 300, N, dtype=np.int64) * W.NS
    snap = W.make_snapshot(sizes, wants, has, np.ones(N, np.int64), exp, np.asarray(kinds, np.int32),
                           np.asarray(caps), lease_length_s=20, refresh_interval_s=5)
    free = np.asarray(RELEASED_ROWS)  # (the 40-row resource is the first)
    snap["wants"][free], snap["has"][free], snap["subclients"][free] = 0.0, 0.0, 0
    snap["expiry_ns"][free] = W.RELEASED
    W.add_store_sums(snap)
    return snap, under, over


def assert_same_store(A, B, label):
    """assert_same_state without the leases: after a call that is not a tick there are none."""
    sa, sb = A.read_store(), B.read_store()
    for k in COLS:
        np.testing.assert_array_equal(sa[k].view(np.int64), sb[k].view(np.int64), err_msg=f"{label}: {k}")
    ra, rb = A.resources(safe=False), B.resources(safe=False)  # (the safe capacity needs a tick's result)
    for k in ra:
        np.testing.assert_array_equal(ra[k].view(np.int64), rb[k].view(np.int64), err_msg=f"{label}: resources {k}")


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
    snap, under, over = make_store()
    host = copy_of(snap)
    host_tick(host, NOW)
    for t in (1, 2, 3):  # the data's condition: from tick 2 on the under-capacity resources stay as they are
        same = unchanged_by_tick(host, NOW + 2 * t * W.NS)
        assert same[under].all(), f"tick {t + 1}: {np.asarray(under)[~same[under]]}"
    return snap, under, over


class Pair:
    """Engine A (mode off) and engine B (keep_keys on) on the same store, and the oracle's
    host copy of it."""

    def __init__(self, snap, under=(), keep=True):
        from doorman_amd.engine import Engine
        self.A, self.B = Engine(0), Engine(0)
        self.host = copy_of(snap)
        self.off = np.asarray(snap["seg_off"])
        self.keyed = np.diff(self.off) > 256  # the workgroup bins' resources ...
        self.keyed &= np.diff(self.off) <= 4096  # ... (257-4096 rows): those with a key
        self.under = set(r for r in under if self.keyed[r])  # ... and those that must hold a valid one
        self.fixed = np.zeros(len(self.off) - 1, bool)  # A's last writeback tick left the resource as it was
        try:
            if keep:
                self.B.keep_keys(True)
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

    def same(self, label, leases=True):
        (assert_same_state if leases else assert_same_store)(self.A, self.B, label)

    def info(self, e):
        p, s = e.plan_info(), e.store_stats()
        return {"parts": p["fixed_parts"], "sweep": p["sweep_parts"], "items": s["fixed_items"],
                "kept": p["kept_refreshes"], "inplace": p["wb_inplace"]}

    def tick(self, label, dt, oracle=True, **kw):
        """One tick of both engines at NOW + dt s (writeback unless said otherwise): identical
        bits after it, B's leases against the oracle's.  A writeback tick advances the host
        copy.  Returns (A's info, B's info)."""
        now = NOW + dt * W.NS
        kw.setdefault("writeback", True)
        # (in place by request: with a large resource in the store an "auto" tick may take the
        # speculative chain, which writes the alternate column, and no key is ever set)
        kw.setdefault("wb_columns", "inplace")
        before = self.control()
        self.both(lambda e: e.apportion(now, **kw))
        self.same(label)
        if kw["writeback"]:
            after = self.control()
            moved = np.add.reduceat((before[0] != after[0]).astype(np.int64), self.off[:-1])  # (no resource is empty)
            self.fixed = (moved == 0) & (before[1] == after[1]).all(axis=0)
        if oracle:
            assert_leases_match(self.host, *self.B.leases(), O.apportion(self.host, now), label)
        if kw["writeback"]:
            host_tick(self.host, now)
        return self.info(self.A), self.info(self.B)

    def control(self):
        """Engine A's has column and its running sums (one row per sum), as bits."""
        res = self.A.resources(safe=False)
        sums = np.stack([np.ascontiguousarray(res[k]).view(np.int64) for k in ("count", "sum_has", "sum_wants")])
        return self.A.read_store()["has"].view(np.int64).copy(), sums

    def valid(self):
        """The resources that hold a valid key after a tick with keys in use."""
        return self.fixed & self.keyed

    def engage(self):
        """Three writeback ticks: hints, keys written, keys used.  Returns B's valid keys: the
        resources the third tick left as they were, among them every under-capacity one."""
        for t in range(3):
            a, b = self.tick(f"tick {t + 1}", 2 * t, oracle=t == 2)
        assert a["parts"] > 0 and b["parts"] > 0 and b["sweep"] > 0, (a, b)
        assert all(self.fixed[r] for r in self.under), self.fixed
        assert a["items"] == b["items"] == int(self.valid().sum()), (a, b, self.fixed)
        return b["items"]

    def refresh(self, rows, vals, label, mask=False):
        """One wants refresh in both engines and on the host copy; identical bits after it.
        Returns the resources in which a live row's wants bits changed."""
        rows, vals = np.asarray(rows, np.int64), np.asarray(vals, np.float64)
        if mask:
            order = np.argsort(rows)
            rows, vals = rows[order], vals[order]
            words = np.zeros((len(self.host["wants"]) + 63) // 64, np.uint64)
            np.bitwise_or.at(words, rows // 64, np.uint64(1) << (rows % 64).astype(np.uint64))
            self.both(lambda e: e.update_wants_mask(words, vals))
        else:
            self.both(lambda e: e.update_wants(rows, vals))
        live = self.host["expiry_ns"][rows] != W.RELEASED
        moved = live & (self.host["wants"][rows].view(np.int64) != vals.view(np.int64))
        self.host["wants"][rows[live]] = vals[live]
        W.add_store_sums(self.host)
        self.same(label, leases=False)
        return set(int(r) for r in np.searchsorted(self.off, rows[moved], side="right") - 1)

    def check_drop(self, items, changed, label):
        """B's valid keys after a kept refresh that changed these resources, `items` before it:
        exactly one less for every changed resource that held one.  A's: none in use.
        Returns the drop."""
        drop = sum(1 for r in changed if self.valid()[r])
        a, b = self.info(self.A), self.info(self.B)
        assert b["items"] == items - drop and a["items"] == 0, (label, items, drop, sorted(changed), a, b)
        return drop

    def row(self, r, i):
        return int(self.off[r] + (i if i >= 0 else self.off[r + 1] - self.off[r] + i))

    def new_value(self, row, dyadic):
        w = self.host["wants"][row]
        return w + 1.0 / 1024 if dyadic else w * 0.5 + 1.0 / 1024

    def settle(self, label, dt, items):
        """Two ticks after a kept refresh that left `items` valid keys: the sweep with the
        cleared keys' rows read, then every under-capacity resource at its new fixed point.
        After each, B's valid keys are exactly the resources the tick left as they were."""
        a, b = self.tick(f"{label}: next tick", dt)
        assert b["parts"] > 0 and b["sweep"] > 0 and b["inplace"] == 1 and a["parts"] == 0, (a, b)
        assert b["items"] == int(self.valid().sum()), (b, self.fixed)
        a, b = self.tick(f"{label}: the tick after", dt + 2)
        assert b["parts"] > 0 and b["items"] == int(self.valid().sum()), (b, items, self.fixed)
        assert all(self.fixed[r] for r in self.under), self.fixed


def by_size(snap, group, n):
    off = snap["seg_off"]
    return next(r for r in group if off[r + 1] - off[r] == n)


def test_one_row_of_one_fixed_resource(store):
    """The refresh of one row (index 70 of 1000) clears one key in B and ends every key's
    use in A; B's next tick is the sweep, A's runs without keys; the tick after, B's keys are
    all back."""
    snap, under, over = store
    P = Pair(snap, under)
    try:
        items = P.engage()
        r = by_size(snap, under, 1000)
        row = P.row(r, 70)
        changed = P.refresh([row], [P.new_value(row, False)], "refresh")
        assert changed == {r}
        assert P.check_drop(items, changed, "refresh") == 1
        a, b = P.info(P.A), P.info(P.B)
        assert b["kept"] == 1 and a["kept"] == 0, (a, b)
        a, b = P.tick("tick 4", 6)
        assert b["parts"] > 0 and b["sweep"] > 0 and a["parts"] == 0 and a["sweep"] == 0, (a, b)
        a, b = P.tick("tick 5", 8)
        assert b["items"] == items and b["parts"] > 0, (a, b)
        assert b["kept"] == 1 and a["kept"] == 0
    finally:
        P.close()


def test_the_same_bits_clear_no_key(store):
    """200 rows across six resources re-send their stored values: no key is cleared, and B's
    next tick has the form of its last."""
    snap, under, over = store
    P = Pair(snap, under)
    try:
        items = P.engage()
        before = P.info(P.B)
        rs = [by_size(snap, under, 257), by_size(snap, over, 512), by_size(snap, under, 1024),
              by_size(snap, over, 2048), by_size(snap, under, 4096), by_size(snap, over, 4096)]
        rows = np.concatenate([P.off[r] + np.arange(0, 34 * 7, 7)[:34 if k < 4 else 32] for k, r in enumerate(rs)])
        assert len(rows) == 200
        assert P.refresh(rows, P.host["wants"][rows].copy(), "list") == set()
        assert P.info(P.B)["items"] == items and P.info(P.A)["items"] == 0
        assert P.refresh(rows, P.host["wants"][rows].copy(), "mask", mask=True) == set()
        assert P.info(P.B)["items"] == items
        a, b = P.tick("tick 4", 6)
        assert {k: b[k] for k in ("parts", "sweep", "items")} == {k: before[k] for k in ("parts", "sweep", "items")}
        assert b["kept"] == 2 and a["parts"] == 0
    finally:
        P.close()


def test_row_list_edges(store):
    """One call of two waves.  The first 64 entries cycle over ten resources (more than 8
    runs: wave_seg_add's per-lane path) with changed and unchanged rows mixed, among them the
    first and the last row of a resource, a released row, and rows of the 40-row and the
    5,000-row resource; the next 64 make four runs, in one of which only a lane that is not
    the run's head changes, and one of which changes nothing."""
    snap, under, over = store
    P = Pair(snap, under)
    try:
        items = P.engage()
        ten = [R_SMALL, R_LARGE] + [by_size(snap, g, n) for n in (257, 513, 1025, 2049) for g in (under, over)]
        rows, vals = [], []

        def add(row, change, dyadic):
            rows.append(row)
            vals.append(P.new_value(row, dyadic) if change else P.host["wants"][row])

        changed_under = set()
        for k in range(64):  # entry k: resource k % 10, its (k // 10)-th pick
            r, pick = ten[k % 10], k // 10
            dy = r not in under or r == R_SMALL
            if r == R_SMALL:
                i = (RELEASED_ROWS[0], 0, 39, 5, 6, 7, 8)[pick]  # a released row: nothing changes
                add(P.row(r, i), pick in (0, 2), False)
            elif r in under:  # at most one changed row per under-capacity resource
                i = (0, -1, 100, 130, 131, 200, 201)[pick]
                want = pick == (1 if r == ten[2] else 3) and r != ten[8]  # (ten[8]: every row unchanged)
                add(P.row(r, i), want, False)
                if want:
                    changed_under.add(r)
            else:
                i = (0, -1, 64, 65, 127, 128, 129)[pick]
                add(P.row(r, i), pick % 2 == 1 and r != ten[9], dy)  # (ten[9]: every row unchanged)
        assert len(rows) == 64
        runs = [(by_size(snap, under, 2048), 16, {9}), (by_size(snap, over, 2048), 16, {0, 15}),
                (by_size(snap, under, 4096), 16, set()), (by_size(snap, over, 1024), 16, {5, 6})]
        for r, n, chg in runs:
            for i in range(n):
                add(P.row(r, 300 + i), i in chg, r not in under)
        assert len(set(rows)) == 128
        changed = P.refresh(rows, vals, "row list")
        assert changed_under <= changed and ten[8] not in changed and ten[9] not in changed
        assert runs[0][0] in changed and runs[2][0] not in changed and R_SMALL in changed and R_LARGE in changed
        assert np.array_equal(P.B.read_store()["wants"][list(RELEASED_ROWS)], np.zeros(3))
        drop = P.check_drop(items, changed, "row list")  # (exact: the changed resources that held a key)
        assert drop >= len(changed_under) + 1 >= 4
        P.settle("row list", 6, items - drop)
    finally:
        P.close()


def test_mask_edges(store):
    """update_wants_mask: a word that straddles the two 257-row resources in which only the
    second one's row changes; sixteen consecutive words of one wave inside one resource,
    changed only in the last; a last wave of fewer than 16 words with a change; a mask bit on
    a released row."""
    snap, under, over = store
    P = Pair(snap, under)
    try:
        items = P.engage()
        N = len(P.host["wants"])
        nwords = (N + 63) // 64
        assert nwords % 16 not in (0,), nwords  # the last wave holds fewer than 16 words
        rows, vals = [], []

        def add(row, change, dyadic):
            rows.append(row)
            vals.append(P.new_value(row, dyadic) if change else P.host["wants"][row])

        r0, r1 = by_size(snap, under, 257), by_size(snap, over, 257)
        assert r1 == r0 + 1 and P.off[r1] % 64 not in (0, 63)  # one word holds rows of both
        add(P.row(r0, -1), False, False)
        add(P.row(r1, 1), True, True)
        assert rows[0] // 64 == rows[1] // 64
        big = by_size(snap, under, 4096)
        w0 = -(-P.off[big] // 1024) * 16  # the first wave whose sixteen words lie inside it
        assert P.off[big] <= 64 * w0 and 64 * (w0 + 16) <= P.off[big + 1]
        for q in range(16):
            add(64 * (w0 + q) + 3 * q, q == 15, False)
        last = by_size(snap, over, 4096)
        tail = 64 * (nwords - nwords % 16) + 70  # in the last wave
        assert P.off[last] <= tail < N and last == len(P.off) - 2
        add(tail, True, True)
        add(P.row(R_SMALL, RELEASED_ROWS[1]), True, False)  # a released row: nothing changes
        add(P.row(R_SMALL, 20), True, False)
        changed = P.refresh(rows, vals, "mask", mask=True)
        assert changed == {r1, big, last, R_SMALL}
        assert P.B.read_store()["wants"][P.row(R_SMALL, RELEASED_ROWS[1])] == 0.0
        drop = P.check_drop(items, changed, "mask")
        assert drop >= 1 and big in P.under
        P.settle("mask", 6, items - drop)
    finally:
        P.close()


def test_nan_and_rejection(store):
    """A NaN refresh ends every key's use in B as in A (k_general decides the resource);
    repaired, the keys come back.  A call with a row twice is refused by both with the
    stores as they were."""
    snap, under, over = store
    P = Pair(snap, under)
    try:
        items = P.engage()
        r = next(x for x in under if snap["kind"][x] == W.FAIR_SHARE)
        row = P.row(r, 5)
        keep = P.host["wants"][row]
        P.refresh([row], [np.nan], "NaN")
        assert P.info(P.B)["items"] == 0 and P.info(P.B)["kept"] == 0
        P.both(lambda e: e.set_profiling(True))
        a, b = P.tick("tick 4 (NaN wants)", 6, oracle=False)
        assert a["parts"] == 0 and b["parts"] == 0
        assert "general" in P.A.kernel_times() and "general" in P.B.kernel_times()
        P.refresh([row], [keep], "repair")
        assert P.info(P.B)["kept"] == 1
        for t in range(4):
            a, b = P.tick(f"tick {5 + t}", 8 + 2 * t, oracle=t == 3)
        assert b["parts"] > 0 and b["items"] >= len(P.under) - 1, b

        before = P.B.read_store()
        for e in (P.A, P.B):
            with pytest.raises(_lib.DmError) as err:
                e.update_wants([row, row + 1, row], [1.0, 2.0, 3.0])
            assert err.value.code == _lib.DM_E_INVAL
        P.same("after the refused call", leases=False)
        assert np.array_equal(P.B.read_store()["wants"].view(np.int64), before["wants"].view(np.int64))
        assert P.info(P.B)["kept"] == 1 and P.info(P.B)["items"] == 0  # a refused call starts a row epoch, as ever
        P.tick("tick 9", 16)
    finally:
        P.close()


def test_around_other_events(store):
    """Kept refreshes before the keys engage, before a release and an arrival, before ticks
    that are not FIXED (non-writeback, recompute, alternate column), with the mode switched
    off mid-run, before load_config halves a capacity, and before a re-layout."""
    snap, under, over = store
    P = Pair(snap, under)
    try:
        r = by_size(snap, under, 1000)
        row = P.row(r, 70)
        P.tick("tick 1", 0)
        P.refresh([row], [P.new_value(row, False)], "before the keys engage")
        assert P.info(P.B) == {**P.info(P.B), "items": 0, "kept": 1}
        P.tick("tick 2", 2)
        a, b = P.tick("tick 3", 4)
        assert b["parts"] > 0 and a["parts"] == 0, (a, b)  # B kept its epoch: hints and the density check hold
        a, b = P.tick("tick 4", 6)
        assert len(P.under) <= b["items"] == a["items"], (a, b)

        P.refresh([row], [P.new_value(row, False)], "before a release")
        freed = np.array([P.row(by_size(snap, under, 1024), 700)], np.int64)
        P.both(lambda e: e.release(freed))
        P.host["has"][freed], P.host["wants"][freed], P.host["subclients"][freed] = 0.0, 0.0, 0
        P.host["expiry_ns"][freed] = W.RELEASED
        W.add_store_sums(P.host)
        P.same("release", leases=False)
        assert P.info(P.B)["items"] == 0  # every other writer ends the keys' use
        P.tick("tick 5 (release)", 8)
        ne = NOW + 112 * W.NS
        P.both(lambda e: e.upsert(freed, np.zeros(1), np.full(1, 0.125), np.ones(1, np.int64), np.full(1, ne)))
        P.host["has"][freed], P.host["wants"][freed], P.host["subclients"][freed] = 0.0, 0.125, 1
        P.host["expiry_ns"][freed] = ne
        W.add_store_sums(P.host)
        P.tick("tick 6 (arrival)", 10)
        for t in range(3):
            a, b = P.tick(f"tick {7 + t}", 12 + 2 * t, oracle=t == 2)
        assert b["parts"] > 0 and a["parts"] > 0, (a, b)

        dt = 18
        for what, kw in (("no writeback", {"writeback": False}), ("recompute", {"recompute": True}),
                         ("alternate column", {"wb_columns": "alternate"})):
            P.refresh([row], [P.new_value(row, False)], f"before the {what} tick")
            a, b = P.tick(f"{what} tick", dt, **kw)
            assert b["parts"] == 0 and b["items"] == 0, (what, b)
            for t in range(3):
                a, b = P.tick(f"tick {t + 1} after the {what} tick", dt + 2 + 2 * t, oracle=t == 2)
            assert b["parts"] > 0, (what, b)
            dt += 8

        kept = P.info(P.B)["kept"]
        P.B.keep_keys(False)
        P.refresh([row], [P.new_value(row, False)], "mode off again")
        assert P.info(P.B)["items"] == 0 and P.info(P.B)["kept"] == kept
        a, b = P.tick("tick after the switch", dt)
        assert b["parts"] == 0
        P.B.keep_keys(True)
        for t in range(3):
            a, b = P.tick(f"tick {t + 2} after the switch", dt + 2 + 2 * t, oracle=t == 2)
        assert b["parts"] > 0 and b["items"] > 0
        dt += 8

        P.refresh([row], [P.new_value(row, False)], "before load_config")
        ro = by_size(snap, over, 1024)
        P.host["capacity"] = P.host["capacity"].copy()
        P.host["capacity"][ro] *= 0.5
        P.both(lambda e: e.load_config(P.host))
        assert P.info(P.B)["items"] == 0
        for t in range(3):
            a, b = P.tick(f"tick {t + 1} after load_config", dt + 2 * t, oracle=t != 1)
        assert b["parts"] > 0
        dt += 6

        P.refresh([row], [P.new_value(row, False)], "before the re-layout")
        sizes = np.diff(P.off)
        sizes[r] += 64
        new_off = np.concatenate([[0], np.cumsum(sizes)])
        P.both(lambda e: e.relayout(new_off))
        P.same("re-layout", leases=False)
        assert P.info(P.B)["items"] == 0
        for t in range(3):
            now = NOW + (dt + 2 * t) * W.NS
            P.both(lambda e: e.apportion(now, writeback=True, wb_columns="inplace"))
            P.same(f"tick {t + 1} after the re-layout")
        assert P.info(P.B)["parts"] > 0 and P.info(P.A)["parts"] > 0
        row2 = int(new_off[r] + 70)
        P.both(lambda e: e.update_wants(np.array([row2], np.int64), np.array([0.25])))
        P.same("refresh after the re-layout", leases=False)
        assert P.info(P.B)["items"] > 0 and P.info(P.A)["items"] == 0
        now = NOW + (dt + 6) * W.NS
        P.both(lambda e: e.apportion(now, writeback=True, wb_columns="inplace"))
        P.same("tick after it")
        assert P.info(P.B)["sweep"] > 0
    finally:
        P.close()


def test_stream_parts_stay_dense_alone():
    """A store whose only work class is one workgroup bin runs it in two stream parts, whose
    verified form is the dense kernel alone with the guard.  Kept refreshes between ten
    ticks keep B in that form (no rest launch after its density check; A, starting a row
    epoch each time, launches its rest kernel again), the guard never trips, and both match
    each other bit for bit and the oracle on every tick."""
    rng = np.random.default_rng(9)
    R = 4200
    sizes = rng.integers(257, 300, R)
    N = int(sizes.sum())
    wants = rng.uniform(0.0, 1.0, N) * np.repeat(0.5 * 1000.0 / sizes, sizes)  # under capacity: gets == wants
    snap = W.make_snapshot(sizes, wants, np.zeros(N), 1, np.full(N, NOW + 600 * W.NS),
                           np.where(np.arange(R) % 2, W.FAIR_SHARE, W.PROPORTIONAL_SHARE).astype(np.int32), 1000.0,
                           lease_length_s=60)
    P = Pair(snap)
    try:
        assert P.B.plan_info()["stream_parts"] == 2 and P.A.plan_info()["stream_parts"] == 2
        P.both(lambda e: e.set_profiling(True))
        rest = lambda e: e.kernel_times().get("block128x4_rest", (0, 0.0))[0]
        seen = []
        for t in range(10):
            if t >= 1:  # one row in each of 50 resources, by list or by mask
                rs = rng.choice(R, 50, replace=False)
                rows = P.off[rs] + rng.integers(0, 257, 50)
                P.refresh(rows, P.host["wants"][rows] * 0.5 + 1.0 / 1024, f"refresh {t}", mask=t % 2 == 0)
            P.tick(f"tick {t + 1}", 2 * t)
            assert not P.A.store_lost() and not P.B.store_lost()
            seen.append((rest(P.A), rest(P.B)))
        assert P.info(P.B)["kept"] == 9 and P.info(P.A)["kept"] == 0
        # B: verified after its second writeback tick, and never again a rest launch; A: one per part and tick
        assert seen[-1][1] == seen[2][1], seen
        assert seen[-1][0] > seen[2][0], seen
    finally:
        P.close()
