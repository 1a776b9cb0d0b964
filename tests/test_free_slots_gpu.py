"""dm_keep_keys' DM_KEEP_FREE_SLOTS: with bit 4 set a dense workgroup-bin
resource that holds released rows (free slots), with no pending arrival and a live row, is an
item of the steady, FIXED, sweep and cycle forms like any other (the kernels' masked builds:
dm_tick_masked.hip, dm_tick_group.h group_segment kMasked): it keeps a fixed-point key and is
skipped at its fixed point or in its proven two-tick cycle.

As in tests/test_keep_keys_gpu.py and tests/test_keep_updates_gpu.py, whose store, Pair and
Track these tests import, nothing a caller can read may depend on the mode: engine A runs mode
0 and engine B mode 7, and after every call and every tick the two hold identical bits, B's
leases match the oracle's, and the oracle's host copy takes the same update.

What differs is the introspection: dm_plan_info's "fixed_parts", "sweep_parts", "cycle_parts"
and "masked_parts" (the form of the last tick) and dm_store_stats' "fixed_items", which after
every tick in which all four workgroup bins ran with keys in use must be exactly the expected
set (Free.expected): the resources A's last tick left bit for bit, holders of released rows
among them, without those whose live rows do not share one subclient count, those with no live
row, and those into which a row arrived since the tick before (the rest kernel absorbed it).

The rest queue's count is not part of the C-ABI.  That the masked build, not the rest kernel,
read a resource's rows shows in its key: the rest kernel keeps none, so a holder of a released
row that A's tick left as it was holds a key after that very tick only if the masked build
decided it.
"""
import numpy as np
import pytest

from doorman_amd import _lib
from doorman_amd import workloads as W
from test_keep_keys_gpu import NOW, Pair, by_size, make_store, store  # noqa: F401 (store: a fixture)
from test_keep_updates_gpu import NBINS, Track

pytestmark = pytest.mark.gpu

MODE3 = _lib.DM_KEEP_REFRESH | _lib.DM_KEEP_UPDATES
MODE7 = MODE3 | _lib.DM_KEEP_FREE_SLOTS


def masked(e):
    return e.plan_info()["masked_parts"]


class Free(Track):
    """Track with B at `mode` (7 unless said otherwise) and the expected keys of that mode."""

    def __init__(self, snap, under=(), mode=MODE7):
        super().__init__(snap, under)
        self.mode = mode
        self.P.B.keep_keys(mode)
        self.arrived = set()  # resources into which a row arrived since the last tick

    def expected(self):
        if not self.mode & _lib.DM_KEEP_FREE_SLOTS:
            return super().expected()
        P, h = self.P, self.P.host
        live = h["expiry_ns"] != W.RELEASED
        keys = P.valid().copy()
        for r in np.flatnonzero(keys):
            lo, hi = P.off[r], P.off[r + 1]
            sub = h["subclients"][lo:hi][live[lo:hi]]
            if len(sub) == 0 or (sub != sub[0]).any():
                keys[r] = False
        keys[list(self.arrived)] = False
        return keys

    def tick(self, label, **kw):
        out = super().tick(label, **kw)
        self.arrived = set()
        return out

    def engage(self, label="engage", ticks=5, want_masked=NBINS):
        for t in range(ticks):
            a, b = self.tick(f"{label}: tick {t + 1}")
            if b["parts"] == NBINS and b["sweep"] == NBINS and masked(self.P.B) == want_masked:
                return b["items"]
        raise AssertionError((label, a, b, masked(self.P.B)))

    def holders(self):
        """Per resource: it holds a released row and a live one."""
        P, h = self.P, self.P.host
        rel = h["expiry_ns"] == W.RELEASED
        n = np.add.reduceat(rel.astype(np.int64), P.off[:-1])
        return (n > 0) & (n < np.diff(P.off))

    def release_each(self, rows_of, label):
        """One release call per resource and wave: each call is one run of one wave, so the
        order of the update kernel's atomics cannot show in the sums."""
        for r, idx in rows_of:
            rows = [self.P.row(r, i) for i in idx]
            assert len(rows) <= 64
            self.release(rows, f"{label}: resource {r}")

    def arrive(self, r, i, label):
        """A narrow arrival into released row i of resource r, with the followers' subclient
        count and the implied expiry (the next tick's time plus the lease length)."""
        P = self.P
        row = np.array([P.row(r, i)], np.int64)
        assert P.host["expiry_ns"][row[0]] == W.RELEASED
        now = NOW + self.dt * W.NS
        before = self.stats()
        had = self.items()
        held = self.keys is not None and bool(self.keys[r])
        P.both(lambda e: e.apply(upsert=(row, None, np.full(1, 0.125), np.ones(1, np.int32), None), now_ns=now))
        self.host_upsert(row, 0.0, 0.125, 1, now + 20 * W.NS)
        P.same(label, leases=False)
        self.touched.add(r)
        self.arrived.add(r)
        assert self.stats()["kept_batches"] == before["kept_batches"] + 1, label
        assert self.items() == had - int(held), (label, had, held)  # the key is cleared
        if self.keys is not None:
            self.keys[r] = False


def edge_rows(n):
    """The first row, the first lane of the second wave, rows of the last slot of every shape
    (k = R - 1 for 128 x 4, x 8 and 64 / 256 x 16 where the resource reaches it) and the last row."""
    return sorted({0, 64, (3 * n) // 4, (7 * n) // 8, (15 * n) // 16, n - 2, n - 1})


def free_slot_plan(snap, under, over):
    """Releases in at least half of every bin's resources, under- and over-capacity ones among
    them; in two of them a whole 64-row run (a call of its own)."""
    picks = [(under, 257), (over, 512), (over, 513), (under, 1000), (over, 1024), (under, 1025), (over, 2048),
             (over, 2049), (under, 4096)]
    plan = []
    for group, n in picks:
        plan.append((by_size(snap, group, n), edge_rows(n)))
    plan.append((by_size(snap, under, 257), list(range(128, 192))))
    plan.append((by_size(snap, under, 4096), list(range(1024, 1088))))
    return plan


@pytest.fixture
def free(store):
    snap, under, over = store
    T = Free(snap, under)
    try:
        yield T, snap, under, over
    finally:
        T.close()


def test_free_slots_above_the_quarter_bound(free):
    """(Fails without the feature: such parts ran as with the bit clear.)  Released rows in half
    of every bin's resources before the keys engage: within five writeback ticks in place all
    four parts run FIXED as the sweep, in the masked builds, and B's valid keys are exactly the
    resources A's last tick left bit for bit, the holders of released rows included."""
    T, snap, under, over = free
    P = T.P
    T.release_each(free_slot_plan(snap, under, over), "free slots")
    hold = T.holders()
    for b_lo, b_hi in ((257, 512), (513, 1024), (1025, 2048), (2049, 4096)):
        sz = np.diff(P.off)
        in_bin = (sz >= b_lo) & (sz <= b_hi)
        assert 2 * int((hold & in_bin).sum()) >= int(in_bin.sum()), (b_lo, hold[in_bin])
    items = T.engage()  # (tick asserts: fixed_items == the expected set, exactly)
    a, b = P.info(P.A), P.info(P.B)
    assert b["parts"] == NBINS and b["sweep"] == NBINS and masked(P.B) == NBINS and b["inplace"] == 1, (a, b)
    assert a["parts"] == 0 and masked(P.A) == 0, a  # the control: above the quarter bound, as ever
    kept = T.keys & hold
    assert kept.sum() >= 4 and all(T.keys[r] for r in P.under), (T.keys, hold)  # under-capacity holders are fixed points
    assert items == int(T.keys.sum())
    for t in range(2):
        T.tick(f"steady tick {t + 1}")
    assert masked(P.B) == NBINS and not P.B.store_lost() and not P.A.store_lost()


def test_mode_3_is_unchanged_on_the_same_store(free):
    """The same store under mode 3: no masked build is ever launched, and no holder of a
    released row holds a key (the parts are above the quarter bound: they run without keys)."""
    T, snap, under, over = free
    P = T.P
    T.mode = MODE3
    P.B.keep_keys(MODE3)
    T.release_each(free_slot_plan(snap, under, over), "free slots")
    for t in range(5):
        a, b = T.tick(f"tick {t + 1}")
        assert masked(P.B) == 0 and masked(P.A) == 0, (t, a, b)
        bound = int(Track.expected(T).sum())  # (mode 3's set: without every holder of a released row)
        assert b["items"] <= bound, (t, b, bound)
        assert b["items"] == bound or b["parts"] < NBINS, (t, b, bound)
    assert T.stats()["mode"] == 3


def test_a_kept_release(free):
    """Under mode 7, one row released in a keyed resource that had no free slot: the key count
    drops by one; the next tick decides the resource in the masked build (its key is back
    after that very tick, which the rest kernel never does), and stays."""
    T, snap, under, over = free
    P = T.P
    items = T.engage(want_masked=0)  # no free slot in the workgroup bins: today's kernels
    r = by_size(snap, under, 1024)
    assert T.keys[r]
    assert T.release([P.row(r, 700)], "release") == 1
    assert T.items() == items - 1
    a, b = T.tick("the next tick")
    assert b["parts"] == NBINS and b["sweep"] == NBINS and a["parts"] == 0, (a, b)
    assert masked(P.B) >= 1, P.B.plan_info()
    assert T.keys[r] and all(T.keys[x] for x in P.under), T.keys  # decided by the masked build: keyed at once
    for t in range(3):
        a, b = T.tick(f"tick {t + 2} after the release")
        assert b["parts"] == NBINS and b["sweep"] == NBINS and masked(P.B) == 1, (a, b, P.B.plan_info())
    assert T.keys[r] and T.holders()[r] and all(T.keys[x] for x in P.under), T.keys
    assert not P.B.store_lost()


def test_an_arrival_into_a_free_slot(free):
    """A keyed resource with one free slot takes an arrival into it (the followers' count, the
    implied expiry): its key is cleared, the rest kernel absorbs the arrival, and within four
    ticks the resource is keyed again without a mask bit.  In the 257-512-row bin (the arrival
    nibble shares the mask byte) and in the 1025-2048-row bin."""
    T, snap, under, over = free
    P = T.P
    T.engage(want_masked=0)
    for n, i in ((512, 391), (2048, 1800)):
        r = by_size(snap, under, n)
        assert T.release([P.row(r, i)], f"{n}: release") == 1
        T.engage(f"{n}: after the release", ticks=4, want_masked=1)
        assert T.keys[r] and T.holders()[r], (n, T.keys)
        dense = P.B.store_stats()["dense_resources"]
        T.arrive(r, i, f"{n}: arrival")
        a, b = T.tick(f"{n}: tick that absorbs the arrival")
        assert not T.keys[r] if T.keys is not None else True
        assert P.B.store_stats()["dense_resources"] == dense  # the state stayed dense throughout
        T.engage(f"{n}: after the arrival", ticks=4, want_masked=0)
        assert T.keys[r] and not T.holders()[r], (n, T.keys)
        assert (P.host["expiry_ns"][P.off[r]:P.off[r + 1]] != W.RELEASED).all()
    assert not P.B.store_lost()


def test_a_lapse(store):
    """A resource on a 3 s lease with a free slot, keyed, is ticked past its followers' expiry:
    the masked build hands it to the rest kernel, which releases every row.  From then on it
    has no live row, is handed over on every tick and never holds a key; the other keys stay."""
    snap, under, over = store
    snap = dict(snap)
    r = by_size(snap, under, 1000)
    snap["lease_length_s"] = np.array(snap["lease_length_s"]).copy()
    snap["lease_length_s"][r] = 3
    T = Free(snap, under)
    P = T.P
    try:
        T.engage(want_masked=0)
        assert T.release([P.row(r, 70)], "release") == 1
        T.engage("after the release", ticks=4, want_masked=1)
        assert T.keys[r] and T.holders()[r]
        T.dt += 2  # 4 s after the last tick: past its follow_exp alone
        a, b = T.tick("the lapse")
        lo, hi = P.off[r], P.off[r + 1]
        assert (P.host["expiry_ns"][lo:hi] == W.RELEASED).all()
        gets, exp = P.B.leases()
        assert not gets[lo:hi].any() and (exp[lo:hi] == W.RELEASED).all()
        assert (np.delete(P.host["expiry_ns"], np.arange(lo, hi)) != W.RELEASED).sum() > 0
        for t in range(4):
            a, b = T.tick(f"tick {t + 1} after the lapse")
            assert b["parts"] == NBINS and not T.keys[r], (t, a, b)  # (tick asserts the exact set)
        assert all(T.keys[x] for x in P.under if x != r) and masked(P.B) == 1, (T.keys, P.B.plan_info())
        assert not P.B.store_lost()
    finally:
        T.close()


def test_the_cycle_form(monkeypatch):
    """Oversubscribed FairShare resources of 1000 rows, eight of twelve with one free slot, on
    the alternate column: B runs the cycle form in its masked builds, and its keys in state 2
    are exactly the resources whose state repeats after two ticks on the control engine,
    holders of a free slot among them.  A row released while the other column still held its
    old value reads +0.0 from both columns (the has column after each of two ticks)."""
    for k in ("DM_FIXED", "DM_SWEEP", "DM_STEADY", "DM_CYCLE"):
        monkeypatch.delenv(k, raising=False)
    snap = W.uniform_range(12, 1000, 0, 12, seed=3)
    P = Pair(snap, keep=False)
    try:
        P.B.keep_keys(MODE7)
        off = P.off
        dt = 0
        for t in range(2):  # both columns hold granted values
            P.tick(f"tick {t + 1}", dt, wb_columns="alternate")
            dt += 2
        rows = np.array([P.row(r, 100 + 37 * r) for r in range(8)], np.int64)
        assert (P.B.read_store()["has"][rows] != 0.0).all()
        for row in rows:  # one call per resource
            P.both(lambda e: e.release(np.array([row], np.int64)))
        h = P.host
        h["has"][rows], h["wants"][rows], h["subclients"][rows] = 0.0, 0.0, 0
        h["expiry_ns"][rows] = W.RELEASED
        W.add_store_sums(h)
        P.same("releases", leases=False)
        st = {}
        for t in range(3, 15):
            P.tick(f"tick {t}", dt, wb_columns="alternate", oracle=t in (3, 4, 14))
            dt += 2
            if t in (3, 4):
                assert (P.B.read_store()["has"][rows].view(np.int64) == 0).all(), t
                assert (P.B.leases()[0][rows].view(np.int64) == 0).all(), t
            st[t] = (P.A.read_store()["has"].view(np.int64).copy(), P.A.resources()["sum_has"].view(np.int64).copy())
        per = lambda same: np.array([same[off[r]:off[r + 1]].all() for r in range(len(off) - 1)])
        back = per(st[12][0] == st[14][0]) & (st[12][1] == st[14][1])
        info, stats = P.B.plan_info(), P.B.store_stats()
        print(f"state repeats after two ticks: {np.flatnonzero(back)}; B: {info['cycle_parts']} cycle parts, "
              f"{info['masked_parts']} masked, {stats['fixed_items']} keys in state 2")
        assert info["cycle_parts"] == 1 and info["masked_parts"] == 1, info
        assert P.A.plan_info()["masked_parts"] == 0
        assert stats["fixed_items"] == int(back.sum()), (stats, back)
        assert back[:8].sum() > 0, back  # holders of a free slot in a proven cycle
        assert (P.B.read_store()["has"][rows].view(np.int64) == 0).all()
        assert not P.B.store_lost()
    finally:
        P.close()


def test_ticks_that_end_and_restore_the_keys(free):
    """A non-writeback tick and a recompute tick between FIXED ticks of a store with free slots
    end the keys' use and the following ticks restore it, as without free slots."""
    T, snap, under, over = free
    P = T.P
    T.release_each(free_slot_plan(snap, under, over), "free slots")
    T.engage()
    for what, kw in (("no writeback", {"writeback": False}), ("recompute", {"recompute": True})):
        a, b = T.tick(f"{what} tick", **kw)
        assert b["parts"] == 0 and b["items"] == 0, (what, b)
        assert masked(P.B) == (NBINS if what == "no writeback" else 0), (what, P.B.plan_info())
        T.engage(f"after the {what} tick", ticks=4)
        assert all(T.keys[x] for x in P.under), (what, T.keys)
    assert not P.B.store_lost()
