"""dm_keep_keys' DM_KEEP_UPDATES: with bit 2 set, dm_store_release,
dm_store_upsert and the synchronous dm_store_apply start no row epoch when no part was rejected
and none carried a NaN.  Their key-clearing builds (dm_update.hip k_release_keys,
k_upsert_keys) store an invalid key for exactly the workgroup-bin resources of which they
wrote a row; every other key stays in use, and the next writeback tick stays FIXED, in place.

As in tests/test_keep_keys_gpu.py, whose store, Pair and helpers these tests import, nothing a
caller can read may depend on the mode: engine A runs with the mode off, engine B with
keep_keys(3), and after every call and every tick the two hold identical bits, B's leases
match the oracle's, and the oracle's host copy takes the same update.

What differs is the introspection.  After every tick in which all four workgroup bins ran
with keys in use, B's "fixed_items" must be exactly the expected set (Track.expected):

  * the resources A's last tick left bit for bit (Pair.valid: what a key says),
  * without those that hold a released row (their items carry the mask bit and go through
    k_block_rest every tick, which keeps no key) or whose live rows do not share one
    subclient count (never dense),
  * without those of which a release or an upsert wrote a row since the tick before: the
    tick handed them to k_block_rest (a mask bit, a pending arrival, a stale hint).

Right after a kept call the count must have dropped by exactly the touched resources that
held a key.  Updates of several rows of one resource either fit one wave (one deterministic
reduction, one atomic per sum) or re-send the stored values (every delta +0.0), so the order
of the update kernels' atomics cannot show in the sums.  The workgroup bins of this store
hold four to six resources, so the quarter bound (dm_split_form.h) is passed by two updated
rows: a test that wants the next tick FIXED updates one row between two ticks.
"""
import numpy as np
import pytest

from doorman_amd import _lib
from doorman_amd import workloads as W
from test_keep_keys_gpu import NOW, R_LARGE, R_SMALL, Pair, by_size, make_store, store  # noqa: F401 (store: a fixture)

pytestmark = pytest.mark.gpu

NBINS = 4  # the store's workgroup bins (257-512, 513-1024, 1025-2048, 2049-4096 rows), one part each
MODE = _lib.DM_KEEP_REFRESH | _lib.DM_KEEP_UPDATES


class Track:
    """A Pair with B at mode 3, the clock, and the set of B's valid keys."""

    def __init__(self, snap, under=()):
        self.P = P = Pair(snap, under, keep=False)
        P.B.keep_keys(MODE)
        self.dt = 0
        self.keys = np.zeros(len(P.off) - 1, bool)  # B's valid keys in use (expected)
        self.touched = set()  # resources a release or an upsert wrote since the last tick

    def close(self):
        self.P.close()

    def seg(self, rows):
        return np.searchsorted(self.P.off, np.asarray(rows, np.int64), side="right") - 1

    # -- ticks --
    def tick(self, label, **kw):
        a, b = self.P.tick(label, self.dt, **kw)
        self.dt += 2
        # (a tick in which some bin ran another form: which keys are in use is not tracked)
        self.keys = self.expected() if b["parts"] == NBINS else None
        self.touched = set()
        if b["parts"] == NBINS:
            assert b["items"] == int(self.keys.sum()), (label, b, np.flatnonzero(self.keys))
        return a, b

    def expected(self):
        P, h = self.P, self.P.host
        live = h["expiry_ns"] != W.RELEASED
        keys = P.valid().copy()
        for r in np.flatnonzero(keys):
            lo, hi = P.off[r], P.off[r + 1]
            sub = h["subclients"][lo:hi][live[lo:hi]]
            if not live[lo:hi].all() or (len(sub) and (sub != sub[0]).any()):
                keys[r] = False
        keys[list(self.touched)] = False
        return keys

    def engage(self, label="engage", ticks=5):
        """Writeback ticks until every bin runs with keys in use; B's keys are then the
        expected set (asserted by tick)."""
        for t in range(ticks):
            a, b = self.tick(f"{label}: tick {t + 1}")
            if b["parts"] == NBINS and b["sweep"] == NBINS:
                return b["items"]
        raise AssertionError((label, a, b))

    # -- calls --
    def stats(self, e=None):
        return (e or self.P.B).keep_stats()

    def items(self, e=None):
        return (e or self.P.B).store_stats()["fixed_items"]

    def host_release(self, rows):
        h = self.P.host
        h["has"][rows], h["wants"][rows], h["subclients"][rows] = 0.0, 0.0, 0
        h["expiry_ns"][rows] = W.RELEASED
        W.add_store_sums(h)

    def host_upsert(self, rows, has, wants, sub, exp):
        h = self.P.host
        h["has"][rows], h["wants"][rows], h["subclients"][rows], h["expiry_ns"][rows] = has, wants, sub, exp
        W.add_store_sums(h)

    def kept(self, rows, label, counter, call):
        """A call that B keeps: `counter` of keep_stats moves by one, B's valid keys drop by
        exactly the touched resources that held one, A has none in use."""
        before = self.stats()
        had = self.items()
        call()
        self.P.same(label, leases=False)
        touched = set(int(r) for r in self.seg(rows))
        self.touched |= touched
        after = self.stats()
        assert after[counter] == before[counter] + 1, (label, before, after)
        assert after["kept_update_rows"] == before["kept_update_rows"] + len(rows), (label, before, after)
        assert self.items(self.P.A) == 0, label
        if self.keys is None:  # (no exact count to hold it against: no key may appear, none but the touched may go)
            most = sum(1 for r in touched if self.P.keyed[r])
            assert had - most <= self.items() <= had, (label, had, sorted(touched))
            return None
        assert had == int(self.keys.sum()), (label, had, np.flatnonzero(self.keys))
        drop = sum(1 for r in touched if self.keys[r])
        self.keys[list(touched)] = False
        assert self.items() == had - drop, (label, had, drop, sorted(touched))
        return drop

    def ended(self, label):
        """A call that ended the keys' use in B as in A."""
        self.keys = np.zeros(len(self.P.off) - 1, bool)
        assert self.items() == 0 and self.items(self.P.A) == 0, label

    def release(self, rows, label):
        rows = np.asarray(rows, np.int64)

        def call():
            self.P.both(lambda e: e.release(rows))
            self.host_release(rows)

        return self.kept(rows, label, "kept_releases", call)

    def upsert(self, rows, has, wants, sub, exp, label):
        rows = np.asarray(rows, np.int64)
        cols = [np.asarray(has, np.float64), np.asarray(wants, np.float64), np.asarray(sub, np.int64),
                np.asarray(exp, np.int64)]

        def call():
            self.P.both(lambda e: e.upsert(rows, *cols))
            self.host_upsert(rows, *cols)

        return self.kept(rows, label, "kept_upserts", call)

    def resend(self, rows, saved, label):
        """Upsert the rows with what `saved` (a copy of the host columns) holds for them, live
        until NOW + 900 s: re-sent to a live row it changes no sum; to a released row it is the
        arrival that restores it."""
        rows = np.asarray(rows, np.int64)
        return self.upsert(rows, saved["has"][rows], saved["wants"][rows], saved["subclients"][rows],
                           np.full(len(rows), NOW + 900 * W.NS), label)


@pytest.fixture
def track(store):
    snap, under, over = store
    T = Track(snap, under)
    try:
        yield T, snap, under, over
    finally:
        T.close()


def test_one_release(track):
    """(Fails without the feature: any release left no key in use.)  One released row clears
    one key; B's next tick is the sweep in place, A's runs without keys; two ticks later, with
    a density record that counts the resource's mask bit, B is still FIXED without it."""
    T, snap, under, over = track
    P = T.P
    items = T.engage()
    assert T.stats() == {"mode": 3, "kept_refreshes": 0, "kept_releases": 0, "kept_upserts": 0, "kept_batches": 0,
                         "kept_update_rows": 0}
    assert T.stats(P.A)["mode"] == 0
    r = by_size(snap, under, 1024)
    assert T.keys[r]
    assert T.release([P.row(r, 700)], "release") == 1
    assert T.items() == items - 1
    assert T.stats()["kept_releases"] == 1 and T.stats(P.A)["kept_releases"] == 0
    a, b = T.tick("the next tick")
    assert b["parts"] == NBINS and b["sweep"] == NBINS and b["inplace"] == 1 and a["parts"] == 0, (a, b)
    assert T.stats()["kept_update_rows"] == 0
    for t in range(2):
        a, b = T.tick(f"tick {t + 2} after the release")
        assert b["parts"] == NBINS and b["sweep"] == NBINS, (a, b)  # (tick asserts the keys: the expected set)
    assert not T.keys[r] and all(T.keys[x] for x in P.under if x != r), T.keys
    assert not P.B.store_lost()


def test_arrivals(track):
    """A narrow arrival into a freed row (the state stays dense, the tick absorbs it); an
    explicit-expiry upsert of a live row (its dense state ends, its key alone is cleared, and
    the resource is dense and keyed again within three ticks); an upsert with count 2
    (maybe_general: k_general decides the resource, which never holds a key again)."""
    T, snap, under, over = track
    P = T.P
    T.engage()
    r = by_size(snap, under, 1024)
    row = np.array([P.row(r, 700)], np.int64)
    T.release(row, "release")
    T.tick("tick after the release")

    now = NOW + T.dt * W.NS  # the next tick's time: the arrival's expiry is not before the followers'
    before = T.stats()
    P.both(lambda e: e.apply(upsert=(row, None, np.full(1, 0.125), np.ones(1, np.int32), None), now_ns=now))
    T.host_upsert(row, 0.0, 0.125, 1, now + 20 * W.NS)
    P.same("narrow arrival", leases=False)
    T.touched.add(r)
    assert T.stats()["kept_batches"] == before["kept_batches"] + 1
    assert T.items() == int(T.keys.sum()) and not T.keys[r]  # (its key was invalid already)
    dense = P.B.store_stats()["dense_resources"]
    T.tick("tick that absorbs the arrival")
    assert P.B.store_stats()["dense_resources"] == dense  # the state stayed dense throughout
    T.engage("after the arrival")
    assert T.keys[r], T.keys  # no released row is left: keyed again

    r2 = by_size(snap, under, 2048)
    row2 = [P.row(r2, 100)]
    saved = {k: P.host[k].copy() for k in ("has", "wants", "subclients")}
    had = int(T.keys.sum())
    assert T.keys[r2]
    dense = P.B.store_stats()["dense_resources"]
    assert T.resend(row2, saved, "explicit-expiry upsert") == 1
    assert T.items() == had - 1
    assert P.B.store_stats()["dense_resources"] == dense - 1
    for t in range(3):
        a, b = T.tick(f"tick {t + 1} after the explicit upsert")
        assert b["parts"] == NBINS and (t > 0 or a["parts"] == 0), (a, b)  # one row: every other key stayed in use
    assert T.keys[r2] and P.B.store_stats()["dense_resources"] == dense

    r3 = by_size(snap, under, 512)
    row3 = np.array([P.row(r3, 9)], np.int64)
    T.upsert(row3, P.host["has"][row3], P.host["wants"][row3], [2], [NOW + 900 * W.NS], "count 2")
    P.both(lambda e: e.set_profiling(True))
    T.tick("tick with k_general")
    assert "general" in P.B.kernel_times() and "general" in P.A.kernel_times()
    T.engage("after count 2")
    assert not T.keys[r3] and T.keys[r2] and T.keys[r]


def test_row_and_wave_edges(track):
    """Each call clears exactly the keys of the resources it writes: rows at the edges of a
    resource's waves; the last row of one resource and the first of the next; one row in each
    keyed resource (more than 8 runs in the wave: wave_seg_add's spread-out path); 70 rows of
    one resource (two waves); rows of the 40-row and the 5,000-row resource (no key).  By
    k_release_keys, then by k_upsert_keys restoring the rows."""
    T, snap, under, over = track
    P = T.P
    T.engage()
    n_keyed = int(P.keyed.sum())
    assert n_keyed == 18
    r = by_size(snap, under, 1000)
    # neighbours in two bins: this store's bins hold four to six resources, and two items of one
    # bin queued for the rest kernel are "too many" for try_split (64 ticks in the mixed kernel)
    r0, r1 = by_size(snap, over, 512), by_size(snap, under, 513)
    assert r1 == r0 + 1
    cases = [("wave edges", [P.row(r, i) for i in (0, 63, 64, 255, 256, -1)], 1),
             ("two resources", [P.row(r0, -1), P.row(r1, 0)], 1 + int(T.keys[r0]))]
    for label, rows, want in cases:
        saved = {k: P.host[k].copy() for k in ("has", "wants", "subclients")}
        assert T.release(rows, f"{label}: release") == want  # (the count after it is asserted there, exactly)
        T.engage(f"{label}: after the release", ticks=6)
        assert not T.keys[T.seg(rows)].any()
        assert T.resend(rows, saved, f"{label}: restore") == 0  # (a resource with a released row holds no key)
        T.engage(f"{label}: after the restore", ticks=6)
        assert all(T.keys[x] for x in P.under), (label, T.keys)

    big = by_size(snap, under, 4096)
    rows = [P.row(big, 1000 + 3 * i) for i in range(70)]
    saved = {k: P.host[k].copy() for k in ("has", "wants", "subclients")}
    assert T.keys[big]
    assert T.resend(rows, saved, "70 rows of one resource") == 1
    T.engage("after the 70 rows", ticks=6)

    had = int(T.keys.sum())
    assert T.release([P.row(R_SMALL, 7), P.row(R_LARGE, 4000)], "rows of resources without keys") == 0
    assert T.items() == had
    T.engage("after the rows without keys", ticks=6)
    assert all(T.keys[x] for x in P.under), T.keys

    # last, since it sends every bin into try_split's back-off: one row in each keyed resource
    rows = [P.row(int(x), 5) for x in np.flatnonzero(P.keyed)]
    saved = {k: P.host[k].copy() for k in ("has", "wants", "subclients")}
    had = int(T.keys.sum())
    assert T.release(rows, "every keyed resource: release") == had >= len(P.under)
    assert T.items() == 0
    T.tick("every keyed resource: tick after the release")
    T.resend(rows, saved, "every keyed resource: restore")
    for t in range(2):
        T.tick(f"every keyed resource: tick {t + 1} after the restore")
    assert not P.B.store_lost()


def test_ends_of_the_mode(track):
    """What ends it: a NaN, a rejection, mode 1 and mode 0 (as before the feature).  What does
    not: a batch of all three parts.  The mode can be switched mid-run."""
    T, snap, under, over = track
    P = T.P
    T.engage()
    r = next(x for x in under if snap["kind"][x] == W.FAIR_SHARE and P.keyed[x])
    row = np.array([P.row(r, 5)], np.int64)
    keep = {k: P.host[k][row].copy() for k in ("has", "wants", "subclients")}
    far = np.full(1, NOW + 900 * W.NS)

    before = T.stats()
    P.both(lambda e: e.upsert(row, keep["has"], np.full(1, np.nan), keep["subclients"], far))
    T.ended("NaN upsert")
    assert T.stats() == before
    P.both(lambda e: e.upsert(row, keep["has"], keep["wants"], keep["subclients"], far))  # repaired
    T.host_upsert(row, keep["has"], keep["wants"], keep["subclients"], far)
    T.engage("after the NaN", ticks=8)

    store_before = P.B.read_store()
    before = T.stats()
    for e in (P.A, P.B):
        with pytest.raises(_lib.DmError) as err:
            e.release(np.array([row[0], row[0] + 1, row[0]], np.int64))
        assert err.value.code == _lib.DM_E_INVAL
    T.ended("rejected release")
    assert T.stats() == before
    P.same("after the rejected release", leases=False)
    for k in store_before:
        assert np.array_equal(P.B.read_store()[k].view(np.int64), store_before[k].view(np.int64)), k
    T.engage("after the rejection", ticks=8)

    # one batch: a refresh of one row, a release, an upsert, in three resources
    ra, rb, rc = by_size(snap, under, 513), by_size(snap, under, 1025), by_size(snap, under, 2049)
    N = len(P.host["wants"])

    wrow, rel, up = P.row(ra, 11), np.array([P.row(rb, 12)], np.int64), np.array([P.row(rc, 13)], np.int64)
    value = P.host["wants"][wrow] * 0.5 + 1.0 / 1024

    def batch():
        words = np.zeros((N + 63) // 64, np.uint64)
        words[wrow // 64] = np.uint64(1) << np.uint64(wrow % 64)
        cols = (up, P.host["has"][up].copy(), P.host["wants"][up].copy(), np.ones(1, np.int64), far)
        P.both(lambda e: e.apply(wants_mask=words, wants=np.array([value]), release_rows=rel, upsert=cols))
        P.host["wants"][wrow] = value
        T.host_release(rel)
        T.host_upsert(*cols)

    assert T.keys[ra] and T.keys[rb] and T.keys[rc]
    assert T.kept([wrow, int(rel[0]), int(up[0])], "batch of three parts", "kept_batches", batch) == 3
    T.engage("after the batch", ticks=8)

    before = T.stats()
    P.both(lambda e: e.apply(wants_mask=np.array([1 << 5], np.uint64), wants=np.array([np.nan]),
                             wants_first_row=int(P.off[ra]) // 64 * 64))
    T.ended("batch with a NaN refresh")
    assert T.stats() == before
    nan_row = int(P.off[ra]) // 64 * 64 + 5
    P.both(lambda e: e.update_wants(np.array([nan_row], np.int64), P.host["wants"][[nan_row]]))  # repaired
    T.engage("after the NaN batch", ticks=8)

    # mode 1: a release ends every key's use, a refresh is kept; mode 0: nothing is kept
    P.B.keep_keys(_lib.DM_KEEP_REFRESH)
    assert T.stats()["mode"] == 1
    before = T.stats()
    frow = P.row(by_size(snap, under, 1000), 70)
    P.refresh([frow], [P.new_value(frow, False)], "mode 1: refresh")
    assert T.stats()["kept_refreshes"] == before["kept_refreshes"] + 1 and T.items() == int(T.keys.sum()) - 1
    T.keys[by_size(snap, under, 1000)] = False
    rel = np.array([P.row(rb, 14)], np.int64)
    P.both(lambda e: e.release(rel))
    T.host_release(rel)
    T.ended("mode 1: release")
    assert T.stats()["kept_releases"] == before["kept_releases"]
    P.B.keep_keys(MODE)
    T.engage("mode 3 again", ticks=8)
    P.B.keep_keys(0)
    before = T.stats()
    rel = np.array([P.row(rb, 15)], np.int64)
    P.both(lambda e: e.release(rel))
    T.host_release(rel)
    T.ended("mode 0: release")
    assert T.stats() == {**before, "mode": 0}
    P.B.keep_keys(MODE)
    T.engage("mode 3 once more", ticks=8)
    assert T.release([P.row(by_size(snap, under, 4096), 16)], "kept again") == 1
    a, b = T.tick("tick after it")
    assert b["parts"] > 0 and a["parts"] == 0, (a, b)


def test_stream_parts_and_the_guard():
    """A bin in two stream parts runs the dense kernel alone once verified.  Kept upserts that
    end dense states leave hint words set and stale, which the density count cannot see: the
    tick after each kept update must launch the rest kernel, and the guard must never trip."""
    rng = np.random.default_rng(9)
    R = 4200
    sizes = rng.integers(257, 300, R)
    N = int(sizes.sum())
    wants = rng.uniform(0.0, 1.0, N) * np.repeat(0.5 * 1000.0 / sizes, sizes)  # under capacity: gets == wants
    snap = W.make_snapshot(sizes, wants, np.zeros(N), 1, np.full(N, NOW + 600 * W.NS),
                           np.where(np.arange(R) % 2, W.FAIR_SHARE, W.PROPORTIONAL_SHARE).astype(np.int32), 1000.0,
                           lease_length_s=60)
    T = Track(snap)
    P = T.P
    try:
        assert P.B.plan_info()["stream_parts"] == 2 and P.A.plan_info()["stream_parts"] == 2
        P.both(lambda e: e.set_profiling(True))
        rest = lambda e: e.kernel_times().get("block128x4_rest", (0, 0.0))[0]
        seen = []
        for t in range(10):
            if t >= 2:
                rs = rng.choice(R, 50, replace=False)
                rows = P.off[rs] + rng.integers(0, 257, 50)
                rows = rows[P.host["expiry_ns"][rows] != W.RELEASED]
                if t % 2 == 0:
                    saved = {k: P.host[k].copy() for k in ("has", "wants", "subclients")}
                    T.resend(rows, saved, f"upserts {t}")
                else:
                    T.release(rows, f"releases {t}")
            before = rest(P.B)
            P.tick(f"tick {t + 1}", 2 * t)
            assert not P.A.store_lost() and not P.B.store_lost()
            seen.append((rest(P.A), rest(P.B)))
            if t >= 2:
                assert rest(P.B) > before, (t, seen)  # the rest kernel follows the kept update
        st = T.stats()
        assert st["kept_upserts"] == 4 and st["kept_releases"] == 4, st
    finally:
        T.close()


def test_the_quarter_bound(track):
    """One call that releases a row in two of the six resources of the 513-1024-row bin, more
    than a quarter of them: B's next tick runs without keys, as it did before the feature, the
    results are right, and the keys engage again."""
    T, snap, under, over = track
    P = T.P
    T.engage()
    rows = [P.row(by_size(snap, under, 1000), 3), P.row(by_size(snap, under, 1024), 4)]
    saved = {k: P.host[k].copy() for k in ("has", "wants", "subclients")}
    assert T.release(rows, "two releases") == 2
    a, b = T.tick("the next tick")
    assert b["parts"] == 0 and b["items"] == 0, (a, b)
    # two of its six resources hold a released row: that bin runs as before the feature (and
    # for 64 ticks in the mixed kernel: try_split); the other three come back
    for t in range(4):
        a, b = T.tick(f"tick {t + 2}")
    assert b["parts"] == NBINS - 1 and b["items"] > 0, (a, b)
    T.resend(rows, saved, "restore")
    T.tick("tick after the restore")
    assert not P.B.store_lost()
