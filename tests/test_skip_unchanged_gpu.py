"""The dense kernels' skip of unchanged gets stores (dm_tick_group.hip group_segment) and the
column rule that lets it engage (dm_apportion: in place unless the caller asks for the
alternate column, the speculative chain may run, or -- on a store beyond the Infinity
Cache -- a call wrote rows since the last writeback tick).

A writeback tick in place leaves out the gets store of every 64-row run whose rows it
leaves bit for bit unchanged.  Nothing the caller can read may depend on it: a store
ticked in place (skipping) and the same store ticked on the alternate column (which
never skips) must hold identical bits after every tick, through wants refreshes,
releases, arrivals, capacity changes and a lapse; ticks may change the column mode
freely; a non-writeback tick never skips.

The store: two resources at each first and last row count of every dense instance
(257 ... 4096: most no multiple of 64, so their last runs are partial), kinds 2 and 3,
one subclient, 20-s leases.  Of each pair one is clearly under capacity (sum of wants
<= C / 2: gets == wants in any summation order, a fixed point from the second tick on)
and one over capacity with wants multiples of 2^-10 and C a power of two; two more
resources have random wants.  The oracle alone confirms that at least 80 % of the
resources are fixed points by tick 3 (a condition of the data, not a device result)."""
import numpy as np
import pytest

from doorman_amd import workloads as W
from oracle import oracle as O
from parity_util import assert_leases_match

pytestmark = pytest.mark.gpu

NOW = W.NOW_NS
EDGES = [257, 512, 513, 1000, 1024, 1025, 2048, 2049, 4096]
SEED = 1  # chosen so that the oracle alone meets the fixed-point condition below
COLS = ("has", "wants", "subclients", "expiry_ns")


def make_store(seed=SEED, big=0):
    """(snapshot, under-capacity resources, over-capacity resources); big: one more resource
    of that many rows (above 4096: the large chain's)."""
    rng = np.random.default_rng(seed)
    sizes, kinds, caps, wants, under, over = [], [], [], [], [], []
    for i, n in enumerate(EDGES):
        for j in range(2):
            r = len(sizes)
            sizes.append(n)
            kinds.append(2 + (i + j) % 2)
            if j == 0:  # sum of wants <= C / 2
                C = 1000.0
                w = rng.uniform(0.0, 1.0, n) * (0.5 * C / n)
                under.append(r)
            else:  # about twice the capacity is wanted; every wants a multiple of 2^-10, C = 2^12
                C = 4096.0
                w = np.round(rng.uniform(0.0, 4.0, n) * (C / n) * 1024.0) / 1024.0
                over.append(r)
            caps.append(C)
            wants.append(w)
    for n in (700, 3000) + ((big,) if big else ()):  # a tenth of the resources: random wants
        sizes.append(n)
        kinds.append(3 if n != 3000 else 2)
        caps.append(777.7)
        wants.append(rng.uniform(0.0, 2.5, n) * (777.7 / n))
    wants = np.concatenate(wants)
    N = len(wants)
    cap_row = np.repeat(np.asarray(caps), sizes) / np.repeat(np.asarray(sizes, np.float64), sizes)
    has = rng.uniform(0.0, 0.4, N) * cap_row
    exp = NOW + rng.integers(30, 300, N, dtype=np.int64) * W.NS
    snap = W.make_snapshot(sizes, wants, has, np.ones(N, np.int64), exp, np.asarray(kinds, np.int32),
                           np.asarray(caps), lease_length_s=20, refresh_interval_s=5)
    return snap, under, over


def copy_of(snap):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in snap.items()}


def host_tick(host, now):
    """The oracle's writeback tick on the host copy; returns its result."""
    ref = O.apportion(host, now)
    live = ref["expiry_ns"] != W.RELEASED
    host["has"] = np.where(live, ref["gets"], 0.0)
    host["wants"] = np.where(live, host["wants"], 0.0)
    host["subclients"] = np.where(live, host["subclients"], 0)
    host["expiry_ns"] = ref["expiry_ns"].copy()
    W.add_store_sums(host)
    return ref


def fixed_share(snap, ticks=3):
    """Per resource: tick `ticks` leaves every row's has bit for bit unchanged (oracle only)."""
    host = copy_of(snap)
    off = host["seg_off"]
    for t in range(ticks):
        before = host["has"].copy()
        host_tick(host, NOW + 2 * t * W.NS)
    same = before.view(np.int64) == host["has"].view(np.int64)
    return np.array([same[off[r]:off[r + 1]].all() for r in range(len(off) - 1)])


@pytest.fixture(scope="module")
def store():
    snap, under, over = make_store()
    fixed = fixed_share(snap)  # the data's condition: most resources are fixed points by tick 3,
    assert fixed.mean() >= 0.8  # among them the over-capacity one whose capacity a test halves
    assert fixed[next(r for r in over if snap["seg_off"][r + 1] - snap["seg_off"][r] == 1024)]
    return snap, under, over


def assert_same_state(A, B, label):
    sa, sb = A.read_store(), B.read_store()
    for k in COLS:
        np.testing.assert_array_equal(sa[k].view(np.int64), sb[k].view(np.int64), err_msg=f"{label}: {k}")
    for x, y, k in zip(A.leases(), B.leases(), ("gets", "expiry")):
        np.testing.assert_array_equal(x.view(np.int64), y.view(np.int64), err_msg=f"{label}: leases {k}")
    ra, rb = A.resources(), B.resources()
    for k in ra:
        np.testing.assert_array_equal(ra[k].view(np.int64), rb[k].view(np.int64), err_msg=f"{label}: resources {k}")


@pytest.mark.parametrize("split", ["1", "0"])
def test_skipping_and_alternate_ticks_agree_bit_for_bit(monkeypatch, store, split):
    """Engine A ticks on the alternate column (never skips), engine B under "auto" (in place:
    skips unchanged runs).  After each of 8 writeback ticks the two stores, their leases and
    their resources hold identical bits, and B matches the oracle on a host copy.  Between
    ticks: one wants refresh in each of three fixed-point resources (a row of the second
    wave, and rows of the last, partial run: one run changes, its neighbours stay), a
    release in a fixed-point resource, an arrival into the freed slot, a capacity halved,
    and at the end every follower lapses (every gets 0.0).  split: DM_DENSE_SPLIT, the
    dense-only kernels (1) or the one-kernel form (0)."""
    from doorman_amd.engine import Engine
    monkeypatch.setenv("DM_DENSE_SPLIT", split)  # read when the context is created
    snap, under, over = store
    off = np.asarray(snap["seg_off"])
    by_size = lambda group, n: next(r for r in group if off[r + 1] - off[r] == n)
    A, B = Engine(0), Engine(0)
    try:
        A.load(snap)
        B.load(snap)
        host = copy_of(snap)

        def both(fn):
            fn(A)
            fn(B)

        freed = int(off[by_size(under, 1024)] + 700)
        for tick, dt in enumerate([0, 2, 4, 6, 8, 10, 12, 40], start=1):
            now = NOW + dt * W.NS
            if tick == 3:
                rows = np.array([off[by_size(under, 1000)] + 70,     # second wave, first run
                                 off[by_size(under, 1000)] + 990,    # the last, partial run
                                 off[by_size(under, 2049)] + 2048,   # a run of one row
                                 off[by_size(under, 513)] + 512], np.int64)
                nw = host["wants"][rows] * 0.5 + 1.0 / 1024
                both(lambda e: e.update_wants(rows, nw))
                host["wants"][rows] = nw
                W.add_store_sums(host)
            if tick == 5:
                rows = np.array([freed], np.int64)
                both(lambda e: e.release(rows))
                host["has"][rows], host["wants"][rows], host["subclients"][rows] = 0.0, 0.0, 0
                host["expiry_ns"][rows] = W.RELEASED
                W.add_store_sums(host)
            if tick == 6:
                rows, ne = np.array([freed], np.int64), now + 100 * W.NS
                both(lambda e: e.upsert(rows, np.zeros(1), np.full(1, 0.125), np.ones(1, np.int64), np.full(1, ne)))
                host["has"][rows], host["wants"][rows], host["subclients"][rows] = 0.0, 0.125, 1
                host["expiry_ns"][rows] = ne
                W.add_store_sums(host)
            if tick == 7:
                host["capacity"] = host["capacity"].copy()
                host["capacity"][by_size(over, 1024)] *= 0.5
                both(lambda e: e.load_config(host))
            A.apportion(now, writeback=True, wb_columns="alternate")
            B.apportion(now, writeback=True, wb_columns="auto")
            assert A.plan_info()["wb_inplace"] == 0 and B.plan_info()["wb_inplace"] == 1
            gets, exp = B.leases()
            ref = O.apportion(host, now)
            assert_leases_match(host, gets, exp, ref, f"tick {tick}")
            host_tick(host, now)
            assert_same_state(A, B, f"tick {tick}")
        assert not gets.any() and (exp == W.RELEASED).all()  # every follower lapsed at the last tick
    finally:
        A.close()
        B.close()


def test_column_mode_may_change_from_tick_to_tick(store):
    """auto, alternate, auto, auto, alternate, alternate, inplace with a wants refresh before
    the third tick: every tick matches the oracle (a skip taken against the wrong column
    would leave values two ticks old) and plan_info names the column written."""
    from doorman_amd.engine import Engine
    snap, _, _ = store
    rng = np.random.default_rng(3)
    with Engine(0) as eng:
        eng.load(snap)
        assert eng.plan_info()["wb_inplace"] == -1
        host = copy_of(snap)
        modes = ["auto", "alternate", "auto", "auto", "alternate", "alternate", "inplace"]
        for t, (mode, want) in enumerate(zip(modes, [1, 0, 1, 1, 0, 0, 1])):
            now = NOW + 2 * t * W.NS
            if t == 2:
                rows = np.sort(rng.choice(len(host["wants"]), 200, replace=False))
                nw = host["wants"][rows] * 0.75
                eng.update_wants(rows, nw)
                host["wants"][rows] = nw
                W.add_store_sums(host)
            eng.apportion(now, writeback=True, wb_columns=mode)
            assert eng.plan_info()["wb_inplace"] == want, f"tick {t}"
            gets, exp = eng.leases()
            ref = O.apportion(host, now)
            assert_leases_match(host, gets, exp, ref, f"tick {t} ({mode})")
            host_tick(host, now)
            st = eng.read_store()
            np.testing.assert_array_equal(st["expiry_ns"], host["expiry_ns"], err_msg=f"tick {t}")


def test_non_writeback_tick_between_writeback_ticks(store):
    """writeback, non-writeback, writeback: the non-writeback tick writes its own output
    column and must not skip; its leases and both writeback ticks match the oracle."""
    from doorman_amd.engine import Engine
    snap, _, _ = store
    with Engine(0) as eng:
        eng.load(snap)
        host = copy_of(snap)
        for t, wb in enumerate([True, True, False, True]):  # (two writeback ticks first: fixed points)
            now = NOW + 2 * t * W.NS
            eng.apportion(now, writeback=wb)
            gets, exp = eng.leases()
            ref = O.apportion(host, now)
            assert_leases_match(host, gets, exp, ref, f"tick {t} writeback={wb}")
            if wb:
                host_tick(host, now)
        assert eng.plan_info()["wb_inplace"] == 1


def test_column_choice_follows_the_speculative_chain():
    """Under "auto" a store with a resource above 4096 rows that may take the speculative
    chain writes the alternate column; a store without one writes in place."""
    from doorman_amd.engine import Engine
    for big, want in ((6000, 0), (0, 1)):
        snap, _, _ = make_store(big=big)
        with Engine(0) as eng:
            eng.load(snap)
            host = copy_of(snap)
            for t in range(3):  # (loaded rows carry explicit expiries: the first tick cannot speculate)
                now = NOW + 2 * t * W.NS
                eng.apportion(now, writeback=True)
                gets, exp = eng.leases()
                assert_leases_match(host, gets, exp, O.apportion(host, now), f"big={big} tick {t}")
                host_tick(host, now)
            assert eng.plan_info()["wb_inplace"] == want, f"big={big}"


def test_store_beyond_the_cache_alternates_after_row_writes():
    """A store above 1 GiB of lease table (23M rows) streams from HBM: under "auto" the first
    writeback tick after a call that wrote rows (the load, a wants refresh) writes the
    alternate column, every other one in place.  Its first 20 resources match the oracle
    after every tick."""
    from doorman_amd.engine import Engine
    snap = W.uniform(23_000, 1000, seed=5)
    host = W.subset_range(snap, 0, 20)
    n = len(host["wants"])
    with Engine(0) as eng:
        eng.load(snap)
        for t, want in enumerate([0, 1, 1, 0, 1]):
            now = NOW + 2 * t * W.NS
            if t == 3:
                rows, nw = np.array([3 * 1000 + 70], np.int64), np.array([0.25])
                eng.update_wants(rows, nw)
                host["wants"][rows] = nw
                W.add_store_sums(host)
            eng.apportion(now, writeback=True)
            assert eng.plan_info()["wb_inplace"] == want, f"tick {t}"
            gets, exp = eng.leases(0, n)
            assert_leases_match(host, gets, exp, O.apportion(host, now), f"tick {t}")
            host_tick(host, now)
