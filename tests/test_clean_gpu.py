"""dm_store_clean on the GPU: Clean (store.go:169-181) run on the device store, against the
host route it replaces -- dm_read_store of the expiry column, the predicate in numpy,
dm_store_release of the rows found -- against the reference store's Clean() and against the
CPU oracle's ticks on the cleaned store.

Bars: the list of released rows, its count, next_expiry_ns, the four store columns and the
resources' counts exact; sum_has / sum_wants of the two routes within parity_util's bar
(REL_TOL x the scale assert_resources_match uses: both routes subtract the same rows from
the same running sums through atomics whose order is free); the ticks that follow under
parity_util's bars.

The state a clean starts from is read back from the device (dm_read_store /
dm_read_resources), so no test carries a copy of the update kernels' arithmetic.
"""
import numpy as np
import pytest

from doorman_amd import _lib
from doorman_amd import workloads as W
from oracle import oracle as O
from parity_util import (assert_leases_match, assert_resources_match, binned_sizes, float_close,
                         snapshot_with_sizes)

pytestmark = pytest.mark.gpu
NOW = W.NOW_NS
S = W.NS
# tests/test_relayout_gpu.py's sizes: empty segments, the tile / group bin boundary, the wave
# boundary, the chunk size, the 4096-row scan block and kLargeMin, a resource over three scan
# blocks, segment starts off the block boundaries (28k rows over eight scan blocks)
SIZES = np.array([0, 1, 4, 5, 64, 65, 2048, 2049, 4095, 4096, 4097, 9000, 0, 3], np.int64)
ALL_RELEASED = 5     # the 65-row resource: every row released
HETERO = (4, 7, 11)  # resources with a few other subclient counts (64, 2049 and 9000 rows)
# lease lengths (s) the cases below count on: after a writeback tick at NOW the followers of
# resources 7 and 9 lapse before NOW + 150 s, those of 6 (a dense 2048-row resource) and 11
# (the 9000-row chain resource) before NOW + 300 s, those of 8 (dense, 4095 rows) and 10 stay
LEASES = {6: 250, 7: 100, 8: 500, 9: 120, 10: 400, 11: 280}
# rows at the scan blocks' edges (index = 4095 and 0 mod 4096), forced live so that a clean
# releases them: 4095 / 4096 lie in resource 7, 8191 / 8192 in resource 8
EDGE_ROWS = np.array([4095, 4096, 8191, 8192], np.int64)
COLS = ("has", "wants", "subclients", "expiry_ns")
STATES = ("loaded", "followers", "mixed", "async")
WHENS = ("before", "now", "exact", "+150s", "+300s", "all")


@pytest.fixture(scope="module")
def engines():
    from doorman_amd.engine import Engine
    a, b = Engine(0), Engine(0)
    yield a, b
    a.close()
    b.close()


def _copy(snap):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in snap.items()}


_SNAP = {}


def _snap():
    """The shared store (built once, handed out as copies): every kind, 5% of the rows already
    expired, ~15% released, one resource with every row released, a few heterogeneous
    subclient counts."""
    if not _SNAP:
        rng = np.random.default_rng(909)
        snap = snapshot_with_sizes(rng, SIZES, kinds=(0, 1, 2, 3), expired_frac=0.05, learning_frac=0.1,
                                   parent_expired_frac=0.05)
        so, N = snap["seg_off"], len(snap["wants"])
        for r, v in LEASES.items():
            snap["lease_length_s"][r] = v
        for r in HETERO:
            snap["kind"][r] = W.FAIR_SHARE
            snap["learning_end_ns"][r] = W.INT64_MIN
            rows = so[r] + rng.choice(int(so[r + 1] - so[r]), 6, replace=False)
            snap["subclients"][rows] = rng.integers(2, 5, 6)
        free = rng.random(N) < 0.15
        free[so[ALL_RELEASED]:so[ALL_RELEASED + 1]] = True
        free[EDGE_ROWS] = False
        snap["wants"][free] = 0.0
        snap["has"][free] = 0.0
        snap["subclients"][free] = 0
        snap["expiry_ns"][free] = W.RELEASED
        snap["subclients"][EDGE_ROWS] = 1
        snap["expiry_ns"][EDGE_ROWS] = NOW + 100 * S
        W.add_store_sums(snap)
        _SNAP["s"] = snap
    return _copy(_SNAP["s"])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _assert_same_store(got, want, label):
    for k in COLS:
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=f"{label}: {k} must be bit-identical")


def _round_of_updates(st, rng, n_gone=40, n_arrive=40, keep_out=EDGE_ROWS):
    """One round's updates on the store st: departures, arrivals and full refreshes with
    explicit expiries, and a masked wants refresh of 5% of the rows that stay."""
    live = np.setdiff1d(np.flatnonzero(st["expiry_ns"] != W.RELEASED), keep_out)
    free = np.flatnonzero(st["expiry_ns"] == W.RELEASED)
    gone = rng.choice(live, n_gone, replace=False)
    keep = np.setdiff1d(live, gone)
    arrive = rng.choice(free, n_arrive, replace=False)
    refresh = rng.choice(keep, 10, replace=False)
    up_rows = np.concatenate([arrive, refresh])
    n = len(up_rows)
    up = (up_rows, np.concatenate([np.zeros(n_arrive), st["has"][refresh]]), rng.uniform(0.1, 50.0, n),
          np.ones(n, np.int64), np.full(n, NOW + 600 * S, np.int64))
    masked = np.sort(rng.choice(np.setdiff1d(keep, refresh), len(keep) // 20, replace=False))
    mask, mw = W.rows_to_mask(masked, len(st["wants"])), rng.uniform(0.1, 50.0, len(masked))
    return gone, up, mask, mw, np.setdiff1d(free, arrive)


def _prepare(eng, state):
    """Bring eng's store into `state` (as tests/test_relayout_gpu.py's _prepare); returns the
    configuration snapshot it runs under."""
    snap = _snap()
    eng.load(snap)
    if state == "loaded":
        return snap
    eng.apportion(NOW, writeback=True)  # every live row a follower, lapsed rows released
    if state == "followers":
        return snap
    rng = np.random.default_rng(11)
    gone, up, mask, mw, free = _round_of_updates(eng.read_store(), rng)
    if state == "mixed":
        eng.release(gone)
        eng.upsert(*up)
        eng.update_wants_mask(mask, mw)
        # arrivals as a round sends them (no expiry column: now + the lease length), which a
        # dense resource takes into its arrival mask
        narrow = free[::9][:30]
        eng.apply(upsert=(narrow, None, rng.uniform(0.1, 50.0, len(narrow)), np.ones(len(narrow), np.int32), None),
                  now_ns=NOW + S)
    else:  # the same round as one asynchronous batch, not yet retired when the clean is called
        eng.apply(mask, mw, gone, up, asynchronous=True)
    return snap


def _state_of(eng):
    """The store as the device reports it: the four columns and the running sums."""
    return eng.read_store(), eng.resources(safe=False)


def _snapshot_of(cfg, st, res):
    """The snapshot the device's state amounts to: its rows and running sums under cfg."""
    post = {"seg_off": cfg["seg_off"], **{k: st[k] for k in COLS}}
    for k in W.CFG_FIELDS:
        post[k] = cfg[k]
    post["agg_count"], post["agg_sum_has"], post["agg_sum_wants"] = res["count"], res["sum_has"], res["sum_wants"]
    return post


def _lapsed(st, when):
    """The reference's predicate (store.go:174) on rows the device reported."""
    e = st["expiry_ns"]
    return np.flatnonzero((e != W.RELEASED) & (when > e))


def _next_expiry(st, when):
    e = st["expiry_ns"]
    stay = e[(e != W.RELEASED) & ~(when > e)]
    return int(stay.min()) if len(stay) else _lib.DM_NO_EXPIRY


def _released_model(st, rows):
    out = {k: st[k].copy() for k in COLS}
    out["has"][rows] = 0.0
    out["wants"][rows] = 0.0
    out["subclients"][rows] = 0
    out["expiry_ns"][rows] = W.RELEASED
    return out


def _assert_sums_close(got, want, cfg, st_before, label):
    """count exact; the float sums under assert_resources_match's scale for them."""
    np.testing.assert_array_equal(got["count"], want["count"], err_msg=f"{label}: count")
    scale_w = np.maximum(np.abs(cfg["capacity"]), 1.0)
    scale_h = np.maximum(scale_w, W.segment_sums(np.abs(st_before["has"]), cfg["seg_off"]))
    for k, scale in (("sum_wants", scale_w), ("sum_has", scale_h)):
        ok = float_close(got[k], want[k], scale)
        assert ok.all(), f"{label}: {k} at resources {np.flatnonzero(~ok).tolist()}: " \
                         f"{got[k][~ok].tolist()} vs {want[k][~ok].tolist()}"


def _assert_tick_matches(eng, cfg, now, label, writeback=True):
    """A tick at `now` against the oracle on the state read back before it; returns that
    state and the oracle's result."""
    st, res = _state_of(eng)
    post = _snapshot_of(cfg, st, res)
    ref = O.apportion(post, now)
    eng.apportion(now, writeback=writeback)
    gets, exp = eng.leases()
    assert_leases_match(post, gets, exp, ref, label)
    assert_resources_match(post, eng.resources(), ref, label)
    assert not eng.store_lost()
    return st, ref


def _when(when, st):
    """The case's time; for "exact", the expiry of a live row chosen from st (a median one
    among the distinct expiries after NOW), which must therefore stay."""
    if when == "exact":
        e = st["expiry_ns"]
        later = np.unique(e[(e != W.RELEASED) & (e > NOW)])
        return int(later[len(later) // 2])
    return {"before": NOW - 400 * S, "now": NOW, "+150s": NOW + 150 * S, "+300s": NOW + 300 * S,
            "all": NOW + 10**6 * S}[when]


def _rows_of(cfg, r):
    return slice(int(cfg["seg_off"][r]), int(cfg["seg_off"][r + 1]))


@pytest.mark.parametrize("when", WHENS)
@pytest.mark.parametrize("state", STATES)
def test_clean_equals_the_release_route(engines, state, when):
    """Context A cleans on the device; context B, in the same state, takes the route the call
    replaces.  (The asynchronous state's batch is in flight on both when they are called.)"""
    A, B = engines
    cfg = _prepare(A, state)
    _prepare(B, state)
    before, res0 = _state_of(B)
    dense_before = B.store_stats()
    now = _when(when, before)
    rows = _lapsed(before, now)
    label = f"{state}/{when}"

    got = A.clean(now)
    B.release(rows)

    # the list, the count, the next expiry
    assert got["released"] == len(rows), label
    np.testing.assert_array_equal(got["rows"], rows, err_msg=f"{label}: the released rows, ascending")
    assert got["next_expiry_ns"] == _next_expiry(before, now), label
    # the store: A against B and against the rows zeroed in numpy
    after = A.read_store()
    _assert_same_store(after, B.read_store(), label + " (A against B)")
    _assert_same_store(after, _released_model(before, rows), label + " (A against the model)")
    ra, rb = A.resources(safe=False), B.resources(safe=False)
    _assert_sums_close(ra, rb, cfg, before, label)
    gone = np.zeros(len(before["wants"]), np.int64)
    gone[rows] = before["subclients"][rows]
    np.testing.assert_array_equal(ra["count"], res0["count"] - W.segment_sums(gone, cfg["seg_off"]), err_msg=label)
    assert A.store_stats() == B.store_stats(), label

    # what the cases were chosen to hit
    if when == "before":
        assert len(rows) == 0
    if when in ("exact", "+150s", "+300s", "all") or (state, when) == ("loaded", "now"):
        assert len(rows) > 0
    if when == "exact":
        kept = before["expiry_ns"] == now
        assert kept.any() and (after["expiry_ns"][kept] == now).all(), f"{label}: a row expiring at now_ns stays"
    if when == "all":
        assert (after["expiry_ns"] == W.RELEASED).all() and got["next_expiry_ns"] == _lib.DM_NO_EXPIRY
    if when in ("+150s", "+300s", "all"):
        assert (rows % 4096 == 4095).any() and (rows % 4096 == 0).any(), f"{label}: rows at a scan block's edges"
    if (state, when) == ("followers", "+300s"):
        hit = np.zeros(len(before["wants"]), bool)
        hit[rows] = True
        live = before["expiry_ns"] != W.RELEASED
        whole = [r for r in range(len(SIZES)) if live[_rows_of(cfg, r)].any()
                 and (hit[_rows_of(cfg, r)] == live[_rows_of(cfg, r)]).all()]
        untouched = [r for r in range(len(SIZES)) if live[_rows_of(cfg, r)].any() and not hit[_rows_of(cfg, r)].any()]
        # 6 (2048 rows) and 8 (4095 rows): one subclient count, 257-4096 rows: dense after the tick
        assert 6 in whole and 11 in whole and 8 in untouched, (whole, untouched)
        assert dense_before["dense_resources"] >= 2, dense_before

    # the ticks that follow: Clean at `now` has nothing left to do, a minute later it has
    _assert_tick_matches(A, cfg, now, label + " tick")
    _assert_tick_matches(A, cfg, now + 60 * S, label + " tick + 60 s")


@pytest.mark.parametrize("state", ("loaded", "mixed"))
def test_clean_counts_match_the_reference_store(engines, state):
    """Per resource: the reference's store holding the device's live rows and running sums,
    its Clean() (store.go:169-181) against the device's."""
    A, _ = engines
    cfg = _prepare(A, state)
    before, res0 = _state_of(A)
    now = NOW + 150 * S
    got = A.clean(now)
    res = A.resources(safe=False)
    so = cfg["seg_off"]
    want = {"count": np.zeros(len(SIZES), np.int64), "sum_has": np.zeros(len(SIZES)), "sum_wants": np.zeros(len(SIZES))}
    for r in range(len(SIZES)):
        lo, hi = int(so[r]), int(so[r + 1])
        store = O.Store(max(hi - lo, 1))
        for i in range(lo, hi):
            if before["expiry_ns"][i] != W.RELEASED:
                store.put(i - lo, int(before["expiry_ns"][i]), float(before["has"][i]), float(before["wants"][i]),
                          int(before["subclients"][i]))
        store.set_sums(int(res0["count"][r]), float(res0["sum_has"][r]), float(res0["sum_wants"][r]))
        n = store.clean(now)
        assert n == int(((got["rows"] >= lo) & (got["rows"] < hi)).sum()), f"{state}: resource {r}"
        want["count"][r], want["sum_has"][r], want["sum_wants"][r] = store.count(), store.sum_has(), store.sum_wants()
    assert got["released"] == len(got["rows"]) > 0
    _assert_sums_close(res, want, cfg, before, state)


@pytest.mark.parametrize("state", ("loaded", "mixed"))
def test_peek_changes_nothing_and_predicts_the_tick(engines, state):
    A, _ = engines
    now = NOW + 150 * S
    _prepare(A, state)
    before, res0 = _state_of(A)  # (no tick result yet: the running sums themselves)
    first = A.clean(now, peek=True)
    st, res = _state_of(A)
    _assert_same_store(st, before, "after a peek")
    for k in ("count", "sum_has", "sum_wants"):
        np.testing.assert_array_equal(_bits(res[k]), _bits(res0[k]), err_msg=f"after a peek: {k}")
    A.apportion(NOW + 2 * S)  # not written back: its leases are the context's last result
    leases = A.leases()
    peek = A.clean(now, peek=True)
    np.testing.assert_array_equal(peek["rows"], _lapsed(before, now))
    np.testing.assert_array_equal(peek["rows"], first["rows"])
    assert peek["released"] == len(peek["rows"]) > 0
    _assert_same_store(A.read_store(), before, "after a tick and a peek")
    again = A.leases()  # the last tick's leases stay readable
    np.testing.assert_array_equal(_bits(again[0]), _bits(leases[0]))
    np.testing.assert_array_equal(again[1], leases[1])
    real = A.clean(now)
    np.testing.assert_array_equal(real["rows"], peek["rows"])
    assert (real["released"], real["next_expiry_ns"]) == (peek["released"], peek["next_expiry_ns"])
    with pytest.raises(_lib.DmError) as e:  # rows were released: the last tick's leases are gone
        A.leases()
    assert e.value.code == _lib.DM_E_STATE

    # on a fresh copy of the state: the peek names the rows the writeback tick's own Clean frees
    _prepare(A, state)
    before = A.read_store()
    peek = A.clean(now, peek=True)
    A.apportion(now, writeback=True)
    after = A.read_store()
    freed = np.flatnonzero((before["expiry_ns"] != W.RELEASED) & (after["expiry_ns"] == W.RELEASED))
    np.testing.assert_array_equal(peek["rows"], freed)


def test_clean_then_tick_is_the_tick(engines):
    """Every dispatch bin: Clean at NOW, then a tick at NOW that is not written back, against
    the oracle's tick (which cleans first) on the loaded snapshot."""
    A, _ = engines
    rng = np.random.default_rng(5)
    snap = snapshot_with_sizes(rng, binned_sizes(rng, per_bin=2, large=True), hetero=False)
    A.load(snap)
    ref = O.apportion(snap, NOW)
    got = A.clean(NOW)
    A.apportion(NOW)
    gets, exp = A.leases()
    assert_leases_match(snap, gets, exp, ref, "clean then tick")
    assert_resources_match(snap, A.resources(), ref, "clean then tick")
    want = np.flatnonzero((ref["expiry_ns"] == O.RELEASED) & (snap["expiry_ns"] != W.RELEASED))
    np.testing.assert_array_equal(got["rows"], want)
    assert got["released"] == len(want) > 0
    assert not A.store_lost()


def test_rounds_of_updates_clean_and_tick(engines):
    """The host loop the call exists for: four rounds a minute apart of a masked refresh, a
    few departures and arrivals, Clean, a writeback tick.  The arrivals take free rows only
    from the clean lists and the rows released at the start."""
    A, _ = engines
    cfg = _snap()
    # (a tick renews every lease it decides: only leases shorter than the rounds' minute lapse
    # between two ticks -- here those of a 64-row, a dense 2048-row and the 4097-row resource)
    cfg["lease_length_s"][[4, 6, 10]] = (20, 30, 45)
    A.load(cfg)
    A.apportion(NOW, writeback=True)
    rng = np.random.default_rng(23)
    st = A.read_store()
    N = len(st["wants"])
    pool = np.flatnonzero(st["expiry_ns"] == W.RELEASED)  # the host's free rows
    listed = np.zeros(0, np.int64)                        # every row a clean has reported so far
    from_lists = 0
    for k in range(1, 5):
        now = NOW + 60 * k * S
        live = np.flatnonzero(st["expiry_ns"] != W.RELEASED)
        gone = rng.choice(live, 5, replace=False)
        masked = np.sort(rng.choice(np.setdiff1d(live, gone), len(live) // 20, replace=False))
        take = rng.choice(len(pool), 25, replace=False)
        arrive, pool = pool[take], np.delete(pool, take)
        from_lists += int(np.isin(arrive, listed).sum())
        A.apply(W.rows_to_mask(masked, N), rng.uniform(0.1, 50.0, len(masked)), gone,
                (arrive, None, rng.uniform(0.1, 50.0, len(arrive)), np.ones(len(arrive), np.int32), None), now_ns=now)
        before = A.read_store()
        got = A.clean(now)
        np.testing.assert_array_equal(got["rows"], _lapsed(before, now), err_msg=f"round {k}")
        assert got["next_expiry_ns"] == _next_expiry(before, now), f"round {k}"
        _assert_same_store(A.read_store(), _released_model(before, got["rows"]), f"round {k}")
        listed = np.concatenate([listed, got["rows"]])
        pool = np.concatenate([pool, got["rows"]])
        _assert_tick_matches(A, cfg, now, f"round {k}")
        st = A.read_store()
    assert len(listed) > 4096 and from_lists > 0, (len(listed), from_lists)


def test_clean_is_profiled_under_the_release_class(engines):
    """The passes are timed as "store_release" (the count pass, then the apply pass when
    something lapsed); no kernel class is added."""
    A, _ = engines
    _prepare(A, "loaded")
    A.set_profiling(True)
    try:
        A.reset_kernel_times()
        assert A.clean(NOW - 400 * S)["released"] == 0
        assert A.kernel_times()["store_release"][0] == 1
        assert A.clean(NOW + 150 * S, peek=True)["released"] > 0
        assert A.clean(NOW + 150 * S)["released"] > 0
        times = A.kernel_times()
        assert times["store_release"][0] == 5 and times["store_release"][1] > 0.0
        assert set(times) <= set(_lib.kernel_class_names())
    finally:
        A.set_profiling(False)
        A.reset_kernel_times()
    assert not any("clean" in n for n in _lib.kernel_class_names())


def test_read_cleaned_ranges_and_states(engines):
    from doorman_amd.engine import Engine
    A, B = engines

    def code_of(fn):
        with pytest.raises(_lib.DmError) as e:
            fn()
        return e.value.code

    with Engine(0) as e0:  # no store
        assert code_of(lambda: e0.clean(NOW)) == _lib.DM_E_STATE
        assert code_of(lambda: e0.read_cleaned(0, 0)) == _lib.DM_E_STATE
    cfg = _prepare(A, "followers")
    assert code_of(lambda: A.read_cleaned(0, 0)) == _lib.DM_E_STATE  # loaded since any clean
    res = _lib.CleanResult()
    assert A._L.dm_store_clean(A._ctx, NOW, 2, res) == _lib.DM_E_INVAL  # an unknown flag bit
    assert A._L.dm_store_clean(A._ctx, NOW, _lib.DM_CLEAN_PEEK | 4, None) == _lib.DM_E_INVAL
    assert code_of(lambda: A.read_cleaned(0, 0)) == _lib.DM_E_STATE

    now = NOW + 300 * S
    before = A.read_store()
    got = A.clean(now, want_rows=False)
    n = got["released"]
    assert got["rows"] is None and n == len(_lapsed(before, now)) > 4096
    whole = A.read_cleaned()
    np.testing.assert_array_equal(whole, _lapsed(before, now))
    cuts = [0, 1, 63, 64, 4097, n - 1, n]
    parts = [A.read_cleaned(a, z - a) for a, z in zip(cuts[:-1], cuts[1:])]
    np.testing.assert_array_equal(np.concatenate(parts), whole)
    assert len(A.read_cleaned(n, 0)) == 0
    assert len(A.read_cleaned(5)) == n - 5
    for off, cnt in ((0, n + 1), (n, 1), (n + 1, 0), (-1, 1), (0, -1)):
        assert code_of(lambda: A.read_cleaned(off, cnt)) == _lib.DM_E_RANGE, (off, cnt)
    assert A._L.dm_store_clean(A._ctx, now, 0, None) == 0  # a NULL result; nothing is left to release
    assert A._L.dm_read_cleaned(A._ctx, 0, 0, None) == 0
    assert code_of(lambda: A.read_cleaned(0, 1)) == _lib.DM_E_RANGE
    assert A.clean(now)["released"] == 0 and len(A.read_cleaned()) == 0

    # a re-layout and a load end the list
    A.clean(NOW + 10**6 * S, peek=True)
    assert len(A.read_cleaned(0, 1)) == 1
    A.relayout(np.concatenate([[0], np.cumsum(SIZES + 1)]))
    assert code_of(lambda: A.read_cleaned(0, 0)) == _lib.DM_E_STATE
    A.clean(NOW, peek=True)
    A.read_cleaned(0, 0)
    A.load_store(_snap())
    assert code_of(lambda: A.read_cleaned(0, 0)) == _lib.DM_E_STATE

    # a rejected asynchronous batch in flight: its error, its applied parts, nothing released
    cfg = _prepare(A, "followers")
    _prepare(B, "followers")
    st = A.read_store()
    N = len(st["wants"])
    masked = np.flatnonzero(st["expiry_ns"] != W.RELEASED)[::50]
    mask, mw = W.rows_to_mask(masked, N), np.linspace(1.0, 9.0, len(masked))
    bad = np.array([3, N + 5], np.int64)
    A.apply(mask, mw, bad, asynchronous=True)
    with pytest.raises(_lib.DmError) as e:
        A.clean(now)
    assert e.value.code == _lib.DM_E_RANGE and "asynchronous batch" in str(e.value), str(e.value)
    assert code_of(lambda: B.apply(mask, mw, bad)) == _lib.DM_E_RANGE
    after = A.read_store()
    _assert_same_store(after, B.read_store(), "after the rejected batch")
    np.testing.assert_array_equal(after["expiry_ns"], st["expiry_ns"])  # nothing was released
    assert not np.array_equal(_bits(after["wants"]), _bits(st["wants"]))  # the refresh part was applied
    got = A.clean(now)  # ... and the call made again goes through
    np.testing.assert_array_equal(got["rows"], _lapsed(after, now))
    _assert_tick_matches(A, cfg, now, "after the rejected batch")
