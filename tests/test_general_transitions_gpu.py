"""Store updates that turn a store general, through every call that maintains the host's
routing state (dm_ctx.h: maybe_general, all_sub_one, and the window in which an
asynchronous batch is pending).

A FairShare resource whose live rows carry different subclient counts, or a NaN wants,
is left undecided by the tick's kernels and appended to a worklist; whether the
worklist is reset and k_general launched is the host's decision (dm_apportion:
`general`).  The flag words of the update kernels feed it through dm_store_upsert,
dm_store_update_wants[_mask], dm_store_apply, the retire of dm_store_apply_async
batches (dm_store_apply_wait, set reuse, dm_config_load) and dm_store_load's scan.  A
flag left false on a heterogeneous store shows only on the resources concerned: their
leases stay undecided.  So every cell here makes a few target resources of every
non-small class general by one cause, through one route, and compares every following
tick with the oracle on a host copy (expiries and counts exact, gets within
parity_util.REL_TOL x max(|ref|, capacity)); preconditions (the targets really are
heterogeneous, SumWants > capacity, k_general really ran) are asserted beside it.

The host copy keeps the reference's running sums: store.go:156-158 adds new - old to
sumWants / sumHas, so a NaN that once entered a sum stays in it (NaN - NaN is NaN) even
after the row that brought it is refreshed, released or lapses.  The device's running
sums behave the same, and the oracle takes the sums verbatim (_sums below).
"""
import numpy as np
import pytest

from doorman_amd import workloads as W
from oracle import oracle as O
from parity_util import assert_leases_match, snapshot_with_sizes
from test_parity_gpu import _apply_host, _writeback_host
from test_parts_gpu import _check

pytestmark = pytest.mark.gpu
NOW = W.NOW_NS
PER_BIN = 40  # resources per workgroup bin
_BINS = {"bin3": (290, 330), "bin4": (780, 830), "bin5": (1480, 1530), "bin6": (2950, 3050)}
_SUB = (6, 12, 24, 48, 100, 200)  # the sub-wave bins
_LARGE = (4097, 6145, 10241)  # the large path's chunk edges (kChunkRows = 2048)
_SUB_TARGETS = (6, 48, 200)
_NONE = np.zeros(0, np.int64)
STEPS_S = (3, 7, 11)  # seconds between the ticks after an update: resources with shorter leases lapse


@pytest.fixture(scope="module")
def eng():
    from doorman_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _sums(host):
    """The store's running sums on the host copy: exact sums of the rows, except that a
    sum a NaN entered stays NaN (store.go:156-158, see the module docstring)."""
    W.add_store_sums(host)
    R = len(host["kind"])
    for k in ("agg_sum_has", "agg_sum_wants"):
        stuck = host.setdefault("nan_" + k, np.zeros(R, bool))
        stuck |= np.isnan(host[k])
        host[k][stuck] = np.nan


def _copy(snap):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in snap.items()}


def _make_target(snap, r, rng, count):
    """Resource r as a target: FairShare, not learning, parent lease alive, live rows that
    outlive the test, three free rows for arrivals, and every live row hungry: it wants
    more than its equal share, so SumWants is well over the capacity.

    Why hungry.  A FairShare resource hands its whole capacity out, so after a disturbance
    some rows are cut to capacity - SumHas + has (algorithm.go:120): what they get is
    SumHas' rounding residue, and when many rows are cut at once the next SumHas carries
    that residue times their number.  With uneven grants an arrival that holds nothing,
    or a NaN wants (it fails every comparison of :131-204 and takes deservedShare +
    deservedExtra + deservedExtraExtra on top of a capacity already handed out in full),
    starts that on consecutive ticks, and no two implementations of the running sums,
    the reference's own included, then agree to 1e-9 of the capacity three ticks later.
    When every row wants more than its equal share nothing is left over to hand out
    (extra = 0): every row -- an arrival and a NaN row too -- gets its subclients' part of
    capacity / Count, and the residue is multiplied once at the most.  A new Count still
    moves every grant; a NaN refresh does not, but a target that k_general did not decide
    keeps its old expiry, which the ticks' advancing clock shows.  (The round-2 arithmetic
    on uneven grants is tests/test_general_gpu.py's subject; this file's is the routing.)"""
    so = snap["seg_off"]
    a, n = int(so[r]), int(so[r + 1] - so[r])
    snap["kind"][r] = W.FAIR_SHARE
    snap["learning_end_ns"][r] = W.INT64_MIN
    snap["parent_expiry_ns"][r] = W.INT64_MAX
    snap["capacity"][r] = 1000.0
    snap["lease_length_s"][r] = 300
    free = np.zeros(n, bool)
    free[[1, n // 2, n - 1]] = True
    w = rng.uniform(1.2, 3.0, n) * 1000.0 / (n - 3)
    w[free] = 0.0
    snap["wants"][a:a + n] = w
    snap["has"][a:a + n] = np.where(free, 0.0, rng.uniform(0.0, 1.0, n) * 1000.0 / n)
    snap["subclients"][a:a + n] = np.where(free, 0, count)
    snap["expiry_ns"][a:a + n] = np.where(free, W.RELEASED, NOW + rng.integers(100, 200, n) * W.NS)


_STORES = {}


def _store(count=1):
    """The shared store (built once per subclient count, handed out as copies): PER_BIN
    resources in each workgroup bin, the sub-wave bins, tiles, three large resources;
    ProportionalShare / FairShare, 2% free rows, 2% rows already expired, every live row
    with `count` subclients.  Returns (the snapshot to load, the host copy after two
    writeback ticks at NOW, the targets by class)."""
    if count not in _STORES:
        rng = np.random.default_rng(600 + count)
        sizes, cls = [], []
        for name, (lo, hi) in _BINS.items():
            sizes += list(rng.integers(lo, hi + 1, PER_BIN))
            cls += [name] * PER_BIN
        for n in _SUB:
            sizes += [n] * 4
            cls += ["sub"] * 4
        sizes += list(rng.integers(0, 5, 12)) + list(_LARGE)
        cls += ["tile"] * 12 + ["large"] * 3
        order = rng.permutation(len(sizes))
        sizes, cls = np.asarray(sizes, np.int64)[order], np.asarray(cls)[order]
        snap = snapshot_with_sizes(rng, sizes, kinds=(2, 3), expired_frac=0.02, learning_frac=0.0,
                                   parent_expired_frac=0.0)
        N = len(snap["wants"])
        free = rng.random(N) < 0.02
        snap["wants"][free] = 0.0
        snap["has"][free] = 0.0
        snap["subclients"] = np.where(free, 0, count).astype(np.int64)
        snap["expiry_ns"] = np.where(free, W.RELEASED, snap["expiry_ns"])
        targets = {name: [int(r) for r in np.flatnonzero(cls == name)[:2]] for name in _BINS}
        targets["sub"] = [int(np.flatnonzero((cls == "sub") & (sizes == n))[0]) for n in _SUB_TARGETS]
        targets["large"] = [int(r) for r in np.flatnonzero(cls == "large")]
        for rs in targets.values():
            for r in rs:
                _make_target(snap, r, rng, count)
        W.add_store_sums(snap)
        host = _copy(snap)
        for _ in range(2):
            _writeback_host(host, O.apportion(host, NOW))
            _sums(host)
        _STORES[count] = (snap, host, targets)
    snap, host, targets = _STORES[count]
    return _copy(snap), _copy(host), targets


def _rows(host, r, live):
    so = host["seg_off"]
    a, z = int(so[r]), int(so[r + 1])
    return a + np.flatnonzero((host["expiry_ns"][a:z] != W.RELEASED) == live)


def _assert_targets(host, tg, hetero=True):
    """Conditions of the scenario, from the host copy: each target has >= 2 live rows, they
    are heterogeneous (or hold a NaN wants) -- or, hetero=False, are not -- and the
    resource is contended: SumWants <= capacity is false (so it is for a NaN SumWants), no
    path that grants every row its wants applies."""
    for r in tg:
        rows = _rows(host, r, True)
        assert len(rows) >= 2, r
        s, w = host["subclients"][rows], host["wants"][rows]
        assert (s.min() != s.max() or bool(np.isnan(w).any())) == hetero, (r, s.min(), s.max())
        assert host["kind"][r] != W.FAIR_SHARE or host["learning_end_ns"][r] == W.INT64_MIN
        assert not host["agg_sum_wants"][r] <= host["capacity"][r], r


def _spec(step, route, host, tg, now, rng, count):
    """One update: the cause `step` on every target, and for the batch routes a round's
    ordinary traffic beside it (finite refreshes, departures, arrivals with the store's
    count on other resources)."""
    N, so = len(host["wants"]), host["seg_off"]
    batch = route == "apply" or route.startswith("async")
    on_target = np.zeros(N, bool)
    for r in tg:
        on_target[so[r]:so[r + 1]] = True
    alive = host["expiry_ns"] != W.RELEASED
    ref_rows, ref_vals, gone = np.zeros(0, np.int64), np.zeros(0), np.zeros(0, np.int64)
    rows, has, wants, sub, exp = _NONE, np.zeros(0), np.zeros(0), _NONE, _NONE
    if batch:
        others = np.flatnonzero(alive & ~on_target)
        ref_rows = others[::17]
        ref_vals = host["wants"][ref_rows] * rng.uniform(0.5, 1.5, len(ref_rows))
        gone = others[5::1001]
        rows = np.flatnonzero(~alive & ~on_target)[::7]
        wants = rng.uniform(0.1, 2.0, len(rows))
        has, sub = np.zeros(len(rows)), np.full(len(rows), count, np.int64)
        exp = np.full(len(rows), now + 600 * W.NS, np.int64)
    t_live = np.array([_rows(host, r, True)[1] for r in tg])  # the second live row of each target
    t_free = np.array([_rows(host, r, False)[0] for r in tg])  # its first free row
    k = len(tg)
    if step == "a" and route == "upsert":  # the refresh as a full Assign of the row
        rows, has, wants = t_live, host["has"][t_live], np.full(k, np.nan)
        sub, exp = host["subclients"][t_live], np.full(k, now + 600 * W.NS, np.int64)
    elif step == "a":
        ref_rows, ref_vals = np.concatenate([ref_rows, t_live]), np.concatenate([ref_vals, np.full(k, np.nan)])
    if step != "a":  # an arrival onto a free row of each target, hungry as the other rows (_make_target)
        n_sub = {"b": 3, "c": count, "d_same": count, "d_one": 1}[step]
        share = host["capacity"][tg] * n_sub / (host["agg_count"][tg] + n_sub)
        n_wants = np.full(k, np.nan) if step == "c" else share * rng.uniform(1.2, 3.0, k)
        rows, has = np.concatenate([rows, t_free]), np.concatenate([has, np.zeros(k)])
        wants = np.concatenate([wants, n_wants])
        sub = np.concatenate([sub, np.full(k, n_sub, np.int64)])
        exp = np.concatenate([exp, np.full(k, now + 600 * W.NS, np.int64)])
    o = np.argsort(ref_rows)  # the mask form takes its values in row order
    narrow = step == "c"  # has and expiry implied: 0, now + the resource's lease length
    if narrow:
        exp = now + host["lease_length_s"][np.searchsorted(so, rows, side="right") - 1] * W.NS
    return {"ref_rows": ref_rows[o], "ref_vals": ref_vals[o], "gone": gone, "new": (rows, has, wants, sub, exp),
            "narrow": narrow}


def _send(eng, route, sp, host, now):
    """The update through its route, and on the host copy."""
    N = len(host["wants"])
    rows, has, wants, sub, exp = sp["new"]
    if route == "rows":
        eng.update_wants(sp["ref_rows"], sp["ref_vals"])
    elif route == "mask":
        eng.update_wants_mask(W.rows_to_mask(sp["ref_rows"], N), sp["ref_vals"])
    elif route == "upsert":
        eng.upsert(rows, has, wants, sub, exp)
    else:
        ups = (rows, None, wants, sub.astype(np.int32), None) if sp["narrow"] else sp["new"]
        some = len(sp["ref_rows"]) > 0
        eng.apply(W.rows_to_mask(sp["ref_rows"], N) if some else None, sp["ref_vals"] if some else None,
                  sp["gone"] if len(sp["gone"]) else None, ups if len(rows) else None, now_ns=now,
                  asynchronous=route != "apply")
    _apply_host(host, sp["ref_rows"], sp["ref_vals"], sp["gone"], rows, has, wants, sub, exp)
    _sums(host)


def _tick(eng, host, now, shape, label):
    """One writeback tick in the given shape against the oracle on the host copy, which
    takes the tick.  "defer" reads nothing: the ticks' outcome is compared afterwards, in
    the store (each tick's has feeds the next)."""
    if shape == "defer":
        eng.apportion(now, writeback=True, asynchronous=True, defer_join=True)
        ref = O.apportion(host, now)
    else:
        eng.apportion(now, writeback=True, wb_columns="alternate" if shape == "alternate" else "auto")
        gets, exp = eng.leases()
        ref = O.apportion(host, now)
        assert_leases_match(host, gets, exp, ref, label)
    _writeback_host(host, ref)
    _sums(host)


def _clean_batch(eng, host, tg, rng, k):
    """An asynchronous batch that cannot make a store general: finite wants on a few live
    rows of other resources."""
    N, so = len(host["wants"]), host["seg_off"]
    ok = host["expiry_ns"] != W.RELEASED
    for r in tg:
        ok[so[r]:so[r + 1]] = False
    rows = np.flatnonzero(ok)[3 + k::29]
    vals = rng.uniform(0.1, 2.0, len(rows))
    eng.apply(W.rows_to_mask(rows, N), vals, asynchronous=True)
    _apply_host(host, rows, vals, *[_NONE] * 6)
    _sums(host)


ROUTES = ("rows", "mask", "upsert", "apply", "async_wait", "async_reuse", "async_cfg", "async_cfg_flip")
# Not every cause fits every route: a refresh (rows, mask) cannot change a count or land on
# a free row; arrivals with has and expiry implied exist in dm_store_batch only.
FITS = {"a": ROUTES, "b": ROUTES[2:], "c": ROUTES[3:], "d": ROUTES[2:]}
CELLS = [(c, r, s) for c in "abcd" for r in FITS[c] for s in ("sync", "defer", "alternate")]


@pytest.mark.parametrize("cause,route,shape", CELLS, ids=["-".join(c) for c in CELLS])
def test_update_that_turns_the_store_general(eng, cause, route, shape):
    """cause: (a) a NaN wants on a live row of each target, by refresh; (b) an arrival with
    3 subclients where the live rows have 1; (c) an arrival with has and expiry implied,
    the dense resource's own count and a NaN wants -- k_upsert keeps the resource dense,
    so the tick finds the NaN in the wants column alone; (d) a store with 2 subclients
    everywhere (all_sub_one false from the load) taking an arrival with 2 (homogeneous
    still: k_general runs on an empty worklist) and then one with 1.
    route: the single calls, dm_store_apply, and dm_store_apply_async with one tick
    enqueued while the batch is pending and the batch then retired by dm_store_apply_wait,
    by set reuse (two further batches), by dm_config_load with the same configuration, or
    by dm_config_load with one target flipped to ProportionalShare and back a tick later.
    shape: the three ticks after it -- synchronous, deferred-join back to back with
    nothing read, or the alternate columns (the large targets ran on the speculative
    chain in the ticks before the update)."""
    count = 2 if cause == "d" else 1
    snap, host, targets = _store(count)
    tg = [r for rs in targets.values() for r in rs]
    rng = np.random.default_rng(len(route) * 7 + ord(cause))
    cols = "alternate" if shape == "alternate" else "auto"
    eng.load(snap)
    for _ in range(2):  # the workgroup bins dense, no explicit expiry left, the chain speculative
        eng.apportion(NOW, writeback=True, wb_columns=cols)
    now = NOW
    eng.set_profiling(True)
    try:
        for step in {"d": ("d_same", "d_one")}.get(cause, (cause,)):
            label = f"{cause}/{route}/{shape}/{step}"
            eng.reset_kernel_times()
            ticks = 0
            _send(eng, route, _spec(step, route, host, tg, now, rng, count), host, now)
            _assert_targets(host, tg, hetero=step != "d_same")
            flip = None
            if route.startswith("async"):
                _tick(eng, host, now, shape, label + " (batch pending)")
                ticks += 1
                if route == "async_wait":
                    eng.apply_wait()
                elif route == "async_reuse":
                    for k in range(2):  # the second one reuses the cause's set and retires it
                        _clean_batch(eng, host, tg, rng, k)
                    eng.apply_wait()  # the clean batches: nothing pending keeps the ticks general
                elif route == "async_cfg":
                    eng.load_config(host)
                else:
                    flip = targets["bin5"][0]
                    host["kind"][flip] = W.PROPORTIONAL_SHARE
                    eng.load_config(host)
            for k, dt in enumerate(STEPS_S):
                now += dt * W.NS
                _tick(eng, host, now, shape, f"{label} tick {k}")
                ticks += 1
                if flip is not None and k == 0:
                    host["kind"][flip] = W.FAIR_SHARE
                    eng.load_config(host)
            eng.sync()
            _check(eng, host, label)
            _assert_targets(host, tg, hetero=step != "d_same")  # still so: no target lapsed
            assert eng.kernel_times().get("general", (0, 0))[0] >= ticks, (label, eng.kernel_times())
    finally:
        eng.set_profiling(False)


@pytest.mark.parametrize("name", ["bin4", "bin5", "bin6"])
def test_general_episode_there_and_back(eng, name):
    """The bins with more than 4 rows per lane keep arrival-mask entries that only a
    writeback tick with the arrivals bit in its hint clears; k_general resets the hint
    first, and k_release clears a row's arrival bit only while the resource is dense.
    So: a dense resource takes an arrival with its own count (arrival mask set), a NaN
    refresh on another row before the next tick, the tick (k_general), the release of the
    arrived row while the resource is not dense, the NaN row back to a finite wants, two
    ticks (dense again), an arrival onto another free row, two more ticks.  Every tick
    against the oracle; at the end the store equals the host copy and Count is exact -- a
    released row that came back through a stale arrival bit would show there."""
    snap, host, targets = _store(1)
    tg = targets[name]
    eng.load(snap)
    for _ in range(2):
        eng.apportion(NOW, writeback=True)
    assert eng.store_stats()["dense_resources"] >= 4 * PER_BIN
    free = np.array([_rows(host, r, False)[:2] for r in tg])
    nan_row = np.array([_rows(host, r, True)[1] for r in tg])
    now = NOW
    lease = host["lease_length_s"][np.asarray(tg)] * W.NS
    share = host["capacity"][tg] / host["agg_count"][tg]  # every row stays hungry (_make_target)

    def arrive(rows, wants):
        k = len(rows)
        eng.apply(upsert=(rows, None, wants, np.ones(k, np.int32), None), now_ns=now)
        _apply_host(host, _NONE, _NONE, _NONE, rows,np.zeros(k), wants, np.ones(k, np.int64), now + lease)
        _sums(host)

    def refresh(rows, wants):
        eng.update_wants(rows, wants)
        _apply_host(host, rows, wants, *[_NONE] * 6)
        _sums(host)

    eng.set_profiling(True)
    try:
        eng.reset_kernel_times()
        arrive(free[:, 0], 2.5 * share)
        refresh(nan_row, np.full(len(tg), np.nan))
        _assert_targets(host, tg)
        now += 5 * W.NS
        _tick(eng, host, now, "sync", f"{name}: the general tick")
        assert eng.kernel_times().get("general", (0, 0))[0] >= 1
    finally:
        eng.set_profiling(False)
    eng.release(free[:, 0])
    _apply_host(host, _NONE, _NONE, free[:, 0], *[_NONE] * 5)
    _sums(host)
    refresh(nan_row, 1.5 * share)
    for k in range(2):
        now += 5 * W.NS
        _tick(eng, host, now, "sync", f"{name}: back, tick {k}")
    arrive(free[:, 1], 2.0 * share)
    for k in range(2):
        now += 5 * W.NS
        _tick(eng, host, now, "sync", f"{name}: after the second arrival, tick {k}")
    _check(eng, host, name)
    for r, gone in zip(tg, free[:, 0]):
        assert host["expiry_ns"][gone] == W.RELEASED and host["agg_count"][r] == len(_rows(host, r, True))


def test_rejected_async_batch_surfaces_in_config_load(eng):
    """A rejected asynchronous batch (duplicate departure rows: its refresh stays applied,
    its departures and arrivals are not), then a valid one whose arrivals bring 3
    subclients, then dm_config_load: it retires both, returns the first one's error
    without loading, and the second batch's flags still count -- after a second, clean
    dm_config_load the next three ticks run k_general and match the oracle."""
    from doorman_amd._lib import DM_E_INVAL, DmError
    snap, host, targets = _store(1)
    tg = [r for rs in targets.values() for r in rs]
    rng = np.random.default_rng(17)
    N = len(host["wants"])
    eng.load(snap)
    for _ in range(2):
        eng.apportion(NOW, writeback=True)
    now = NOW
    bad = _spec("b", "async_cfg", host, tg, now, rng, 1)
    dup = np.concatenate([bad["gone"], bad["gone"][:1]])
    eng.apply(W.rows_to_mask(bad["ref_rows"], N), bad["ref_vals"], dup, bad["new"], asynchronous=True)
    _apply_host(host, bad["ref_rows"], bad["ref_vals"], *[_NONE] * 6)  # the refresh only
    _sums(host)
    _send(eng, "async_cfg", _spec("b", "async_cfg", host, tg, now, rng, 1), host, now)
    _assert_targets(host, tg)
    with pytest.raises(DmError) as e:
        eng.load_config(host)
    assert e.value.code == DM_E_INVAL and "earlier asynchronous batch" in str(e.value), str(e.value)
    assert "release" in str(e.value), str(e.value)
    eng.load_config(host)
    eng.set_profiling(True)
    try:
        eng.reset_kernel_times()
        for k, dt in enumerate(STEPS_S):
            now += dt * W.NS
            _tick(eng, host, now, "sync", f"after the rejected batch, tick {k}")
        _check(eng, host, "after the rejected batch")
        assert eng.kernel_times().get("general", (0, 0))[0] >= 3, eng.kernel_times()
    finally:
        eng.set_profiling(False)
    eng.apply_wait()  # nothing left in flight


def test_parts_store_taking_an_async_nan_refresh():
    """A store in stream parts (one workgroup bin of >= 4096 FairShare resources): a NaN
    refresh on resources of both halves arrives through dm_store_apply_async, and the
    deferred-join ticks behind it are enqueued back to back while the batch is pending
    (only async_may_general makes them general).  The parts stay."""
    import torch
    from doorman_amd.engine import Engine
    torch.cuda.set_device(0)
    rng = np.random.default_rng(98)
    sizes = rng.integers(513, 701, 4300)
    snap = snapshot_with_sizes(rng, sizes, kinds=(3,), expired_frac=0.02, learning_frac=0.0, parent_expired_frac=0.0)
    tg = [3, 100, 2400, 4200]
    for r in tg:
        _make_target(snap, r, rng, 1)
    W.add_store_sums(snap)
    host = _copy(snap)
    with Engine(0) as e:
        e.load(snap)
        assert e.plan_info()["stream_parts"] == 2
        for _ in range(2):
            e.apportion(NOW, writeback=True, asynchronous=True, defer_join=True)
            _writeback_host(host, O.apportion(host, NOW))
            _sums(host)
        now = NOW
        e.set_profiling(True)
        _send(e, "async_wait", _spec("a", "async_wait", host, tg, now, rng, 1), host, now)
        _assert_targets(host, tg)
        for k, dt in enumerate(STEPS_S):
            now += dt * W.NS
            _tick(e, host, now, "defer", f"parts tick {k}")
        e.sync()
        e.apply_wait()
        _check(e, host, "parts, NaN refresh in flight")
        assert e.plan_info()["stream_parts"] == 2
        assert e.kernel_times().get("general", (0, 0))[0] >= 3, e.kernel_times()
