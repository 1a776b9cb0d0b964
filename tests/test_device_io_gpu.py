"""The store loaded from and read into device memory (dm_store_load_device,
dm_read_store_device, dm_read_store_sums_device, dm_read_leases_device) against the host
calls they twin, on two engines of device 0.

Bars: whatever a host call reports, its device twin reports bit for bit (floats compared as
int64 bits); a device load leaves the state of a host load of the same values: the same
rows, sums, plan, byte-equal leases tick after tick and the same kernel classes launched
(which pins maybe_general and all_sub_one in both directions).  Against the oracle the
ticks keep parity_util's bars.  A rejected call leaves the store as it was.

The oracle's snapshot before every tick is read from engine A, the host-loaded one
(dm_read_store / dm_read_resources), so the model needs no copy of a tick's arithmetic.

Row-order sums: the snapshot holds -0.0, +Inf, 1e300 and 1e-300 in has and wants, next to
ordinary values whose sum depends on the order of the additions in its low bits.
"""
import ctypes

import numpy as np
import pytest

from doorman_amd import _lib
from doorman_amd import workloads as W
from oracle import oracle as O
from parity_util import REL_TOL, assert_leases_match, float_close, row_capacity, snapshot_with_sizes

pytestmark = pytest.mark.gpu
NOW = W.NOW_NS
# tests/test_relayout_gpu.py's sizes (empty segments, the tile / group bin boundary, the wave
# boundary, the chunk size, the 4096-row scan block, a resource over three scan blocks) and
# one resource of 20,000 rows: 313 steps of the wave-per-resource sum, the last one partial
SIZES = np.array([0, 1, 4, 5, 64, 65, 2048, 2049, 4095, 4096, 4097, 9000, 0, 3, 20000], np.int64)
ALL_RELEASED = 5    # the 65-row resource: every row released
HETERO = (4, 7, 11)  # FairShare resources with a few other subclient counts (64, 2049 and 9000 rows)
SPECIAL = {6: -0.0, 8: np.inf, 9: 1e300, 10: 1e-300, 14: 1e300, 3: -0.0}  # resource -> a value of some of its rows
COLS = ("has", "wants", "subclients", "expiry_ns")
SUMS = ("count", "sum_has", "sum_wants")
BIN_SLOTS = ("small_tiles", "sub16x4", "sub32x4", "wave64x4", "block128x4", "block128x8", "block256x8", "block2k4k",
             "sub8x2", "sub16x2", "large_resources", "large_chunks", "leases", "bin_shapes")
VARIANTS = ("mixed", "nan", "homogeneous")


@pytest.fixture(scope="module")
def engines():
    import torch  # noqa: F401  (before the library: one HIP runtime in the process)
    from doorman_amd.engine import Engine
    a, b = Engine(0), Engine(0)
    a.set_profiling(True)
    b.set_profiling(True)
    yield a, b
    a.close()
    b.close()


def _copy(snap):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in snap.items()}


_SNAPS = {}


def _snap(variant="mixed"):
    """The shared store (built once per variant, handed out as copies): every kind, ~15 %
    released rows scattered, one resource entirely released, 5 % rows already lapsed.
    mixed: a few other subclient counts in three FairShare resources; nan: that and one NaN
    wants in the 4097-row resource; homogeneous: every count 1, no NaN."""
    if variant not in _SNAPS:
        rng = np.random.default_rng(4242)
        snap = snapshot_with_sizes(rng, SIZES, kinds=(0, 1, 2, 3), expired_frac=0.05, learning_frac=0.1,
                                   parent_expired_frac=0.05)
        so, N = snap["seg_off"], len(snap["wants"])
        if variant != "homogeneous":
            for r in HETERO:
                snap["kind"][r] = W.FAIR_SHARE
                snap["learning_end_ns"][r] = W.INT64_MIN
                rows = so[r] + rng.choice(int(so[r + 1] - so[r]), 6, replace=False)
                snap["subclients"][rows] = rng.integers(2, 5, 6)
        for r, v in SPECIAL.items():
            k = min(5, int(so[r + 1] - so[r]))
            snap["has"][so[r] + rng.choice(int(so[r + 1] - so[r]), k, replace=False)] = v
            snap["wants"][so[r] + rng.choice(int(so[r + 1] - so[r]), k, replace=False)] = v
        free = rng.random(N) < 0.15
        free[so[ALL_RELEASED]:so[ALL_RELEASED + 1]] = True
        snap["wants"][free] = 0.0
        snap["has"][free] = 0.0
        snap["subclients"][free] = 0
        snap["expiry_ns"][free] = W.RELEASED
        if variant == "nan":
            row = so[10] + int(np.flatnonzero(~free[so[10]:so[11]])[7])
            snap["wants"][row] = np.nan
        for k in ("agg_count", "agg_sum_has", "agg_sum_wants"):
            snap.pop(k, None)
        _SNAPS[variant] = snap
    return _copy(_SNAPS[variant])


def _with_sums(snap):
    """Running sums that deliberately differ from the rows' sums (carried, not recomputed)."""
    W.add_store_sums(snap)
    snap["agg_count"] = snap["agg_count"] + (np.arange(len(SIZES)) % 3 == 0)
    snap["agg_sum_has"] = snap["agg_sum_has"] + 0.125
    snap["agg_sum_wants"] = snap["agg_sum_wants"] + 0.25
    return snap


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _np(t):
    return t.cpu().numpy()


def _dev(snap):
    """The store's columns of a snapshot as torch tensors on device 0."""
    import torch
    keys = ("seg_off",) + tuple(k for k in ("wants", "has", "subclients", "expiry_ns", "agg_count", "agg_sum_has",
                                              "agg_sum_wants") if snap.get(k) is not None)
    out = {k: torch.from_numpy(np.ascontiguousarray(snap[k])).to("cuda:0") for k in keys}
    torch.cuda.synchronize()
    return out


def _assert_same(got, want, keys, label):
    for k in keys:
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=f"{label}: {k} must be bit-identical")


def _state(eng):
    return eng.read_store(), eng.resources(safe=False)


def _oracle_snapshot(cfg, eng):
    """What the oracle starts a tick from: the configuration and the store as eng holds it."""
    st, res = _state(eng)
    post = {"seg_off": cfg["seg_off"], **st, **{k: cfg[k] for k in W.CFG_FIELDS}}
    post.update(agg_count=res["count"], agg_sum_has=res["sum_has"], agg_sum_wants=res["sum_wants"])
    return post


def _classes(eng):
    eng.sync()
    return set(eng.kernel_times())


# ---------------------------------------------------------------------------------------
# the device load leaves the state of a host load
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sums", ("sums given", "sums recomputed"))
@pytest.mark.parametrize("variant", VARIANTS)
def test_device_load_leaves_the_state_of_a_host_load(engines, variant, sums):
    A, B = engines
    snap = _snap(variant)
    if sums == "sums given":
        _with_sums(snap)
    label = f"{variant}/{sums}"
    A.load_store(snap)
    B.load_store_device(_dev(snap))
    assert (B.n_resources, B.n_leases) == (A.n_resources, A.n_leases) == (len(SIZES), int(SIZES.sum()))
    np.testing.assert_array_equal(B.seg_off, A.seg_off)
    sa, ra = _state(A)
    sb, rb = _state(B)
    _assert_same(sb, sa, COLS, label + " store")
    _assert_same(sb, snap, COLS, label + " store against the snapshot")
    _assert_same(rb, ra, SUMS, label + " running sums")
    if sums == "sums given":
        _assert_same(rb, {"count": snap["agg_count"], "sum_has": snap["agg_sum_has"], "sum_wants": snap["agg_sum_wants"]},
                     SUMS, label + " sums carried")
    pa, pb = A.plan_info(), B.plan_info()
    assert [pb[k] for k in BIN_SLOTS] == [pa[k] for k in BIN_SLOTS], label
    for eng in (A, B):  # a tick needs a configuration; leases_device none before it
        with pytest.raises(_lib.DmError) as e:
            eng.leases()
        assert e.value.code == _lib.DM_E_STATE
    A.load_config(snap)
    B.load_config(snap)
    now = NOW
    for tick, wb in enumerate((True, True, True, False)):
        now += 2 * W.NS
        ref_snap = _oracle_snapshot(snap, A)
        ref = O.apportion(ref_snap, now)
        A.reset_kernel_times()
        B.reset_kernel_times()
        A.apportion(now, writeback=wb)
        B.apportion(now, writeback=wb)
        ga, ea = A.leases()
        gb, eb = B.leases()
        tl = f"{label} tick {tick} writeback={wb}"
        np.testing.assert_array_equal(_bits(gb), _bits(ga), err_msg=tl + ": gets must be byte-equal")
        np.testing.assert_array_equal(eb, ea, err_msg=tl + ": expiry must be byte-equal")
        assert_leases_match(ref_snap, gb, eb, ref, tl)
        ca, cb = _classes(A), _classes(B)
        assert ca == cb, (tl, sorted(ca ^ cb))
        if variant == "homogeneous":
            assert "general" not in ca | cb, tl
        else:
            assert "general" in ca, tl
    assert not A.store_lost() and not B.store_lost()


# ---------------------------------------------------------------------------------------
# device reads equal host reads
# ---------------------------------------------------------------------------------------
def _update_round(eng, snap):
    """Releases, upserts and a mask refresh (the relayout test's round)."""
    rng = np.random.default_rng(11)
    st = eng.read_store()
    live = np.flatnonzero(st["expiry_ns"] != W.RELEASED)
    free = np.flatnonzero(st["expiry_ns"] == W.RELEASED)
    gone = rng.choice(live, 40, replace=False)
    keep = np.setdiff1d(live, gone)
    arrive = rng.choice(free, 40, replace=False)
    refresh = rng.choice(keep, 10, replace=False)
    up_rows = np.concatenate([arrive, refresh])
    masked = np.sort(rng.choice(np.setdiff1d(keep, refresh), len(keep) // 20, replace=False))
    eng.release(gone)
    eng.upsert(up_rows, np.concatenate([np.zeros(40), st["has"][refresh]]), rng.uniform(0.1, 50.0, 50),
               np.ones(50, np.int64), np.full(50, NOW + 600 * W.NS, np.int64))
    eng.update_wants_mask(W.rows_to_mask(masked, len(st["wants"])), rng.uniform(0.1, 50.0, len(masked)))
    narrow = np.setdiff1d(free, arrive)[::9][:30]  # arrivals without an expiry column
    eng.apply(upsert=(narrow, None, rng.uniform(0.1, 50.0, len(narrow)), np.ones(len(narrow), np.int32), None),
              now_ns=NOW + W.NS)


def _assert_reads_equal(eng, label, sums_want=None, leases=True):
    N, R = eng.n_leases, eng.n_resources
    for off, n in ((0, N), (2051, 9001), (4097, 0), (N, 0)):
        want = eng.read_store(off, n)
        got = {k: _np(v) for k, v in eng.read_store_device(off, n).items()}
        _assert_same(got, want, COLS, f"{label}: read_store_device({off}, {n})")
        part = eng.read_store_device(off, n, columns=("wants", "expiry_ns"))
        assert set(part) == {"wants", "expiry_ns"}
        _assert_same({k: _np(v) for k, v in part.items()}, want, ("wants", "expiry_ns"), f"{label}: two columns")
        part = eng.read_store_device(off, n, columns=("subclients",))
        _assert_same({k: _np(v) for k, v in part.items()}, want, ("subclients",), f"{label}: one column")
        if leases:
            g, e = eng.leases(off, n)
            dg, de = eng.leases_device(off, n)
            _assert_same({"gets": _np(dg), "expiry_ns": _np(de)}, {"gets": g, "expiry_ns": e}, ("gets", "expiry_ns"),
                         f"{label}: leases_device({off}, {n})")
            import torch
            only = torch.full((max(n, 1),), 7, dtype=torch.int64, device="cuda:0")  # expiry alone, gets NULL
            torch.cuda.synchronize()
            eng._chk(eng._L.dm_read_leases_device(eng._ctx, off, n, None, only.data_ptr()))
            np.testing.assert_array_equal(_np(only)[:n], e, err_msg=f"{label}: expiry alone")
    for r0, n in ((0, R), (3, 9), (5, 0), (R, 0)):
        want = ({k: sums_want[k][r0:r0 + n] for k in SUMS} if sums_want is not None
                else eng.resources(r0, n, safe=False))
        got = {k: _np(v) for k, v in eng.store_sums_device(r0, n).items()}
        _assert_same(got, want, SUMS, f"{label}: store_sums_device({r0}, {n})")
        part = eng.store_sums_device(r0, n, columns=("sum_has",))
        assert set(part) == {"sum_has"}
        _assert_same({k: _np(v) for k, v in part.items()}, want, ("sum_has",), f"{label}: sum_has alone")


def test_device_reads_equal_host_reads(engines):
    A, _ = engines
    snap = _snap("mixed")
    A.load_device(_dev(snap) | {k: snap[k] for k in W.CFG_FIELDS})
    _assert_reads_equal(A, "loaded", leases=False)
    A.apportion(NOW, writeback=True)
    _assert_reads_equal(A, "followers")
    _update_round(A, snap)
    _assert_reads_equal(A, "after updates", leases=False)
    before = A.resources(safe=False)  # the store's running sums: no tick's view stands in for them here
    A.apportion(NOW + 2 * W.NS, writeback=False)
    after = A.resources(safe=False)
    assert any((_bits(after[k]) != _bits(before[k])).any() for k in SUMS), "the plain tick's view should differ"
    _assert_reads_equal(A, "after a tick without writeback", sums_want=before)
    assert not A.store_lost()


# ---------------------------------------------------------------------------------------
# clone
# ---------------------------------------------------------------------------------------
def test_clone_store_to_another_engine(engines):
    A, B = engines
    snap = _snap("mixed")
    A.load(snap)
    A.apportion(NOW, writeback=True)
    _update_round(A, snap)
    A.apportion(NOW + 2 * W.NS, writeback=True)
    _update_round(A, snap)  # the mixed state: followers, released rows, arrivals with and without expiry, refreshes
    B.load(_snap("homogeneous"))  # whatever B held goes
    A.clone_store_to(B)
    sa, ra = _state(A)
    sb, rb = _state(B)
    _assert_same(sb, sa, COLS, "clone: store")
    _assert_same(rb, ra, SUMS, "clone: running sums")
    np.testing.assert_array_equal(B.seg_off, A.seg_off)
    B.load_config(snap)
    now = NOW + 9 * W.NS
    ref_snap = _oracle_snapshot(snap, A)
    ref = O.apportion(ref_snap, now)
    A.apportion(now, writeback=True)
    B.apportion(now, writeback=True)
    ga, ea = A.leases()
    gb, eb = B.leases()
    assert_leases_match(ref_snap, gb, eb, ref, "clone: B against the oracle")
    np.testing.assert_array_equal(eb, ea, err_msg="clone: expiry")
    ok = float_close(gb, ga, row_capacity(snap), REL_TOL)
    assert ok.all(), ("clone: gets of A and B", np.flatnonzero(~ok)[:10].tolist())
    assert not A.store_lost() and not B.store_lost()


# ---------------------------------------------------------------------------------------
# rejections
# ---------------------------------------------------------------------------------------
def _raw_load(eng, cols, R=None, N=None):
    """dm_store_load_device through the raw binding; cols: name -> tensor, or an int address."""
    s = _lib.Snapshot()
    s.n_resources = len(cols["seg_off"]) - 1 if R is None else R
    s.n_leases = len(cols["wants"]) if N is None else N
    for k, v in cols.items():
        setattr(s, k, v if isinstance(v, int) else (v.data_ptr() or None))
    return eng._L.dm_store_load_device(eng._ctx, ctypes.byref(s))


LOAD_REJECTIONS = ("subclients -1", "subclients 2^31-1", "seg_off not from 0", "seg_off decreasing",
                   "seg_off ending elsewhere", "two of three sums", "host pointer for a column",
                   "host pointer for seg_off", "columns missing")


@pytest.fixture(scope="module")
def held(engines):
    """Engine B holding a store with a tick's leases, and what it reports: the state every
    rejection must leave."""
    _, B = engines
    snap = _snap("mixed")
    B.load(snap)
    B.apportion(NOW, writeback=True)
    B.apportion(NOW + 2 * W.NS, writeback=False)
    return snap, _state(B), B.leases()


def _assert_untouched(B, held, label):
    snap, (st, res), (g, e) = held
    assert (B.n_leases, B.n_resources) == (len(st["wants"]), len(SIZES))
    sb, rb = _state(B)
    _assert_same(sb, st, COLS, label + ": store")
    _assert_same(rb, res, SUMS, label + ": sums")
    gb, eb = B.leases()  # the last tick's leases are still there ...
    _assert_same({"gets": gb, "expiry_ns": eb}, {"gets": g, "expiry_ns": e}, ("gets", "expiry_ns"), label + ": leases")
    B.apportion(NOW + 2 * W.NS, writeback=False)  # ... and the tick made again gives them again
    gb, eb = B.leases()
    _assert_same({"gets": gb, "expiry_ns": eb}, {"gets": g, "expiry_ns": e}, ("gets", "expiry_ns"), label + ": tick")
    assert not B.store_lost()


@pytest.mark.parametrize("case", LOAD_REJECTIONS)
def test_rejected_device_loads_leave_the_store_untouched(engines, held, case):
    import torch
    _, B = engines
    bad = _snap("mixed")
    keep = []  # host arrays whose address is passed: valid host memory of the column's size
    if case == "subclients -1":
        bad["subclients"][12345] = -1
    elif case == "subclients 2^31-1":
        bad["subclients"][len(bad["wants"]) - 1] = 2**31 - 1
    elif case == "seg_off not from 0":
        bad["seg_off"][0] = 1
    elif case == "seg_off decreasing":
        bad["seg_off"][5] = bad["seg_off"][4] - 1
    elif case == "seg_off ending elsewhere":
        bad["seg_off"][-1] -= 1
    elif case == "two of three sums":
        W.add_store_sums(bad)
        bad["agg_sum_has"] = None
    cols = _dev(bad)
    if case == "host pointer for a column":
        keep.append(np.ascontiguousarray(bad["wants"]))
        cols["wants"] = keep[-1].ctypes.data
    elif case == "host pointer for seg_off":
        keep.append(np.ascontiguousarray(bad["seg_off"]))
        cols["seg_off"] = keep[-1].ctypes.data
    elif case == "columns missing":
        cols["has"] = 0
    torch.cuda.synchronize()
    rc = _raw_load(B, cols, R=len(SIZES), N=len(bad["wants"]))
    assert rc == _lib.DM_E_INVAL, (case, rc, B._L.dm_last_error(B._ctx))
    _assert_untouched(B, held, case)


def test_rejected_device_reads(engines, held):
    """A host pointer for a destination: DM_E_INVAL from each read, nothing written to it; a
    range beyond the store: DM_E_RANGE; the store untouched."""
    import torch
    _, B = engines
    N, R = B.n_leases, B.n_resources
    host_f = np.full(64, 7.0)
    host_i = np.full(64, 7, np.int64)
    dev_f = torch.full((64,), 7.0, dtype=torch.float64, device="cuda:0")
    dev_i = torch.full((64,), 7, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    L, ctx = B._L, B._ctx
    hf, hi, df, di = host_f.ctypes.data, host_i.ctypes.data, dev_f.data_ptr(), dev_i.data_ptr()
    assert L.dm_read_store_device(ctx, 10, 64, hf, df, di, di) == _lib.DM_E_INVAL
    assert L.dm_read_store_device(ctx, 10, 64, df, df, di, hi) == _lib.DM_E_INVAL
    assert L.dm_read_store_sums_device(ctx, 0, R, di, hf, df) == _lib.DM_E_INVAL
    assert L.dm_read_leases_device(ctx, 10, 64, hf, di) == _lib.DM_E_INVAL
    assert L.dm_read_leases_device(ctx, 10, 64, df, hi) == _lib.DM_E_INVAL
    assert (host_f == 7.0).all() and (host_i == 7).all()
    assert (_np(dev_f) == 7.0).all() and (_np(dev_i) == 7).all(), "a rejected read wrote a destination"
    assert L.dm_read_store_device(ctx, N - 10, 64, df, None, None, None) == _lib.DM_E_RANGE
    assert L.dm_read_store_device(ctx, -1, 4, df, None, None, None) == _lib.DM_E_RANGE
    assert L.dm_read_store_sums_device(ctx, R - 1, 2, di, None, None) == _lib.DM_E_RANGE
    assert L.dm_read_leases_device(ctx, N, 1, df, None) == _lib.DM_E_RANGE
    _assert_untouched(B, held, "rejected reads")


def test_reads_without_a_store_or_a_tick_are_state_errors(engines):
    import torch
    from doorman_amd.engine import Engine
    dev_f = torch.zeros(8, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    with Engine(0) as e0:
        assert e0._L.dm_read_store_device(e0._ctx, 0, 0, None, None, None, None) == _lib.DM_E_STATE
        assert e0._L.dm_read_leases_device(e0._ctx, 0, 0, dev_f.data_ptr(), None) == _lib.DM_E_STATE
        e0.load_device(_dev(_snap("homogeneous")) | {k: _snap("homogeneous")[k] for k in W.CFG_FIELDS})
        with pytest.raises(_lib.DmError) as e:
            e0.leases_device()
        assert e.value.code == _lib.DM_E_STATE
        e0.apportion(NOW)
        g, x = e0.leases()
        dg, dx = e0.leases_device()
        _assert_same({"gets": _np(dg), "expiry_ns": _np(dx)}, {"gets": g, "expiry_ns": x}, ("gets", "expiry_ns"), "first tick")


# ---------------------------------------------------------------------------------------
# empty shapes, a batch in flight
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", (0, 3))
def test_empty_shapes(engines, R):
    """No rows, with and without resources: load, reads of nothing, a tick -- as the host load."""
    A, B = engines
    rng = np.random.default_rng(1)
    snap = snapshot_with_sizes(rng, np.zeros(R, np.int64), kinds=(3,))
    for k in ("agg_count", "agg_sum_has", "agg_sum_wants"):
        snap.pop(k, None)
    A.load(snap)
    B.load_device(_dev(snap) | {k: snap[k] for k in W.CFG_FIELDS})
    assert (B.n_resources, B.n_leases) == (R, 0)
    _assert_same(B.resources(safe=False), A.resources(safe=False), SUMS, f"R={R}: sums")
    assert all(len(v) == 0 for v in B.read_store_device(0, 0).values())
    got = {k: _np(v) for k, v in B.store_sums_device().items()}
    _assert_same(got, A.resources(safe=False), SUMS, f"R={R}: store_sums_device")
    assert [B.plan_info()[k] for k in BIN_SLOTS] == [A.plan_info()[k] for k in BIN_SLOTS]
    for wb in (True, False):
        A.apportion(NOW, writeback=wb)
        B.apportion(NOW, writeback=wb)
        g, e = B.leases_device(0, 0)
        assert len(g) == 0 and len(e) == 0
        _assert_same(B.resources(), A.resources(), SUMS, f"R={R}: tick")


def test_a_batch_in_flight_at_the_load_is_dropped(engines):
    """apply(asynchronous=True), then load_store_device: the new store is the snapshot's and
    the batch's outcome -- here a rejection -- is gone, as with dm_store_load."""
    _, B = engines
    first = _snap("homogeneous")
    B.load(first)
    rng = np.random.default_rng(3)
    live = np.flatnonzero(first["expiry_ns"] != W.RELEASED)
    masked = np.sort(rng.choice(live, 500, replace=False))
    B.apply(W.rows_to_mask(masked, len(first["wants"])), rng.uniform(0.1, 50.0, 500),
            release_rows=np.array([len(first["wants"]) + 5], np.int64), asynchronous=True)
    snap = _snap("mixed")
    B.load_store_device(_dev(snap))
    B.apply_wait()  # nothing left to retire: the rejected release went with the store it was sent to
    sb, rb = _state(B)
    _assert_same(sb, snap, COLS, "batch in flight: store")
    want = W.add_store_sums(_copy(snap))
    np.testing.assert_array_equal(rb["count"], want["agg_count"])
    B.load_config(snap)
    ref_snap = _oracle_snapshot(snap, B)
    B.apportion(NOW, writeback=True)
    g, e = B.leases()
    assert_leases_match(ref_snap, g, e, O.apportion(ref_snap, NOW), "batch in flight: tick")
