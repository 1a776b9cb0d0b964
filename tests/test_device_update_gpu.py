"""Store updates from device memory (dm_store_*_device, dm_store_apply_device[_async]) and the
dense wants refresh (dm_store_refresh_wants_device) against the host calls they twin, on two
engines of device 0: A is driven through the host calls, B through the device calls, both
from the same snapshot.

Bars: no tolerance of this file's own.  After a call, read_store(), resources(safe=False),
plan_info() and store_stats() of A and B are identical (floats as int64 bits); a writeback tick
and a plain tick follow, whose leases are byte-equal between A and B, within parity_util's
bars of the oracle started from A's state, and which launch the same kernel classes (that pins
maybe_general and all_sub_one in both directions).  A rejected call returns the twin's code
and message and leaves B as it was.

Exact sums: store updates add their deltas with atomics in an order that varies from run to
run, so every has and wants here -- in the store and in every update -- is a multiple of 2^-8
below 2^20: each delta and each partial sum is then exact and the running sums are bit-equal
whatever the order.  The specials (NaN, -0.0) go into cases of their own, whose sums are
compared with float_close.

plan_info is compared without three slots that are not the store's state: "queue_perm" and
"aux_own_queues" (a context's hardware queues, chosen by timing and by creation order) and
"kept_refreshes" (counted since dm_create; the keep-keys case compares its growth).
"""
import ctypes

import numpy as np
import pytest

from doorman_amd import _lib
from doorman_amd import workloads as W
from oracle import oracle as O
from parity_util import REL_TOL, assert_leases_match, float_close, snapshot_with_sizes

pytestmark = pytest.mark.gpu
NOW = W.NOW_NS
# tests/test_device_io_gpu.py's sizes: empty resources, runs of 64 rows that straddle resources,
# a resource over several waves (1024 rows each) and workgroups (4096 rows) of the refresh
# kernel, every bin
SIZES = np.array([0, 1, 4, 5, 64, 65, 2048, 2049, 4095, 4096, 4097, 9000, 0, 3, 20000], np.int64)
ALL_RELEASED = 5  # the 65-row resource: every row released
FAIR = (4, 7, 11)  # FairShare resources out of learning mode: other subclient counts / a NaN there need k_general
COLS = ("has", "wants", "subclients", "expiry_ns")
SUMS = ("count", "sum_has", "sum_wants")
PLAN_SKIP = ("queue_perm", "aux_own_queues", "kept_refreshes")
GRID = 256.0


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


def _grid(rng, n, lo=1):
    """n values on the grid: multiples of 2^-8 in [lo / 256, 2^12)."""
    return rng.integers(lo, 1 << 20, n).astype(np.float64) / GRID


_SNAP = []


def _snap():
    """The shared store (built once, handed out as copies): every kind, every value on the grid,
    about 15 % of the rows released and one resource entirely, 5 % of the rows lapsed, every
    subclients count 1, no NaN; the running sums are the load's (exact on the grid)."""
    if not _SNAP:
        rng = np.random.default_rng(777)
        snap = snapshot_with_sizes(rng, SIZES, kinds=(0, 1, 2, 3))
        so, N = snap["seg_off"], len(snap["wants"])
        snap["wants"], snap["has"] = _grid(rng, N, 0), _grid(rng, N, 0)
        for r in FAIR:
            snap["kind"][r] = W.FAIR_SHARE
            snap["learning_end_ns"][r] = W.INT64_MIN
        free = rng.random(N) < 0.15
        free[so[ALL_RELEASED]:so[ALL_RELEASED + 1]] = True
        snap["wants"][free] = 0.0
        snap["has"][free] = 0.0
        snap["subclients"][free] = 0
        snap["expiry_ns"][free] = W.RELEASED
        for k in ("agg_count", "agg_sum_has", "agg_sum_wants"):
            snap.pop(k, None)
        _SNAP.append(snap)
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _SNAP[0].items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _t(a, dtype=None):
    """A host array as a torch tensor on device 0 (uint64 words as their int64 bits)."""
    import torch
    a = np.ascontiguousarray(a, dtype)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    t = torch.from_numpy(a.copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _load(engines):
    A, B = engines
    snap = _snap()
    for e in (A, B):
        e.keep_keys(0)
        e.load(snap)
    return A, B, snap


def _state(e):
    plan = {k: v for k, v in e.plan_info().items() if k not in PLAN_SKIP}
    return e.read_store(), e.resources(safe=False), plan, e.store_stats()


def _assert_state(got, want, label, close_sums=False):
    (sg, rg, pg, tg), (sw, rw, pw, tw) = got, want
    for k in COLS:
        np.testing.assert_array_equal(_bits(sg[k]), _bits(sw[k]), err_msg=f"{label}: {k} must be bit-identical")
    np.testing.assert_array_equal(rg["count"], rw["count"], err_msg=f"{label}: count")
    for k in ("sum_has", "sum_wants"):
        if close_sums:  # a case with NaN or -0.0 in it: the order of the atomics may show in the last bit
            ok = float_close(rg[k], rw[k], np.maximum(np.abs(rw[k]), 1.0), REL_TOL)
            assert ok.all(), (label, k, np.flatnonzero(~ok)[:10].tolist())
        else:
            np.testing.assert_array_equal(_bits(rg[k]), _bits(rw[k]), err_msg=f"{label}: {k} must be bit-identical")
    assert pg == pw, (label, {k: (pg[k], pw[k]) for k in pg if pg[k] != pw[k]})
    assert tg == tw, (label, tg, tw)


def _same(A, B, label, close_sums=False):
    _assert_state(_state(B), _state(A), label, close_sums)


def _follow(A, B, snap, label, general=None, close_sums=False, ticks=(True, False)):
    """The state of A and B compared, then a writeback tick and a plain tick: byte-equal leases,
    the oracle from A's state, the same kernel classes (general: whether k_general must be among
    them)."""
    _same(A, B, label, close_sums)
    now = NOW
    for wb in ticks:
        now += 2 * W.NS
        st, res = A.read_store(), A.resources(safe=False)
        ref_snap = {"seg_off": snap["seg_off"], **st, **{k: snap[k] for k in W.CFG_FIELDS}}
        ref_snap.update(agg_count=res["count"], agg_sum_has=res["sum_has"], agg_sum_wants=res["sum_wants"])
        ref = O.apportion(ref_snap, now)
        for e in (A, B):
            e.reset_kernel_times()
            e.apportion(now, writeback=wb)
        ga, ea = A.leases()
        gb, eb = B.leases()
        tl = f"{label}: tick writeback={wb}"
        np.testing.assert_array_equal(_bits(gb), _bits(ga), err_msg=tl + ": gets must be byte-equal")
        np.testing.assert_array_equal(eb, ea, err_msg=tl + ": expiry must be byte-equal")
        assert_leases_match(ref_snap, gb, eb, ref, tl)
        A.sync(), B.sync()
        ca, cb = set(A.kernel_times()), set(B.kernel_times())
        assert ca == cb, (tl, sorted(ca ^ cb))
        if general is not None:
            assert ("general" in ca) == general, (tl, sorted(ca))
    assert not A.store_lost() and not B.store_lost()


def _rows(snap, rng, n_live, n_free=0, within=None):
    """Distinct live rows and free rows of the snapshot (within: of one resource)."""
    so = snap["seg_off"]
    idx = np.arange(len(snap["wants"])) if within is None else np.arange(so[within], so[within + 1])
    live = idx[snap["expiry_ns"][idx] != W.RELEASED]
    free = idx[snap["expiry_ns"][idx] == W.RELEASED]
    return rng.choice(live, n_live, replace=False), rng.choice(free, n_free, replace=False)


def _mask_of(rows, N, first_row=0, nwords=None):
    nwords = (N - first_row + 63) // 64 if nwords is None else nwords
    return W.rows_to_mask(rows, nwords * 64, first_row)


def _upsert_args(snap, rng, n_live, n_free, sub=None):
    live, free = _rows(snap, rng, n_live, n_free)
    rows = np.concatenate([free, live])
    n = len(rows)
    sub = np.ones(n, np.int64) if sub is None else sub
    return rows, _grid(rng, n), _grid(rng, n), sub, np.full(n, NOW + 600 * W.NS, np.int64)


def _batch(snap, rng, narrow, parts=("refresh", "release", "upsert"), n=300):
    """One round's host columns: a masked refresh, departures and arrivals over disjoint rows."""
    N = len(snap["wants"])
    live, free = _rows(snap, rng, 3 * n, n)
    ref, gone, again = np.sort(live[:n]), live[n:2 * n], live[2 * n:]
    kw = {}
    if "refresh" in parts:
        kw.update(wants_mask=_mask_of(ref, N), wants=_grid(rng, n))
    if "release" in parts:
        kw.update(release_rows=gone)
    if "upsert" in parts:
        rows = np.concatenate([free, again])
        m = len(rows)
        if narrow:
            kw.update(upsert=(rows, None, _grid(rng, m), np.ones(m, np.int32), None), now_ns=NOW + W.NS)
        else:
            kw.update(upsert=(rows, _grid(rng, m), _grid(rng, m), np.ones(m, np.int64),
                              np.full(m, NOW + 600 * W.NS, np.int64)))
    return kw


def _dev_batch(kw):
    out = dict(kw)
    for k in ("wants_mask", "wants", "release_rows"):
        if k in out:
            out[k] = _t(out[k])
    if "upsert" in out:
        out["upsert"] = tuple(None if c is None else _t(c) for c in out["upsert"])
    return out


# ---------------------------------------------------------------------------------------
# each single call and the batch against its twin
# ---------------------------------------------------------------------------------------
CALLS = ("upsert", "upsert other subclients", "update_wants", "update_wants nan", "update_wants_mask", "release",
         "batch", "batch narrow")


@pytest.mark.parametrize("call", CALLS)
def test_each_call_against_its_twin(engines, call):
    A, B, snap = _load(engines)
    rng = np.random.default_rng(31)
    general, close = False, False
    if call.startswith("upsert"):
        args = _upsert_args(snap, rng, 200, 200)
        if call == "upsert other subclients":  # all_sub_one falls, the tick prepares for k_general
            live, _ = _rows(snap, rng, 6, within=FAIR[2])
            args = (live, _grid(rng, 6), _grid(rng, 6), rng.integers(2, 5, 6), np.full(6, NOW + 600 * W.NS, np.int64))
            general = True
        A.upsert(*args)
        B.upsert_device(*[_t(a) for a in args])
    elif call.startswith("update_wants") and call != "update_wants_mask":
        rows, _ = _rows(snap, rng, 500, within=FAIR[2])
        vals = _grid(rng, 500)
        if call == "update_wants nan":
            vals[17] = np.nan
            general, close = True, True
        A.update_wants(rows, vals)
        B.update_wants_device(_t(rows), _t(vals))
    elif call == "update_wants_mask":
        rows, _ = _rows(snap, rng, 5000)
        rows = np.sort(rows)
        mask, vals = _mask_of(rows, len(snap["wants"])), _grid(rng, 5000)
        A.update_wants_mask(mask, vals)
        B.update_wants_mask_device(_t(mask), _t(vals))
    elif call == "release":
        rows, _ = _rows(snap, rng, 400)
        A.release(rows)
        B.release_device(_t(rows))
    else:
        kw = _batch(snap, rng, narrow=call == "batch narrow")
        A.apply(**kw)
        B.apply_device(**_dev_batch(kw))
    _follow(A, B, snap, call, general=general, close_sums=close)


# ---------------------------------------------------------------------------------------
# sizes that cross the steps
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 64, 65))
def test_row_calls_of_n_rows(engines, n):
    A, B, snap = _load(engines)
    rng = np.random.default_rng(100 + n)
    live, free = _rows(snap, rng, 3 * n, n)
    up = (np.concatenate([free, live[:n]]), _grid(rng, 2 * n), _grid(rng, 2 * n), np.ones(2 * n, np.int64),
          np.full(2 * n, NOW + 600 * W.NS, np.int64))
    A.upsert(*up)
    B.upsert_device(*[_t(a) for a in up])
    vals = _grid(rng, n)
    A.update_wants(live[n:2 * n], vals)
    B.update_wants_device(_t(live[n:2 * n]), _t(vals))
    A.release(live[2 * n:])
    B.release_device(_t(live[2 * n:]))
    _follow(A, B, snap, f"n={n}", general=False, ticks=(True,))


@pytest.mark.parametrize("where", ("whole store, ending mid-word", "first_row 64", "the last aligned word"))
def test_masks_at_the_edges(engines, where):
    A, B, snap = _load(engines)
    N = len(snap["wants"])
    assert N % 64 not in (0, 63)  # the store ends mid-word
    rng = np.random.default_rng(7)
    live = np.flatnonzero(snap["expiry_ns"] != W.RELEASED)
    if where == "whole store, ending mid-word":
        first, rows = 0, np.union1d(rng.choice(live, 900, replace=False), live[-3:])
    elif where == "first_row 64":
        first, rows = 64, live[(live >= 64) & (live < 64 + 130)]
    else:
        first = N // 64 * 64
        rows = live[live >= first]
    assert len(rows) > 0
    nwords = (int(rows.max()) - first) // 64 + 1
    mask, vals = _mask_of(rows, N, first, nwords), _grid(rng, len(rows))
    A.update_wants_mask(mask, vals, first_row=first)
    B.update_wants_mask_device(_t(mask), _t(vals), first_row=first)
    _follow(A, B, snap, where, general=False, ticks=(True,))


@pytest.mark.parametrize("empty", ("refresh", "release", "upsert"))
@pytest.mark.parametrize("narrow", (False, True))
def test_batches_with_a_part_empty(engines, empty, narrow):
    A, B, snap = _load(engines)
    kw = _batch(snap, np.random.default_rng(5), narrow, parts=tuple(p for p in ("refresh", "release", "upsert") if p != empty),
                n=70)
    A.apply(**kw)
    B.apply_device(**_dev_batch(kw))
    _follow(A, B, snap, f"batch without {empty}, narrow={narrow}", general=False, ticks=(True,))


# ---------------------------------------------------------------------------------------
# rejections
# ---------------------------------------------------------------------------------------
def _raises(fn):
    with pytest.raises(_lib.DmError) as e:
        fn()
    return e.value.code, str(e.value)


REJECTIONS = ("row >= N", "row < 0", "duplicate row", "subclients 2^31-1", "n != popcount", "mask bit past the end",
              "release row >= N")


@pytest.mark.parametrize("case", REJECTIONS)
def test_rejections_are_the_twins(engines, case):
    A, B, snap = _load(engines)
    N = len(snap["wants"])
    rng = np.random.default_rng(9)
    before = _state(B)
    rows, _ = _rows(snap, rng, 100)
    vals = _grid(rng, 100)
    if case in ("row >= N", "row < 0"):
        rows[41] = N if case == "row >= N" else -1
        host, dev = (lambda: A.update_wants(rows, vals)), (lambda: B.update_wants_device(_t(rows), _t(vals)))
        code = _lib.DM_E_RANGE
    elif case == "release row >= N":
        rows[99] = N + 7
        host, dev = (lambda: A.release(rows)), (lambda: B.release_device(_t(rows)))
        code = _lib.DM_E_RANGE
    elif case in ("duplicate row", "subclients 2^31-1"):
        sub = np.ones(100, np.int64)
        if case == "duplicate row":
            rows[70] = rows[3]
        else:
            sub[5] = 2**31 - 1
        args = (rows, vals, vals, sub, np.full(100, NOW + 600 * W.NS, np.int64))
        host, dev = (lambda: A.upsert(*args)), (lambda: B.upsert_device(*[_t(a) for a in args]))
        code = _lib.DM_E_INVAL
    elif case == "n != popcount":
        mask = _mask_of(np.sort(rows), N)
        host = lambda: A.update_wants_mask(mask, vals[:99])
        dev = lambda: B.update_wants_mask_device(_t(mask), _t(vals[:99]))
        code = _lib.DM_E_INVAL
    else:
        mask = _mask_of(np.sort(rows), N)
        mask[-1] |= np.uint64(1) << np.uint64(63)  # row 64 nwords - 1 >= N: the store ends mid-word
        host = lambda: A.update_wants_mask(mask, np.append(vals, 1.0))
        dev = lambda: B.update_wants_mask_device(_t(mask), _t(np.append(vals, 1.0)))
        code = _lib.DM_E_RANGE
    ca, ma = _raises(host)
    cb, mb = _raises(dev)
    assert (cb, mb) == (ca, ma) and ca == code, (case, ca, ma, cb, mb)
    _assert_state(_state(B), before, case + ": B untouched")
    _same(A, B, case)


def test_a_part_rejected_inside_a_batch(engines):
    """The release names a row past the end: the refresh before it is applied, the arrivals
    behind it are not, in B as in A; the code and message are the twin's."""
    A, B, snap = _load(engines)
    kw = _batch(snap, np.random.default_rng(12), narrow=False)
    kw["release_rows"] = np.append(kw["release_rows"], len(snap["wants"]))
    before = B.read_store()
    ca, ma = _raises(lambda: A.apply(**kw))
    cb, mb = _raises(lambda: B.apply_device(**_dev_batch(kw)))
    assert (cb, mb) == (ca, ma) and ca == _lib.DM_E_RANGE and "release: " in mb, (ca, ma, cb, mb)
    _same(A, B, "rejected part")
    after = B.read_store()
    assert (_bits(after["wants"]) != _bits(before["wants"])).sum() > 0, "the refresh before the rejected part is applied"
    up = kw["upsert"][0]
    np.testing.assert_array_equal(_bits(after["has"][up]), _bits(before["has"][up]), err_msg="arrivals not applied")
    np.testing.assert_array_equal(after["expiry_ns"], before["expiry_ns"], err_msg="no release, no arrival")


def test_host_pointers_and_short_tensors_are_refused(engines):
    """At the ctypes level: a numpy (host) pointer for any column, and a count the tensor's
    allocation cannot hold: DM_E_INVAL, nothing launched, B untouched."""
    A, B, snap = _load(engines)
    N = len(snap["wants"])
    before = _state(B)
    L, ctx = B._L, B._ctx
    rng = np.random.default_rng(2)
    rows, _ = _rows(snap, rng, 64)
    vals = _grid(rng, 64)
    sub, exp = np.ones(64, np.int64), np.full(64, NOW + 600 * W.NS, np.int64)
    sub32 = sub.astype(np.int32)
    mask = _mask_of(np.sort(rows), N)
    dr, dv, ds, de, dm = _t(rows), _t(vals), _t(sub), _t(exp), _t(mask)
    hr, hv, hm = rows.ctypes.data, vals.ctypes.data, mask.ctypes.data
    pr, pv, ps, pe, pm = (t.data_ptr() for t in (dr, dv, ds, de, dm))
    INV = _lib.DM_E_INVAL
    assert L.dm_store_update_wants_device(ctx, 64, hr, pv) == INV
    assert L.dm_store_update_wants_device(ctx, 64, pr, hv) == INV
    assert b"not device memory" in L.dm_last_error(ctx)
    assert L.dm_store_upsert_device(ctx, 64, pr, pv, hv, ps, pe) == INV
    assert L.dm_store_upsert_device(ctx, 64, pr, pv, pv, ps, exp.ctypes.data) == INV
    assert L.dm_store_release_device(ctx, 64, hr) == INV
    assert L.dm_store_update_wants_mask_device(ctx, 0, len(mask), hm, 64, pv) == INV
    assert L.dm_store_update_wants_mask_device(ctx, 0, len(mask), pm, 64, hv) == INV
    assert L.dm_store_refresh_wants_device(ctx, 0, 64, hv, None) == INV
    for fn in (L.dm_store_apply_device, L.dm_store_apply_device_async):
        b = _lib.StoreBatch()
        b.release_n, b.release_rows = 64, hr
        assert fn(ctx, ctypes.byref(b)) == INV
        b = _lib.StoreBatch()
        b.wants_nwords, b.wants_mask, b.wants_n, b.wants = len(mask), pm, 64, hv
        assert fn(ctx, ctypes.byref(b)) == INV
        b = _lib.StoreBatch()
        b.upsert_n, b.upsert_rows, b.upsert_wants, b.upsert_subclients32 = 64, pr, pv, sub32.ctypes.data
        b.upsert_now_ns = NOW
        assert fn(ctx, ctypes.byref(b)) == INV
    B.apply_wait()  # nothing was enqueued
    # A tensor shorter than n: 2^28 packed values (2 GiB) from a 64-entry tensor.  Asked of the
    # masked forms only, whose kernels never read a packed value when the count differs from
    # the mask's set bits: were the check ever to let the pointer through, nothing would be
    # read out of bounds.
    big = 1 << 28
    assert L.dm_store_update_wants_mask_device(ctx, 0, len(mask), pm, big, pv) == INV
    assert b"does not hold" in L.dm_last_error(ctx)
    b = _lib.StoreBatch()
    b.wants_nwords, b.wants_mask, b.wants_n, b.wants = len(mask), pm, big, pv
    assert L.dm_store_apply_device(ctx, ctypes.byref(b)) == INV
    assert b"does not hold" in L.dm_last_error(ctx)
    _assert_state(_state(B), before, "refused pointers: B untouched")
    _same(A, B, "refused pointers")


BAD_MASK = "bad masked update (first_row must be a multiple of 64)"
NO_MASK = "packed values without a mask"
PAST_END = "mask words past the store's end"


def _scalar_faults(W1):
    """(call, arguments, code, message) of the argument checks that the host runs before it
    looks at a pointer.  A letter stands for a valid column (host memory for the host call,
    device memory for its twin; upper case: host memory for both); W1: the mask words of the
    whole store.  Single calls take their arguments in the C order; a batch is the fields that
    differ from an empty one."""
    INV, RNG, OK = _lib.DM_E_INVAL, _lib.DM_E_RANGE, _lib.DM_OK
    up = ("r", "h", "w", "s", "e")
    yield "upsert", (-1,) + up, INV, "bad upsert"
    for k in range(5):
        yield "upsert", (64,) + up[:k] + (None,) + up[k + 1:], INV, "bad upsert"
    yield "upsert", (0, "R", "H", "W", "S", "E"), OK, None
    yield "update_wants", (-1, "r", "w"), INV, "bad update"
    yield "update_wants", (64, None, "w"), INV, "bad update"
    yield "update_wants", (64, "r", None), INV, "bad update"
    yield "update_wants", (0, "R", "W"), OK, None
    yield "release", (-1, "r"), INV, "bad release"
    yield "release", (64, None), INV, "bad release"
    yield "release", (0, "R"), OK, None
    # (first_row, nwords, mask, n, wants)
    yield "update_wants_mask", (0, W1, "m", -1, "w"), INV, BAD_MASK
    yield "update_wants_mask", (0, W1, None, 64, "w"), INV, BAD_MASK
    yield "update_wants_mask", (0, W1, "m", 64, None), INV, BAD_MASK
    yield "update_wants_mask", (-64, 1, "m", 64, "w"), INV, BAD_MASK
    yield "update_wants_mask", (32, 1, "m", 64, "w"), INV, BAD_MASK
    yield "update_wants_mask", (0, -1, "m", 0, "w"), INV, BAD_MASK
    yield "update_wants_mask", (0, 0, "m", 64, "w"), INV, NO_MASK
    yield "update_wants_mask", (0, W1 + 1, "m", 64, "w"), RNG, PAST_END
    yield "update_wants_mask", (0, 0, "M", 0, "W"), OK, None
    for k in ("wants_nwords", "wants_n", "release_n", "upsert_n"):
        yield "apply", {k: -1}, INV, "negative batch sizes"
    yield "apply", dict(release_n=64), INV, "bad release"
    arrivals = dict(upsert_n=64, upsert_rows="r", upsert_has="h", upsert_wants="w", upsert_subclients="s",
                    upsert_expiry_ns="e")
    for k in ("upsert_rows", "upsert_wants", "upsert_subclients"):
        yield "apply", {**arrivals, k: None}, INV, "bad upsert"
    refresh = dict(wants_first_row=0, wants_nwords=W1, wants_mask="m", wants_n=64, wants="w")
    yield "apply", {**refresh, "wants_mask": None}, INV, BAD_MASK
    yield "apply", {**refresh, "wants": None}, INV, BAD_MASK
    yield "apply", {**refresh, "wants_first_row": -64, "wants_nwords": 1}, INV, BAD_MASK
    yield "apply", {**refresh, "wants_first_row": 32, "wants_nwords": 1}, INV, BAD_MASK
    yield "apply", {**refresh, "wants_nwords": 0}, INV, NO_MASK
    yield "apply", {**refresh, "wants_nwords": W1 + 1}, RNG, PAST_END
    yield "apply", dict(wants_mask="M", wants="W", release_rows="R", upsert_rows="R", upsert_wants="W"), OK, None


def test_scalar_argument_checks_are_the_twins(engines):
    """The argument checks that come before the pointer checks, through ctypes on both twins
    with the same scalars: the same code and dm_last_error text on both, equal to the table
    above; with nothing to do the device twin returns DM_OK before it looks at a pointer (host
    pointers pass); neither store changes."""
    A, B, snap = _load(engines)
    N = len(snap["wants"])
    W1 = (N + 63) // 64
    before = _state(A), _state(B)
    host = {"r": np.arange(64, dtype=np.int64), "h": np.full(64, 2.0), "w": np.full(64, 3.0),
            "s": np.ones(64, np.int64), "e": np.full(64, NOW + 600 * W.NS, np.int64), "m": np.zeros(W1 + 1, np.uint64)}
    dev = {k: _t(v) for k, v in host.items()}
    hp = {k: v.ctypes.data for k, v in host.items()}
    ptrs = {False: {**hp, **{k.upper(): p for k, p in hp.items()}},
            True: {**{k: t.data_ptr() for k, t in dev.items()}, **{k.upper(): p for k, p in hp.items()}}}
    wrong = []
    for call, args, code, msg in _scalar_faults(W1):
        got = []
        for e, device in ((A, False), (B, True)):
            fn = getattr(e._L, f"dm_store_{call}_device" if device else f"dm_store_{call}")
            if call == "apply":
                b = _lib.StoreBatch()
                for k, v in args.items():
                    setattr(b, k, ptrs[device].get(v, v) if isinstance(v, str) else v)
                rc = fn(e._ctx, ctypes.byref(b))
            else:
                rc = fn(e._ctx, *[ptrs[device][a] if isinstance(a, str) else a for a in args])
            got.append((rc, e._L.dm_last_error(e._ctx).decode() if rc != _lib.DM_OK else None))
        print(call, args, got)
        if got != [(code, msg)] * 2:
            wrong.append((call, args, got, (code, msg)))
    assert not wrong, wrong
    _assert_state(_state(A), before[0], "refused scalars: A untouched")
    _assert_state(_state(B), before[1], "refused scalars: B untouched")


# ---------------------------------------------------------------------------------------
# asynchronous device batches
# ---------------------------------------------------------------------------------------
def _rounds(snap, k, n=120):
    """k rounds over disjoint rows, so that each is valid whatever was applied before it."""
    rng = np.random.default_rng(77)
    N = len(snap["wants"])
    live, free = _rows(snap, rng, 3 * n * k, n * k)
    out = []
    for i in range(k):
        lv, fr = live[3 * n * i:3 * n * (i + 1)], free[n * i:n * (i + 1)]
        rows = np.concatenate([fr, lv[2 * n:]])
        out.append(dict(wants_mask=_mask_of(np.sort(lv[:n]), N), wants=_grid(rng, n), release_rows=lv[n:2 * n],
                        upsert=(rows, _grid(rng, 2 * n), _grid(rng, 2 * n), np.ones(2 * n, np.int64),
                                np.full(2 * n, NOW + 600 * W.NS, np.int64))))
    return out


@pytest.mark.parametrize("route", ("device", "alternated"))
def test_asynchronous_rounds_back_to_back(engines, route):
    A, B, snap = _load(engines)
    for i, kw in enumerate(_rounds(snap, 5)):
        A.apply(**kw)
        if route == "device" or i % 2 == 0:
            B.apply_device(asynchronous=True, **_dev_batch(kw))
        else:
            B.apply(asynchronous=True, **kw)
    B.apply_wait()
    _follow(A, B, snap, f"five asynchronous rounds ({route})", general=None, ticks=(True,))


def test_a_rejected_asynchronous_device_batch_is_reported_late(engines):
    A, B, snap = _load(engines)
    good = _rounds(snap, 2)
    bad = dict(release_rows=np.array([len(snap["wants"]) + 5], np.int64))
    B.apply_device(asynchronous=True, **_dev_batch(bad))
    B.apply_device(asynchronous=True, **_dev_batch(good[0]))  # enqueued behind it, applied
    code, msg = _raises(lambda: B.apply_device(asynchronous=True, **_dev_batch(good[1])))  # retires the first
    assert code == _lib.DM_E_RANGE and "an earlier asynchronous batch's release: row out of range" in msg, (code, msg)
    B.apply_wait()
    A.apply(**good[0])  # the retiring call enqueued nothing
    _same(A, B, "late rejection")
    B.apply_device(asynchronous=True, **_dev_batch(bad))
    code, msg = _raises(B.apply_wait)
    assert code == _lib.DM_E_RANGE and "an earlier asynchronous batch" in msg, (code, msg)
    _same(A, B, "late rejection by apply_wait")


def test_a_device_batch_in_flight_at_a_load_is_dropped(engines):
    A, B, snap = _load(engines)
    kw = _rounds(snap, 1)[0]
    kw["release_rows"] = np.array([len(snap["wants"]) + 5], np.int64)
    B.apply_device(asynchronous=True, **_dev_batch(kw))
    B.load_store(snap)
    B.apply_wait()  # nothing left to retire: the rejection went with the store it was sent to
    B.load_config(snap)
    _same(A, B, "batch in flight at a load")


# ---------------------------------------------------------------------------------------
# the dense refresh
# ---------------------------------------------------------------------------------------
def _dense_case(A, snap, rng, density, first, n):
    """A new wants column for rows [first, first + n) of A's store: about `density` of the
    entries differ from the stored bits (on the grid), released rows included, which get
    garbage besides.  Returns (column, the live rows that differ)."""
    st = A.read_store()
    cur, live = st["wants"][first:first + n], st["expiry_ns"][first:first + n] != W.RELEASED
    pick = np.ones(n, bool) if density >= 1.0 else rng.random(n) < density
    new = cur.copy()
    new[pick] = cur[pick] + rng.integers(1, 1 << 10, int(pick.sum())) / GRID
    new[~live & (rng.random(n) < 0.5)] = 12345.5
    differ = _bits(new) != _bits(cur)
    return new, first + np.flatnonzero(live & differ)


@pytest.mark.parametrize("span", ("whole store", "sub-range"))
@pytest.mark.parametrize("density", (0.0, 0.01, 0.5, 1.0))
def test_dense_refresh_against_the_mask_form(engines, density, span):
    A, B, snap = _load(engines)
    N = len(snap["wants"])
    first, n = (0, N) if span == "whole store" else (2048, 4097 + 17)
    rng = np.random.default_rng(int(density * 100) + first)
    new, rows = _dense_case(A, snap, rng, density, first, n)
    if density == 0.0:
        assert len(rows) == 0
    nwords = (n + 63) // 64
    A.update_wants_mask(_mask_of(rows, N, first, nwords), new[rows - first], first_row=first)
    got = B.refresh_wants_device(_t(new), first_row=first)
    assert got == len(rows), (got, len(rows))
    sb = B.read_store()
    freed = sb["expiry_ns"] == W.RELEASED
    assert (sb["wants"][freed] == 0.0).all() and (sb["subclients"][freed] == 0).all(), "released rows stay zero"
    np.testing.assert_array_equal(freed, snap["expiry_ns"] == W.RELEASED)
    _follow(A, B, snap, f"dense refresh {density} {span}", general=False, ticks=(True,))


def test_dense_refresh_keeps_the_keys_of_untouched_resources():
    """(b) a column equal to the stored one writes nothing and keeps every key; (c) one changed
    row in each of three resources clears exactly the keys of the workgroup-bin resources among
    them and counts as one kept refresh, as the mask form does on A; the next tick is
    byte-equal.  The store and its fixed point: tests/test_keep_keys_gpu.py's."""
    import torch  # noqa: F401
    from test_keep_keys_gpu import R_SMALL, Pair, make_store
    snap, under, _ = make_store()
    P = Pair(snap, under, keep=True)
    try:
        P.A.keep_keys(True)  # A in the same mode: it is driven through the host mask form
        items = P.engage()
        assert items > 0
        stored = P.B.read_store()["wants"]
        kept0 = P.B.keep_stats()["kept_refreshes"]
        assert P.B.refresh_wants_device(_t(stored)) == 0
        assert P.B.store_stats()["fixed_items"] == items, "an unchanged column keeps every key"
        P.same("unchanged column", leases=False)
        assert P.B.keep_stats()["kept_refreshes"] == kept0 + 1
        # (c)
        ka, kb = P.A.keep_stats()["kept_refreshes"], P.B.keep_stats()["kept_refreshes"]
        targets = [under[0], under[4], R_SMALL]
        keyed = [r for r in targets if P.valid()[r]]
        assert len(keyed) == 2, (targets, keyed)
        # ascending, as the mask form takes its packed values (row 5 of the small resource is live)
        rows = np.sort(np.array([P.off[r] + 5 for r in targets], np.int64))
        assert (P.host["expiry_ns"][rows] != W.RELEASED).all()
        vals = stored[rows] * 0.5 + 2.0 ** -10
        new = stored.copy()
        new[rows] = vals
        P.A.update_wants_mask(W.rows_to_mask(rows, len(stored)), vals)
        assert P.B.refresh_wants_device(_t(new)) == 3
        P.same("three changed rows", leases=False)
        for e in (P.A, P.B):
            assert e.store_stats()["fixed_items"] == items - len(keyed), (e.store_stats(), items, keyed)
        assert P.A.keep_stats()["kept_refreshes"] == ka + 1 and P.B.keep_stats()["kept_refreshes"] == kb + 1
        P.host["wants"][rows] = vals
        W.add_store_sums(P.host)
        P.tick("the tick after the dense refresh", 8)
    finally:
        P.close()


def test_dense_refresh_nan_and_negative_zero(engines):
    """(d) a changed NaN has the twin's consequences (no kept refresh, k_general), a NaN already
    stored with equal bits is no change; (e) -0.0 over +0.0 is one."""
    A, B, snap = _load(engines)
    N = len(snap["wants"])
    rng = np.random.default_rng(8)
    (row, zero), _ = _rows(snap, rng, 2, within=FAIR[2])
    for e in (A, B):
        e.keep_keys(1)
        e.update_wants(np.array([zero]), np.array([0.0]))
    k0 = (A.keep_stats()["kept_refreshes"], B.keep_stats()["kept_refreshes"])
    new = A.read_store()["wants"]
    new[row] = np.nan
    A.update_wants_mask(_mask_of([row], N), np.array([np.nan]))
    assert B.refresh_wants_device(_t(new)) == 1
    assert (A.keep_stats()["kept_refreshes"], B.keep_stats()["kept_refreshes"]) == k0, "a NaN refresh is not kept"
    _same(A, B, "changed NaN", close_sums=True)
    assert B.refresh_wants_device(_t(new)) == 0, "the stored NaN, bit for bit, is no change"
    assert B.keep_stats()["kept_refreshes"] == k0[1] + 1
    _same(A, B, "stored NaN again", close_sums=True)
    new[zero] = -0.0
    A.update_wants_mask(_mask_of([zero], N), np.array([-0.0]))
    assert B.refresh_wants_device(_t(new)) == 1, "-0.0 over +0.0 is a change"
    assert _bits(B.read_store()["wants"])[zero] == np.int64(-2**63)
    for e in (A, B):
        e.keep_keys(0)
    _follow(A, B, snap, "NaN and -0.0", general=True, close_sums=True)


def test_dense_refresh_errors(engines):
    import torch
    from doorman_amd.engine import Engine
    A, B, snap = _load(engines)
    N = len(snap["wants"])
    before = _state(B)
    col = _t(np.full(N, 3.0))
    L, ctx = B._L, B._ctx
    n = ctypes.c_int64(-1)
    assert L.dm_store_refresh_wants_device(ctx, 64, N - 63, col.data_ptr(), ctypes.byref(n)) == _lib.DM_E_RANGE
    assert L.dm_store_refresh_wants_device(ctx, N // 64 * 64 + 64, 1, col.data_ptr(), None) == _lib.DM_E_RANGE
    assert L.dm_store_refresh_wants_device(ctx, 32, 64, col.data_ptr(), None) == _lib.DM_E_INVAL
    assert L.dm_store_refresh_wants_device(ctx, -64, 64, col.data_ptr(), None) == _lib.DM_E_INVAL
    assert L.dm_store_refresh_wants_device(ctx, 0, -1, col.data_ptr(), None) == _lib.DM_E_INVAL
    assert L.dm_store_refresh_wants_device(ctx, 0, 64, None, None) == _lib.DM_E_INVAL
    assert n.value == -1, "a refused call writes no count"
    assert L.dm_store_refresh_wants_device(ctx, 0, 0, None, ctypes.byref(n)) == _lib.DM_OK and n.value == 0
    _assert_state(_state(B), before, "refused dense refreshes: B untouched")
    with Engine(0) as e0:
        code, _ = _raises(lambda: e0.refresh_wants_device(col))
        assert code == _lib.DM_E_STATE
        code, _ = _raises(lambda: e0.release_device(_t(np.array([0]))))
        assert code == _lib.DM_E_STATE
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------
# Engine argument checks
# ---------------------------------------------------------------------------------------
def test_engine_argument_checks(engines):
    """ValueError before any library call (the store stays as it was) for a CPU tensor, a wrong
    dtype, a non-contiguous view and mismatched lengths."""
    import torch
    A, B, snap = _load(engines)
    before = _state(B)
    rows, vals = _t(np.arange(8)), _t(np.full(8, 2.0))
    wide = _t(np.full(16, 2.0))
    with pytest.raises(ValueError):
        B.update_wants_device(rows, torch.full((8,), 2.0, dtype=torch.float64))
    with pytest.raises(ValueError):
        B.update_wants_device(rows, vals.to(torch.float32))
    with pytest.raises(ValueError):
        B.update_wants_device(rows, wide[::2])
    with pytest.raises(ValueError):
        B.update_wants_device(rows, wide)
    with pytest.raises(ValueError):
        B.refresh_wants_device(wide[::2])
    with pytest.raises(ValueError):
        B.release_device(rows.to(torch.int32))
    with pytest.raises(ValueError):
        B.apply_device(release_rows=rows.cpu())
    with pytest.raises(ValueError):
        B.upsert_device(rows, vals, vals, rows, _t(np.arange(7)))
    _assert_state(_state(B), before, "argument checks: B untouched")
