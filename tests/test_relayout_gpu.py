"""dm_store_relayout on the GPU: the device store re-laid out in HBM (resources grow,
shrink, are compacted or appended) against the host route it replaces -- dm_read_store of
every row, the permutation in numpy, dm_store_load with the running sums as aggregates --
and against the CPU oracle on the permuted snapshot.

Bars: the four store columns, the running sums and the row map bit-exact; the ticks that
follow under parity_util's bars (expiries and counts exact, capacities within REL_TOL x
max(|ref|, capacity)).

The state a re-layout starts from is read back from the device (dm_read_store /
dm_read_resources resolve the column encoding and return the running sums as the device
holds them), so the model below needs no copy of the update kernels' arithmetic: it
permutes what the device reported.
"""
import numpy as np
import pytest

from doorman_amd import _lib
from doorman_amd import workloads as W
from oracle import oracle as O
from parity_util import assert_leases_match, assert_resources_match, snapshot_with_sizes

pytestmark = pytest.mark.gpu
NOW = W.NOW_NS
# empty segments, the tile / group bin boundary (4 / 5), the wave boundary, the chunk size
# (2048), the 4096-row scan block and kLargeMin, a resource over three scan blocks, segment
# starts off the block boundaries
SIZES = np.array([0, 1, 4, 5, 64, 65, 2048, 2049, 4095, 4096, 4097, 9000, 0, 3], np.int64)
ALL_RELEASED = 5   # the 65-row resource: every row released
HETERO = (4, 7, 11)  # resources with a few other subclient counts (64, 2049 and 9000 rows)
COLS = ("has", "wants", "subclients", "expiry_ns")
RELAYOUTS = ("grow", "shrink_to_fit", "append_resources", "compact_tight", "compact_grow")
STATES = ("loaded", "followers", "mixed", "async")


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
    """The shared store (built once, handed out as copies): every kind, ~15% released rows
    scattered, 5% rows already expired, a few heterogeneous subclient counts, one resource
    with every row released."""
    if not _SNAP:
        rng = np.random.default_rng(707)
        snap = snapshot_with_sizes(rng, SIZES, kinds=(0, 1, 2, 3), expired_frac=0.05, learning_frac=0.1,
                                   parent_expired_frac=0.05)
        so, N = snap["seg_off"], len(snap["wants"])
        for r in HETERO:
            snap["kind"][r] = W.FAIR_SHARE
            snap["learning_end_ns"][r] = W.INT64_MIN
            rows = so[r] + rng.choice(int(so[r + 1] - so[r]), 6, replace=False)
            snap["subclients"][rows] = rng.integers(2, 5, 6)
        free = rng.random(N) < 0.15
        free[so[ALL_RELEASED]:so[ALL_RELEASED + 1]] = True
        snap["wants"][free] = 0.0
        snap["has"][free] = 0.0
        snap["subclients"][free] = 0
        snap["expiry_ns"][free] = W.RELEASED
        W.add_store_sums(snap)
        _SNAP["s"] = snap
    return _copy(_SNAP["s"])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _assert_same_store(got, want, label):
    for k in COLS:
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=f"{label}: {k} must be bit-identical")


def _prepare(eng, state):
    """Bring eng's store into `state`; returns the configuration snapshot it runs under."""
    snap = _snap()
    eng.load(snap)
    if state == "loaded":
        return snap
    eng.apportion(NOW, writeback=True)  # every live row a follower, lapsed rows released
    if state == "followers":
        return snap
    rng = np.random.default_rng(11)
    st = eng.read_store()
    live = np.flatnonzero(st["expiry_ns"] != W.RELEASED)
    free = np.flatnonzero(st["expiry_ns"] == W.RELEASED)
    so = snap["seg_off"]
    gone = rng.choice(live, 40, replace=False)
    keep = np.setdiff1d(live, gone)
    arrive = rng.choice(free, 40, replace=False)
    refresh = rng.choice(keep, 10, replace=False)
    up_rows = np.concatenate([arrive, refresh])
    up = (up_rows, np.concatenate([np.zeros(40), st["has"][refresh]]), rng.uniform(0.1, 50.0, 50),
          np.ones(50, np.int64), np.full(50, NOW + 600 * W.NS, np.int64))
    masked = np.sort(rng.choice(np.setdiff1d(keep, refresh), len(keep) // 20, replace=False))
    mask, mw = W.rows_to_mask(masked, len(st["wants"])), rng.uniform(0.1, 50.0, len(masked))
    if state == "mixed":
        eng.release(gone)
        eng.upsert(*up)
        eng.update_wants_mask(mask, mw)
        # arrivals as a round sends them (no expiry column: now + the lease length), which a
        # dense resource takes into its arrival mask
        narrow = np.setdiff1d(free, arrive)[::9][:30]
        eng.apply(upsert=(narrow, None, rng.uniform(0.1, 50.0, len(narrow)), np.ones(len(narrow), np.int32), None),
                  now_ns=NOW + W.NS)
    else:  # the same round as one asynchronous batch, not yet retired when the re-layout is called
        eng.apply(mask, mw, gone, up, asynchronous=True)
    assert so[-1] == len(st["wants"])
    return snap


def _state_of(eng):
    """The store as the device reports it: the four columns and the running sums."""
    st = eng.read_store()
    res = eng.resources(safe=False)
    return st, res


def _new_sizes(kind, st, old_off):
    sizes = np.diff(old_off)
    live = st["expiry_ns"] != W.RELEASED
    nlive = np.array([int(live[a:z].sum()) for a, z in zip(old_off[:-1], old_off[1:])], np.int64)
    last = np.array([(int(np.flatnonzero(live[a:z])[-1]) + 1) if live[a:z].any() else 0
                     for a, z in zip(old_off[:-1], old_off[1:])], np.int64)
    if kind == "grow":
        return 2 * sizes + 1, False
    if kind == "shrink_to_fit":
        return last, False
    if kind == "append_resources":
        return np.concatenate([sizes + 1, [7, 0, 300]]), False
    if kind == "compact_tight":
        return nlive, True
    if kind == "compact_grow":
        return 2 * nlive + 3, True
    raise ValueError(kind)


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _model(st, old_off, new_off, compact):
    """dm_store_relayout in numpy: the permuted columns and the row map."""
    R, Nn = len(old_off) - 1, int(new_off[-1])
    out = {"has": np.zeros(Nn), "wants": np.zeros(Nn), "subclients": np.zeros(Nn, np.int64),
           "expiry_ns": np.full(Nn, W.RELEASED, np.int64)}
    row_map = np.full(int(old_off[-1]), -1, np.int64)
    for r in range(R):
        a, z, nlen = int(old_off[r]), int(old_off[r + 1]), int(new_off[r + 1] - new_off[r])
        if compact:
            src = a + np.flatnonzero(st["expiry_ns"][a:z] != W.RELEASED)
        else:
            src = np.arange(a, min(z, a + nlen))
        assert len(src) <= nlen
        dst = int(new_off[r]) + np.arange(len(src))
        for k in COLS:
            out[k][dst] = st[k][src]
        row_map[src] = dst
    return out, row_map


def _post_snapshot(cfg, st, res, old_off, sizes, compact):
    """The snapshot the host route would load: the permuted rows under the new layout, the
    running sums carried (zero for appended resources), the configuration extended."""
    new_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cols, row_map = _model(st, old_off, new_off, compact)
    R, Rn = len(old_off) - 1, len(sizes)
    post = {"seg_off": new_off, **cols}
    fill = {"kind": W.FAIR_SHARE, "capacity": 500.0, "lease_length_s": 60, "refresh_interval_s": 5,
            "learning_end_ns": W.INT64_MIN, "parent_expiry_ns": W.INT64_MAX, "safe_capacity": np.nan}
    for k in W.CFG_FIELDS:
        post[k] = np.concatenate([cfg[k], np.full(Rn - R, fill[k], cfg[k].dtype)])
    post["agg_count"] = np.concatenate([res["count"], np.zeros(Rn - R, np.int64)])
    post["agg_sum_has"] = np.concatenate([res["sum_has"], np.zeros(Rn - R)])
    post["agg_sum_wants"] = np.concatenate([res["sum_wants"], np.zeros(Rn - R)])
    return post, row_map


def _assert_sums_carried(eng, post, label):
    res = eng.resources(safe=False)
    np.testing.assert_array_equal(res["count"], post["agg_count"], err_msg=f"{label}: count")
    np.testing.assert_array_equal(_bits(res["sum_has"]), _bits(post["agg_sum_has"]), err_msg=f"{label}: sum_has")
    np.testing.assert_array_equal(_bits(res["sum_wants"]), _bits(post["agg_sum_wants"]), err_msg=f"{label}: sum_wants")


def _assert_ticks_match(eng, post, now, label):
    """A plain tick, then a writeback tick, against the oracle on the permuted snapshot."""
    ref = O.apportion(post, now)
    for wb in (False, True):
        eng.apportion(now, writeback=wb)
        gets, exp = eng.leases()
        assert_leases_match(post, gets, exp, ref, f"{label} writeback={wb}")
        assert_resources_match(post, eng.resources(), ref, f"{label} writeback={wb}")
    assert not eng.store_lost()


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("relayout", RELAYOUTS)
def test_relayout_equals_the_host_route(engines, relayout, state):
    """Context A is re-laid out on the device; context B loads what the host route builds
    from A's rows.  (The asynchronous state's batch is still to be retired when the call
    is made; its kernels have run, since the state is read from A first.)"""
    A, B = engines
    cfg = _prepare(A, state)
    st, res = _state_of(A)
    old_off = A.seg_off.copy()
    sizes, compact = _new_sizes(relayout, st, old_off)
    post, want_map = _post_snapshot(cfg, st, res, old_off, sizes, compact)
    label = f"{relayout}/{state}"

    row_map = A.relayout(post["seg_off"], compact=compact, want_row_map=True)
    np.testing.assert_array_equal(row_map, want_map, err_msg=f"{label}: row map")
    assert A.n_leases == len(post["wants"]) and A.n_resources == len(sizes)
    B.load_store(post)
    B.load_config(post)
    got = A.read_store()
    _assert_same_store(got, B.read_store(), label + " (A against B)")
    _assert_same_store(got, post, label + " (A against the model)")
    _assert_sums_carried(A, post, label)
    if len(sizes) != len(old_off) - 1:  # the configuration is stale until one is loaded for the new count
        with pytest.raises(_lib.DmError) as e:
            A.apportion(NOW + 7 * W.NS)
        assert e.value.code == _lib.DM_E_STATE
        A.load_config(post)
    _assert_ticks_match(A, post, NOW + 7 * W.NS, label)


def test_relayout_without_a_row_map_and_back(engines):
    """NULL row map; a grow followed by the shrink back restores the first layout's store."""
    A, _ = engines
    cfg = _prepare(A, "followers")
    st, res = _state_of(A)
    old_off = A.seg_off.copy()
    grown, _ = _new_sizes("grow", st, old_off)
    assert A.relayout(np.concatenate([[0], np.cumsum(grown)])) is None
    assert A.relayout(old_off) is None
    _assert_same_store(A.read_store(), st, "grow and back")
    post, _ = _post_snapshot(cfg, st, res, old_off, np.diff(old_off), False)
    _assert_sums_carried(A, post, "grow and back")
    _assert_ticks_match(A, post, NOW + 7 * W.NS, "grow and back")


REJECTIONS = ("default shrink dropping a live row", "compact one short", "decreasing seg_off", "seg_off[0] != 0",
              "n_resources < R", "rejected asynchronous batch pending")


@pytest.mark.parametrize("case", REJECTIONS)
def test_rejected_relayouts_leave_the_store_untouched(engines, case):
    """The stated code, then: dm_read_store and the running sums bit-identical to before, a
    tick that still matches the oracle, the store not lost."""
    A, _ = engines
    cfg = _prepare(A, "followers")
    st, res = _state_of(A)
    old_off = A.seg_off.copy()
    sizes = np.diff(old_off)
    same, _ = _post_snapshot(cfg, st, res, old_off, sizes, False)
    live = st["expiry_ns"] != W.RELEASED
    nlive = np.array([int(live[a:z].sum()) for a, z in zip(old_off[:-1], old_off[1:])], np.int64)
    last, _ = _new_sizes("shrink_to_fit", st, old_off)
    victim = 8  # the 4095-row resource
    assert last[victim] > 1 and nlive[victim] > 1
    compact, word = False, None
    if case == "default shrink dropping a live row":
        drop = sizes.copy()
        drop[victim] = last[victim] - 1  # one short of its last live row
        off, code, word = _off(drop), _lib.DM_E_RANGE, f"resource {victim}"
    elif case == "compact one short":
        short = 2 * nlive + 3
        short[victim] = nlive[victim] - 1  # one short of its live count
        off, code, word, compact = _off(short), _lib.DM_E_RANGE, f"resource {victim}", True
    elif case == "decreasing seg_off":
        off, code, word = old_off.copy(), _lib.DM_E_INVAL, "non-decreasing"
        off[5] = off[4] - 1
    elif case == "seg_off[0] != 0":
        off, code, word = old_off.copy(), _lib.DM_E_INVAL, "start at 0"
        off[0] = 1
    elif case == "n_resources < R":
        off, code, word = old_off[:-1], _lib.DM_E_INVAL, "n_resources"
    else:  # the batch's error is returned, and nothing is re-laid
        A.apply(release_rows=np.array([len(st["wants"]) + 5], np.int64), asynchronous=True)
        off, code, word = _off(2 * sizes + 1), _lib.DM_E_RANGE, "asynchronous batch"
    with pytest.raises(_lib.DmError) as e:
        A.relayout(off, compact=compact, want_row_map=True)
    assert e.value.code == code, str(e.value)
    assert word in str(e.value), str(e.value)
    assert A.n_leases == len(st["wants"]) and A.n_resources == len(sizes)
    _assert_same_store(A.read_store(), st, case)
    _assert_sums_carried(A, same, case)
    _assert_ticks_match(A, same, NOW + 7 * W.NS, case)
    if case == "rejected asynchronous batch pending":  # ... and the call made again goes through
        _prepare(A, "followers")
        A.apply(release_rows=np.array([len(st["wants"]) + 5], np.int64), asynchronous=True)
        with pytest.raises(_lib.DmError):
            A.relayout(off)
        A.relayout(off)
        assert A.n_leases == int(off[-1])


def test_relayout_without_a_store_is_a_state_error():
    from doorman_amd.engine import Engine
    with Engine(0) as e0:
        with pytest.raises(_lib.DmError) as e:
            e0.relayout(np.array([0, 4], np.int64))
        assert e.value.code == _lib.DM_E_STATE


def test_config_is_kept_while_the_resource_count_stays(engines):
    """With R unchanged a tick runs without reloading the configuration (the appended case,
    DM_E_STATE until dm_config_load, is asserted in test_relayout_equals_the_host_route)."""
    A, _ = engines
    cfg = _prepare(A, "loaded")
    st, res = _state_of(A)
    old_off = A.seg_off.copy()
    sizes, _ = _new_sizes("grow", st, old_off)
    post, _ = _post_snapshot(cfg, st, res, old_off, sizes, False)
    A.relayout(post["seg_off"])
    got = A.config()
    for k in W.CFG_FIELDS:
        np.testing.assert_array_equal(got[k], cfg[k], err_msg=k)
    _assert_ticks_match(A, post, NOW + 7 * W.NS, "config kept")


def test_resource_count_is_fixed_while_a_publish_ring_is_bound(engines):
    """A ring's blocks hold 1 + R records: appending resources is DM_E_STATE and leaves the
    store alone; a re-layout that keeps R goes through and the next writeback tick still
    publishes every resource's {SumWants, Count}."""
    import ctypes

    import torch
    A, _ = engines
    cfg = _prepare(A, "followers")
    st, res = _state_of(A)
    old_off = A.seg_off.copy()
    R = len(old_off) - 1
    bufs = [torch.zeros((1 + R, 2), dtype=torch.float64, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    ring = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in bufs])
    A._chk(A._L.dm_publish_ring(A._ctx, 3, ring))
    try:
        more, _ = _new_sizes("append_resources", st, old_off)
        with pytest.raises(_lib.DmError) as e:
            A.relayout(_off(more))
        assert e.value.code == _lib.DM_E_STATE
        same, _ = _post_snapshot(cfg, st, res, old_off, np.diff(old_off), False)
        _assert_same_store(A.read_store(), st, "ring bound")
        _assert_sums_carried(A, same, "ring bound")
        sizes, _ = _new_sizes("grow", st, old_off)
        post, _ = _post_snapshot(cfg, st, res, old_off, sizes, False)
        A.relayout(post["seg_off"])
        now = NOW + 7 * W.NS
        ref = O.apportion(post, now)
        A.apportion(now, writeback=True)  # the ring's first tick: bufs[0]
        gets, exp = A.leases()
        assert_leases_match(post, gets, exp, ref, "ring bound")
        after = A.resources(safe=False)
        block = bufs[0].cpu().numpy()
        np.testing.assert_array_equal(_bits(block[1:, 0]), _bits(after["sum_wants"]))
        np.testing.assert_array_equal(_bits(block[1:, 1]), after["count"])
    finally:
        A._chk(A._L.dm_publish_ring(A._ctx, 0, None))


def test_small_heterogeneous_resources_growing_into_the_bins(engines):
    """Resources of the small tiles (which decide any rows themselves) holding other
    subclient counts or a NaN wants, on a store whose load found nothing for k_general:
    grown past the tiles they need it, and the ticks after the re-layout still decide them."""
    A, _ = engines
    rng = np.random.default_rng(9)
    sizes = np.array([3, 4, 4, 2, 40], np.int64)
    snap = snapshot_with_sizes(rng, sizes, kinds=(3,), expired_frac=0.0, learning_frac=0.0, parent_expired_frac=0.0)
    snap["capacity"][:] = 100.0
    snap["wants"][:] = rng.uniform(30.0, 90.0, int(sizes.sum()))  # contended: SumWants > capacity
    snap["subclients"][:11] = [1, 2, 3, 1, 1, 4, 2, 5, 5, 5, 1]   # resources 0-2 heterogeneous
    snap["wants"][12] = np.nan                                    # resource 3: a NaN wants
    W.add_store_sums(snap)
    A.load(snap)
    st, res = _state_of(A)
    new_sizes = np.array([12, 16, 5, 8, 40], np.int64)
    post, _ = _post_snapshot(snap, st, res, A.seg_off.copy(), new_sizes, False)
    A.relayout(post["seg_off"])
    _assert_same_store(A.read_store(), post, "small heterogeneous")
    _assert_ticks_match(A, post, NOW + W.NS, "small heterogeneous")


def test_repeated_growth_walks_every_bin(engines):
    """One resource doubled from 3 rows to 6144 (the tiles, every sub-wave and workgroup
    bin, the large chain: eleven doublings), a writeback tick and an arrival onto a new
    free row between the steps, the oracle at every step."""
    A, _ = engines
    rng = np.random.default_rng(4)
    sizes = np.array([3, 10, 300], np.int64)
    snap = snapshot_with_sizes(rng, sizes, kinds=(2, 3), expired_frac=0.0, learning_frac=0.0, parent_expired_frac=0.0)
    snap["lease_length_s"][:] = 300
    snap["capacity"][0] = 1000.0
    A.load(snap)
    now = NOW
    bins_seen = set()
    while sizes[0] <= 4096:
        st, res = _state_of(A)
        old_off = A.seg_off.copy()
        old_n = int(sizes[0])
        sizes = sizes.copy()
        sizes[0] *= 2
        post, want_map = _post_snapshot(snap, st, res, old_off, sizes, False)
        label = f"growth to {int(sizes[0])}"
        np.testing.assert_array_equal(A.relayout(post["seg_off"], want_row_map=True), want_map, err_msg=label)
        _assert_same_store(A.read_store(), post, label)
        _assert_sums_carried(A, post, label)
        info = A.plan_info()
        bins_seen |= {k for k in ("small_tiles", "sub16x4", "sub32x4", "wave64x4", "block128x4", "block128x8",
                                  "block256x8", "block2k4k", "sub8x2", "sub16x2", "large_resources") if info[k] > 0}
        now += 2 * W.NS
        ref = O.apportion(post, now)
        A.apportion(now, writeback=True)
        gets, exp = A.leases()
        assert_leases_match(post, gets, exp, ref, label)
        assert_resources_match(post, A.resources(), ref, label)
        # a new client on the first row of the new tail
        row = np.array([old_n], np.int64)
        w = float(rng.uniform(1.0, 20.0))
        A.upsert(row, [0.0], [w], [1], [now + 300 * W.NS])
        got = A.read_store(old_n, 1)
        assert (got["has"][0], got["wants"][0], got["subclients"][0], got["expiry_ns"][0]) == (0.0, w, 1, now + 300 * W.NS)
        assert A.resources(0, 1, safe=False)["count"][0] == ref["res_count"][0] + 1
        assert not A.store_lost()
    assert sizes[0] == 6144
    assert bins_seen >= {"sub8x2", "sub16x2", "sub16x4", "sub32x4", "wave64x4", "block128x4", "block128x8",
                         "block256x8", "block2k4k", "large_resources"}


def test_server_grows_on_the_device():
    """A TickServer with one row per resource and clients arriving over a few rounds: every
    resource outgrows its rows at least three times, the leases equal the reference server
    model's (sequential Decide + Assign, as tests/test_server_gpu.py), and no store row
    crossed PCIe in the re-layouts."""
    from doorman_amd.server import TickServer
    from test_server_gpu import ServerModel, _check
    rng = np.random.default_rng(77)
    kinds = [W.FAIR_SHARE, W.PROPORTIONAL_SHARE, W.STATIC]
    resources = {f"r{k}": {"kind": kd, "capacity": float(100.0 * (k + 1)), "lease_length_s": 60,
                           "refresh_interval_s": 2} for k, kd in enumerate(kinds)}
    srv = TickServer(resources, slots=1)
    assert srv.stats() == {"relayouts": 0, "pcie_rows": 0}
    model = ServerModel(resources)
    now, arrived = NOW, 0
    for rnd, n_new in enumerate((1, 1, 2, 4, 8, 3)):  # 1, 2, 4, 8, 16, 19 clients: rows 1 -> 2 -> 4 -> 8 -> 16 -> 32
        now += 3 * W.NS
        arrived += n_new
        reqs, tickets = [], {}
        for r in resources:
            for i in rng.permutation(arrived):
                c = f"c{i}"
                cap = resources[r]["capacity"]
                has, wants = float(rng.uniform(0, cap / 8)), float(rng.uniform(0, cap / 4))
                reqs.append((c, r, has, wants, 1))
                tickets[(c, r)] = srv.get_capacity(c, r, has, wants)
        srv.tick(now)
        _check(srv, tickets, model.round(now, reqs, []), f"round={rnd}")
        for r in resources:
            st = srv.resource(r)
            assert st["clients"] == model.clients(r) == arrived
            assert st["count"] == model.stores[r].count()
    stats = srv.stats()
    assert stats["relayouts"] >= 3 and stats["pcie_rows"] == 0, stats
    srv.close()
