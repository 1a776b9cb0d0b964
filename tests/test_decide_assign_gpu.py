"""dm_decide_assign on the GPU: a round decided and assigned by one call, against the pair it
stands for -- dm_decide, then dm_store_upsert of each distinct requested row with the values of
that row's last request -- on a second engine loaded identically.

Both engines run the same decision kernels on the same store, so gets and expiry_ns are equal
bit for bit; both assign through the upsert's row step, so the stored rows, the counts, the
dense state and the flags are equal, and a resource's running sums are the same bits where one
row of it was assigned (one atomic add) and within the project's bar where several were (the
adds' order varies from run to run).  Bar (parity_util.float_close): floats within
1e-9 * max(|ref|, capacity), expiries and counts exact.

The store (8,283 rows): resources of 3, 40, 300, 600, 1,100 and 5,000 rows -- a sub-wave shape,
the workgroup bins 128 x 4, 128 x 8 and 256 x 8, the large chain -- of FairShare and
ProportionalShare, then Static, NoAlgorithm, a FairShare resource in learning mode and a
ProportionalShare one past its parent's expiry; a few released rows in each, a twentieth of the
leases lapsed.  Two states: the store as loaded, and after two writeback ticks, when the
workgroup-bin resources are dense and the Assign goes through the dense-state path (arrival
masks, state bytes; the round then comes 30 s later, after the 20-s leases have lapsed).  The
resource past its parent's expiry keeps 300-s leases: at capacity 0 with every row lapsed, the
branch ProportionalShare takes rests on the rounding residue Clean leaves in sum_wants (0 or a
last bit above it), for dm_decide and the oracle alike, and that is not this call's subject.

The safe capacity is compared with the rule dm_read_resources states (the configured value,
else capacity / count) on the count and configuration the pair engine reports: the call itself
gives its safe column only after a tick (DM_E_STATE otherwise), and the server derives the
value from the count in the same way.
"""
import ctypes

import numpy as np
import pytest

from doorman_amd import _lib
from doorman_amd import workloads as W
from oracle import oracle as O
from parity_util import assert_leases_match, float_close, row_capacity

pytestmark = pytest.mark.gpu
NOW = W.NOW_NS
S = W.NS
COLS = ("has", "wants", "subclients", "expiry_ns")

SIZES = np.array([3, 40, 300, 600, 1100, 5000, 300, 40, 300, 600], dtype=np.int64)
KINDS = np.array([W.FAIR_SHARE, W.PROPORTIONAL_SHARE, W.FAIR_SHARE, W.PROPORTIONAL_SHARE, W.FAIR_SHARE, W.FAIR_SHARE,
                  W.STATIC, W.NO_ALGORITHM, W.FAIR_SHARE, W.PROPORTIONAL_SHARE], dtype=np.int32)
CAPACITY = np.array([10.0, 100.0, 1000.0, 1000.0, 12345.678, 12345.678, 500.0, 50.0, 100.0, 1000.0])
LEASE_S = np.array([20, 300, 300, 300, 300, 300, 300, 20, 20, 300], dtype=np.int64)
SAFE = np.array([np.nan, 7.5, np.nan, 2.25, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan])
LEARNING, PARENT_EXPIRED, BIG = 8, 9, 5
STATES = ("loaded", "dense")
ROUNDS = ("new_wants", "new_clients", "thrice", "single", "fast70", "fast70_other_count", "lapsed")


def _snapshot():
    rng = np.random.default_rng(2024)
    N, R = int(SIZES.sum()), len(SIZES)
    n_row = np.repeat(SIZES, SIZES).astype(np.float64)
    cap_row = np.repeat(CAPACITY, SIZES)
    wants = rng.uniform(0.0, 3.0, N) * cap_row / n_row
    tie = rng.random(N) < 0.1
    wants[tie] = np.round(wants[tie])
    has = rng.uniform(0.0, 1.2, N) * cap_row / n_row
    sub = np.ones(N, np.int64)
    so = np.concatenate([[0], np.cumsum(SIZES)])
    sub[so[1]:so[2]] = rng.integers(1, 6, SIZES[1])  # the 40-row ProportionalShare resource: mixed counts
    exp = NOW + rng.integers(1, 300, N, dtype=np.int64) * S
    dead = rng.random(N) < 0.05
    exp[dead] = NOW - rng.integers(1, 300, int(dead.sum()), dtype=np.int64) * S
    for r in range(R):  # a few released rows in each
        k = max(1, int(SIZES[r]) // 40)
        free = so[r] + rng.choice(SIZES[r], k, replace=False)
        wants[free], has[free], sub[free], exp[free] = 0.0, 0.0, 0, W.RELEASED
    learning = np.full(R, W.INT64_MIN, np.int64)
    learning[LEARNING] = NOW + 3600 * S
    parent = np.full(R, W.INT64_MAX, np.int64)
    parent[PARENT_EXPIRED] = NOW - S
    return W.make_snapshot(SIZES, wants, has, sub, exp, KINDS, CAPACITY, LEASE_S, 5, learning, parent, SAFE)


SNAP = _snapshot()
SO = SNAP["seg_off"]


def _copy(snap):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in snap.items()}


def _host_writeback(host, ref):
    """The host copy takes a writeback tick's state (as the parity tests' host copies do)."""
    live = ref["expiry_ns"] != W.RELEASED
    host["has"] = np.where(live, ref["gets"], 0.0)
    host["wants"] = np.where(live, host["wants"], 0.0)
    host["subclients"] = np.where(live, host["subclients"], 0)
    host["expiry_ns"] = ref["expiry_ns"].copy()
    W.add_store_sums(host)


_HOSTS = {}


def _host_state(state):
    """The oracle's copy of the store in `state` and the round's time, computed once."""
    if state not in _HOSTS:
        host = _copy(SNAP)
        if state == "dense":
            for t in (NOW, NOW + S):
                _host_writeback(host, O.apportion(host, t))
        _HOSTS[state] = (host, NOW if state == "loaded" else NOW + 30 * S)
    host, now = _HOSTS[state]
    return _copy(host), now


@pytest.fixture(scope="module")
def engines():
    from doorman_amd.engine import Engine
    a, b = Engine(0), Engine(0)
    yield a, b
    a.close()
    b.close()


def _prepare(engines, state):
    for e in engines:
        e.load(SNAP)
        if state == "dense":
            e.apportion(NOW, writeback=True)
            e.apportion(NOW + S, writeback=True)
    if state == "dense":  # the Assign below goes through the dense-state path
        assert engines[0].store_stats()["dense_resources"] >= 4, engines[0].store_stats()


def _round(name, st, now):
    """(rows, has, wants, subclients) of round `name` on the store st (read from the device) at
    time `now`, in the caller's order."""
    rng = np.random.default_rng(ROUNDS.index(name) + 11)
    e = st["expiry_ns"]
    free = e == W.RELEASED
    lapsed = ~free & (now > e)
    live = ~free & ~lapsed

    def of(mask, r, k):
        rows = SO[r] + np.flatnonzero(mask[SO[r]:SO[r + 1]])
        return rng.choice(rows, min(k, len(rows)), replace=False)

    def asks(rows, sub=None):
        rows = np.asarray(rows, np.int64)
        r = np.searchsorted(SO, rows, side="right") - 1
        w = rng.uniform(0.0, 3.0, len(rows)) * CAPACITY[r] / SIZES[r]
        s = np.maximum(st["subclients"][rows], 1) if sub is None else np.full(len(rows), sub, np.int64)
        return rows, rng.uniform(0.0, 1.0, len(rows)) * CAPACITY[r] / SIZES[r], w, s

    def mixed(parts, shuffle=True):
        rows, has, wants, sub = (np.concatenate(c) for c in zip(*parts))
        order = rng.permutation(len(rows)) if shuffle else np.arange(len(rows))
        return rows[order], has[order], wants[order], sub[order].astype(np.int64)

    R = len(SIZES)
    if name == "new_wants":  # existing rows with new wants, every resource
        return mixed([asks(of(live, r, 2 if SIZES[r] < 100 else 6)) for r in range(R)])
    if name == "new_clients":  # new clients on free rows, beside two refreshing ones
        return mixed([asks(of(free, r, 3), sub=1) for r in range(R)] + [asks(of(live, 3, 2))])
    if name == "thrice":  # one row three times (the last wins), another twice, others between
        a, b = of(live, 2, 1)[0], of(live, 3, 1)[0]
        others = [x for x in np.concatenate([of(live, 2, 4), of(live, 3, 3), of(live, 6, 2)]) if x not in (a, b)]
        return mixed([asks([a]), asks(others[:3]), asks([b]), asks([a]), asks(others[3:]), asks([b]), asks([a])],
                     shuffle=False)
    if name == "single":  # resources with exactly one request: their sums are the pair's bits
        return mixed([asks(of(live, r, 1)) for r in (1, 3, 4, 6)])
    if name in ("fast70", "fast70_other_count"):  # 70 requests on the 5,000-row FairShare resource
        rows, has, wants, sub = asks(of(live, BIG, 70), sub=1)
        if name == "fast70_other_count":
            sub[33] = 2  # one request of another count: the fast path declines the resource
        return rows, has, wants, sub
    if name == "lapsed":  # rows whose lease has lapsed at `now` (Clean drops them first: new clients)
        parts = [asks(of(lapsed, r, 3)) for r in range(R)]
        assert sum(len(p[0]) for p in parts) >= 6
        return mixed(parts + [asks(of(live, 4, 2))])
    raise AssertionError(name)


def _last_per_row(rows):
    """The caller's indices of the last request on each distinct row, ascending."""
    last = {}
    for k, row in enumerate(rows):
        last[int(row)] = k
    return np.array(sorted(last.values()), np.int64)


def _pair(eng, now, rows, has, wants, sub):
    """The pair the call stands for, as dm_server_tick makes it."""
    gets, exp = eng.decide(now, rows, has, wants, sub)
    k = _last_per_row(rows)
    eng.upsert(rows[k], gets[k], wants[k], sub[k], exp[k])
    return gets, exp


def _safe_of(eng, rows):
    """dm_read_resources' rule on what the engine reports (the module docstring says why)."""
    cfg, res = eng.config(), eng.resources(safe=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        per_res = np.where(np.isnan(cfg["safe_capacity"]), cfg["capacity"] / res["count"].astype(np.float64),
                           cfg["safe_capacity"])
    return per_res[np.searchsorted(SO, rows, side="right") - 1]


def _assert_same_state(a, b, rows, label):
    sa, sb = a.read_store(), b.read_store()
    for k in COLS:
        assert sa[k].tobytes() == sb[k].tobytes(), (label, k, np.flatnonzero(sa[k] != sb[k])[:8])
    ra, rb = a.resources(safe=False), b.resources(safe=False)
    np.testing.assert_array_equal(rb["count"], ra["count"], err_msg=label)
    assigned = np.bincount(np.searchsorted(SO, np.unique(rows), side="right") - 1, minlength=len(SIZES))
    for k in ("sum_has", "sum_wants"):
        one = assigned <= 1  # no Assign or a single add: the same bits
        assert ra[k][one].tobytes() == rb[k][one].tobytes(), (label, k, ra[k][one], rb[k][one])
        ok = float_close(rb[k], ra[k], CAPACITY)
        assert ok.all(), (label, k, np.flatnonzero(~ok), rb[k][~ok], ra[k][~ok])
    assert a.store_stats() == b.store_stats(), (label, a.store_stats(), b.store_stats())
    return sa


def _oracle_round(host, rows, has, wants, sub, now):
    """The oracle's Resource.Decide replayed request by request, each ending with its Assign
    (resource.go:100-113), on stores made from the host copy; the host copy takes the stores'
    rows and sums afterwards.  Returns the decisions."""
    cfg = O.make_cfg(len(SIZES))
    for f in O.CFG_DTYPE.names:
        cfg[f] = host[f]
    stores = {}
    ref_g, ref_e = np.empty(len(rows)), np.empty(len(rows), np.int64)
    for k, row in enumerate(rows):
        r = int(np.searchsorted(SO, row, side="right")) - 1
        if r not in stores:
            st = O.Store(int(SIZES[r]))
            for j in range(SO[r], SO[r + 1]):
                if host["expiry_ns"][j] != W.RELEASED:
                    st.put(int(j - SO[r]), int(host["expiry_ns"][j]), host["has"][j], host["wants"][j],
                           int(host["subclients"][j]))
            st.set_sums(int(host["agg_count"][r]), host["agg_sum_has"][r], host["agg_sum_wants"][r])
            stores[r] = st
        lease = O.decide(stores[r], cfg[r], int(row - SO[r]), has[k], wants[k], int(sub[k]), now)
        ref_g[k], ref_e[k] = lease.has, lease.expiry_ns
    for r, st in stores.items():
        for j in range(SO[r], SO[r + 1]):
            c = int(j - SO[r])
            if st.has_client(c):
                l = st.get(c)
                host["has"][j], host["wants"][j], host["subclients"][j], host["expiry_ns"][j] = \
                    l.has, l.wants, l.subclients, l.expiry_ns
            else:
                host["has"][j], host["wants"][j], host["subclients"][j], host["expiry_ns"][j] = 0.0, 0.0, 0, W.RELEASED
    W.add_store_sums(host)
    return ref_g, ref_e


@pytest.mark.parametrize("name", ROUNDS)
@pytest.mark.parametrize("state", STATES)
def test_one_call_leaves_what_the_pair_leaves(engines, state, name):
    a, b = engines
    _prepare(engines, state)
    host, now = _host_state(state)
    rows, has, wants, sub = _round(name, a.read_store(), now)
    label = f"{state}/{name}"
    ga, ea = _pair(a, now, rows, has, wants, sub)
    gb, eb, safe = b.decide_assign(now, rows, has, wants, sub, safe=True)
    assert ga.tobytes() == gb.tobytes(), (label, np.flatnonzero(ga != gb)[:8])
    np.testing.assert_array_equal(eb, ea, err_msg=label)
    _assert_same_state(a, b, rows, label)
    want_safe = _safe_of(a, rows)
    assert safe.tobytes() == want_safe.tobytes(), (label, safe[:8], want_safe[:8])
    # the decisions, and two writeback ticks after them, against the oracle's sequential replay
    ref_g, ref_e = _oracle_round(host, rows, has, wants, sub, now)
    np.testing.assert_array_equal(eb, ref_e, err_msg=label)
    cap_row = row_capacity(SNAP)
    ok = float_close(gb, ref_g, cap_row[rows])
    assert ok.all(), (label, np.flatnonzero(~ok)[:8], gb[~ok][:4], ref_g[~ok][:4])
    for i, t in enumerate((now + S, now + 2 * S)):
        ref = O.apportion(host, t)
        leases = []
        for e in engines:
            e.apportion(t, writeback=True)
            leases.append(e.leases())
            assert_leases_match(host, *leases[-1], ref, f"{label}: tick {i}")
        np.testing.assert_array_equal(leases[1][1], leases[0][1], err_msg=label)
        ok = float_close(leases[1][0], leases[0][0], cap_row)
        assert ok.all(), (label, i, np.flatnonzero(~ok)[:8])
        _host_writeback(host, ref)
    assert not a.store_lost() and not b.store_lost()


def test_without_the_safe_column_the_store_and_the_leases_are_the_same(engines):
    a, b = engines
    _prepare(engines, "loaded")
    rows, has, wants, sub = _round("thrice", a.read_store(), NOW)
    ga, ea, _ = a.decide_assign(NOW, rows, has, wants, sub, safe=True)
    gb, eb = b.decide_assign(NOW, rows, has, wants, sub)  # safe_capacity NULL
    assert ga.tobytes() == gb.tobytes() and ea.tobytes() == eb.tobytes()
    _assert_same_state(a, b, rows, "safe NULL")
    for e in engines:
        e.apportion(NOW + S, writeback=True)
    (g0, e0), (g1, e1) = a.leases(), b.leases()
    np.testing.assert_array_equal(e1, e0)
    assert float_close(g1, g0, row_capacity(SNAP)).all()


def test_rejected_and_empty_rounds_leave_the_store_as_it_was(engines):
    a, _ = engines
    _prepare((a,), "loaded")
    before, res_before = a.read_store(), a.resources(safe=False)
    rows, has, wants, sub = _round("new_wants", before, NOW)
    L, ctx = _lib.lib(), a._ctx
    bad = rows.copy()
    bad[len(bad) // 2] = len(SNAP["wants"])  # one row past the store's end, behind valid requests
    gets, safe, exp = np.full(len(rows), -7.0), np.full(len(rows), -8.0), np.full(len(rows), -9, np.int64)
    p = [x.ctypes.data for x in (bad, has, wants, sub, gets, exp, safe)]
    assert L.dm_decide_assign(ctx, NOW, len(rows), *p) == _lib.DM_E_RANGE
    assert b"out of range" in L.dm_last_error(ctx)
    assert (gets == -7.0).all() and (exp == -9).all() and (safe == -8.0).all()
    badsub = sub.copy()
    badsub[0] = -1
    p[3] = badsub.ctypes.data
    p[0] = rows.ctypes.data
    assert L.dm_decide_assign(ctx, NOW, len(rows), *p) == _lib.DM_E_INVAL
    assert L.dm_decide_assign(ctx, NOW, 0, *[None] * 7) == _lib.DM_OK  # n == 0
    assert L.dm_decide_assign(ctx, NOW, 2, *[None] * 7) == _lib.DM_E_INVAL  # columns missing
    after, res_after = a.read_store(), a.resources(safe=False)
    for k in COLS:
        assert after[k].tobytes() == before[k].tobytes(), k
    for k in ("count", "sum_has", "sum_wants"):
        assert res_after[k].tobytes() == res_before[k].tobytes(), k
    # the engine still decides and assigns afterwards
    g, e = a.decide_assign(NOW, rows, has, wants, sub)
    k = _last_per_row(rows)
    st = a.read_store()
    assert st["has"][rows[k]].tobytes() == g[k].tobytes() and st["wants"][rows[k]].tobytes() == wants[k].tobytes()
    np.testing.assert_array_equal(st["expiry_ns"][rows[k]], e[k])
    np.testing.assert_array_equal(st["subclients"][rows[k]], sub[k])


def test_server_tick_gives_what_a_hand_made_pair_gives():
    """dm_server_tick against dm_decide + dm_store_upsert + dm_read_resources made by hand on a
    second context holding the server's store: the four values of every ticket's lease, and the
    stored rows, for a round with a new client and a client asking twice.  Whichever route the
    server takes for its round (the pair, or one dm_decide_assign: DESIGN 9.5 says which and
    why), this is what it must give."""
    from doorman_amd.engine import Engine
    from doorman_amd.server import TickServer
    slots = 4
    resources = {"fs": {"kind": W.FAIR_SHARE, "capacity": 100.0, "lease_length_s": 20, "refresh_interval_s": 3},
                 "ps": {"kind": W.PROPORTIONAL_SHARE, "capacity": 50.0, "lease_length_s": 30, "refresh_interval_s": 7,
                        "safe_capacity": 4.5}}
    ids = list(resources)
    srv = TickServer(resources, slots=slots)
    L = _lib.lib()
    ctx = ctypes.c_void_p(L.dm_server_ctx(srv._srv))
    R, N = len(ids), len(ids) * slots

    def store():
        st = {"has": np.empty(N), "wants": np.empty(N), "subclients": np.empty(N, np.int64),
              "expiry_ns": np.empty(N, np.int64)}
        assert L.dm_read_store(ctx, 0, N, *[st[k].ctypes.data for k in COLS]) == 0
        res = {"count": np.empty(R, np.int64), "sum_has": np.empty(R), "sum_wants": np.empty(R)}
        assert L.dm_read_resources(ctx, 0, R, res["count"].ctypes.data, res["sum_has"].ctypes.data,
                                   res["sum_wants"].ctypes.data, None) == 0
        return st, res

    # round 1: three clients arrive, with wants that tell their rows apart afterwards
    first = {("a", "fs"): 61.0, ("b", "fs"): 62.0, ("a", "ps"): 33.0}
    for (c, r), w in first.items():
        srv.get_capacity(c, r, 0.0, w)
    srv.tick(NOW)
    st, res = store()
    row_of = {cr: int(np.flatnonzero(st["wants"] == w)[0]) for cr, w in first.items()}
    snap = {"seg_off": np.arange(R + 1, dtype=np.int64) * slots, **st,
            "agg_count": res["count"], "agg_sum_has": res["sum_has"], "agg_sum_wants": res["sum_wants"]}
    for f in W.CFG_FIELDS:
        snap[f] = srv._keep[f]
    # round 2: a asks twice on fs, between them a new client c; a refreshes on ps
    now = NOW + 2 * S
    asks = [("a", "fs", 10.0, 70.0), ("c", "fs", 0.0, 55.0), ("a", "fs", 12.0, 40.0), ("a", "ps", 5.0, 20.0)]
    tickets = [srv.get_capacity(c, r, h, w) for c, r, h, w in asks]
    srv.tick(now)
    got = [srv.lease(t) for t in tickets]
    st2, _ = store()
    new_row = np.flatnonzero((st["expiry_ns"] == W.RELEASED) & (st2["expiry_ns"] != W.RELEASED))
    assert len(new_row) == 1 and ids.index("fs") * slots <= new_row[0] < (ids.index("fs") + 1) * slots
    row_of[("c", "fs")] = int(new_row[0])
    srv.close()
    rows = np.array([row_of[(c, r)] for c, r, _, _ in asks], np.int64)
    has, wants = np.array([q[2] for q in asks]), np.array([q[3] for q in asks])
    sub = np.ones(len(asks), np.int64)
    with Engine(0) as e:
        e.load(snap)
        gets, exp = _pair(e, now, rows, has, wants, sub)
        count = e.resources(safe=False)["count"]
        pair_store = e.read_store()
    for k in COLS:
        assert pair_store[k].tobytes() == st2[k].tobytes(), k
    for k, (c, r, _, _) in enumerate(asks):
        i = ids.index(r)
        cfg_safe = resources[r].get("safe_capacity", np.nan)
        safe = resources[r]["capacity"] / float(count[i]) if np.isnan(cfg_safe) else cfg_safe
        want = (gets[k], int(exp[k]) // S, resources[r]["refresh_interval_s"], safe)
        have = (got[k].capacity, got[k].expiry_time, got[k].refresh_interval, got[k].safe_capacity)
        assert have == want, (c, r, have, want)
