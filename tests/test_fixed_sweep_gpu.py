"""The sweep in front of the FIXED build of the dense tick kernel (dm_tick_steady.h
k_sweep / k_block_list): a FIXED launch with keys in use runs as
one lane per item, which finishes every item whose key holds (the write_resource call the
workgroup made) and lists the others with their keys cleared, then the FIXED build over the
list alone, its grid sized from the count the device last told the host.

Nothing a caller can read may depend on it: engine A (DM_SWEEP=0: k_block_dense's kFixed build over
every item, as before) and engine B (the default) hold identical bits after every tick, B
matches the oracle, and dm_plan_info's "sweep_parts" is 0 for A and positive for B exactly
when "fixed_parts" is.

The fixed resources are under capacity (sum of wants <= C / 2) with wants multiples of
2^-10, so that every sum is exact and gets == wants in any summation order: the oracle alone
confirms, before any engine runs, that each is a fixed point from its second tick on
(oracle_fixed, a condition of the data).  The resources that must stay on the worklist are
"moving" ones, FairShare over capacity with wants the oracle shows to change some row on
every tick (the rounding of the round-2 shares feeds back through has), and, where the
test needs a resource that holds no key whatever the arithmetic, resources in learning
mode (group_segment sets no key in learning mode)."""
import numpy as np
import pytest

from doorman_amd import workloads as W
import hier_model as M
import test_fixed_point_gpu as FP
from test_fixed_point_gpu import store  # noqa: F401  (the fixture of the every-instance test)
from test_skip_unchanged_gpu import copy_of, host_tick

pytestmark = pytest.mark.gpu

NOW = W.NOW_NS
ROWS = 257  # the first row count of the 128 x 4 bin
COLS = ("has", "wants", "subclients", "expiry_ns")
TICKS = 5


def sweep_engines(monkeypatch, n=1):
    """n engines with DM_SWEEP=0 and n with the default (read when the context is created)."""
    from doorman_amd.engine import Engine
    monkeypatch.delenv("DM_FIXED", raising=False)  # (a suite run with the FIXED build off: on here)
    monkeypatch.setenv("DM_SWEEP", "0")
    a = [Engine(0) for _ in range(n)]
    monkeypatch.delenv("DM_SWEEP")
    return a, [Engine(0) for _ in range(n)]


def sweep_counts(self, label):
    """B's (fixed_parts, fixed_items).  A never sweeps and B sweeps exactly where its keys are
    in use; both keep the same keys."""
    a, b = self.A.plan_info(), self.B.plan_info()
    assert a["sweep_parts"] == 0, label
    assert a["fixed_parts"] == b["fixed_parts"], label
    assert (b["sweep_parts"] > 0) == (b["fixed_parts"] > 0), (label, b["sweep_parts"], b["fixed_parts"])
    items = self.B.store_stats()["fixed_items"]
    assert self.A.store_stats()["fixed_items"] == items, label
    return b["fixed_parts"], items


class SweepPair(FP.Pair):
    """test_fixed_point_gpu.Pair with A = DM_SWEEP=0 and B = the default."""

    def __init__(self, monkeypatch, snap):
        monkeypatch.setattr(FP, "engines", sweep_engines)
        super().__init__(monkeypatch, snap)

    counts = sweep_counts


def under_wants(rng, n, C=1000.0):
    """sum <= C / 2, multiples of 2^-10"""
    return np.floor(rng.uniform(0.0, 1.0, n) * (0.5 * C / n) * 1024.0) / 1024.0


def changes_every_tick(wants, C, ticks=TICKS + 3):
    """Oracle only: a FairShare resource of these wants (has 0 at first) changes some row's
    has on every writeback tick from the second on."""
    n = len(wants)
    host = W.make_snapshot([n], wants, np.zeros(n), np.ones(n, np.int64), np.full(n, NOW + 100 * W.NS),
                           W.FAIR_SHARE, C, lease_length_s=20, refresh_interval_s=5)
    host_tick(host, NOW)
    for t in range(1, ticks):
        before = host["has"].copy()
        host_tick(host, NOW + 2 * t * W.NS)
        if np.array_equal(before.view(np.int64), host["has"].view(np.int64)):
            return False
    return True


@pytest.fixture(scope="module")
def moving():
    """(wants, capacity) of a 257-row FairShare resource that is never a fixed point: a
    condition of the data, found and confirmed by the oracle alone."""
    rng = np.random.default_rng(77)
    for _ in range(64):
        C = 100.0
        w = rng.uniform(0.5, 1.5, ROWS) * (3.0 * C / ROWS)
        if changes_every_tick(w, C):
            return w, C
    raise AssertionError("no candidate changes on every tick")


def bin_store(K, moving_at, moving, seed=5):
    """K resources of 257 rows, FairShare: the ones at `moving_at` move, the others are under
    capacity."""
    rng = np.random.default_rng(seed)
    mw, mC = moving if moving_at else (None, None)
    wants, caps = [], []
    for r in range(K):
        if r in moving_at:
            wants.append(mw)
            caps.append(mC)
        else:
            wants.append(under_wants(rng, ROWS))
            caps.append(1000.0)
    wants = np.concatenate(wants)
    N = len(wants)
    return W.make_snapshot(np.full(K, ROWS), wants, np.zeros(N), np.ones(N, np.int64),
                           NOW + rng.integers(30, 300, N, dtype=np.int64) * W.NS, W.FAIR_SHARE,
                           np.asarray(caps), lease_length_s=20, refresh_interval_s=5)


def oracle_fixed(snap, ticks=TICKS):
    """Oracle only: per tick from the second on, which resources the tick leaves unchanged."""
    host = copy_of(snap)
    host_tick(host, NOW)
    return [FP.unchanged_by_tick(host, NOW + 2 * t * W.NS) for t in range(1, ticks)]


def edge_positions(K):
    return {p for p in (0, 63, K - 1) if p < K}


CASES = [(K, "edges") for K in (1, 63, 64, 65, 1023, 1024, 1025)] + [(1025, "all fixed"), (65, "none fixed")]


@pytest.mark.parametrize("K,what", CASES, ids=[f"{k}-{w.replace(' ', '-')}" for k, w in CASES])
def test_wave_and_workgroup_edges_of_the_sweep(monkeypatch, moving, K, what):
    """The 257-row bin with 1 ... 1,025 resources (a partial wave, a full wave, one lane of the
    next; a partial workgroup, a full one, one lane of the next), most of them fixed and the
    moving ones at the bin's first, 64th and last positions; every resource fixed (an empty
    worklist); none fixed (the list holds every item).  Five ticks: identical bits after
    each, the oracle on the last, and the keys in use on the last: valid for every fixed
    resource and for no learning one."""
    at = {"edges": edge_positions(K), "all fixed": set(), "none fixed": set(range(K))}[what]
    snap = bin_store(K, at, moving)
    learn = set()
    if what == "none fixed":  # every other one in learning mode: no key, whatever the arithmetic
        learn = set(range(1, K, 2))
        snap["learning_end_ns"] = np.where(np.arange(K) % 2 == 1, NOW + 3600 * W.NS, W.INT64_MIN).astype(np.int64)
    still = np.array([r not in at for r in range(K)])
    for t, same in enumerate(oracle_fixed(snap)):  # the data's condition
        assert same[still].all() and not same[~still & ~np.isin(np.arange(K), list(learn))].any(), f"tick {t + 2}"
    P = SweepPair(monkeypatch, snap)
    try:
        for t in range(TICKS):
            parts, items = P.tick(f"tick {t + 1}", 2 * t, oracle=t == TICKS - 1)
            assert (parts > 0) == (t >= 2), (t, parts)
        # a key for every fixed resource, none for a learning one (the moving ones: the oracle says none)
        assert K - len(at) <= items <= K - len(learn), (items, K, len(at), len(learn))
    finally:
        P.close()


@pytest.mark.parametrize("how", ["parent expiry", "learning"])
def test_a_list_longer_than_the_launched_grid(monkeypatch, how):
    """1,100 fixed resources, 600 of which share a parent expiry that passes between two ticks
    with no call: the tick after finds 600 refuted keys while its grid is sized from a told
    count of 0 (the floor of 16 workgroups strides over the list).  Identical bits and the
    oracle on that tick and the next two; the 600 keys were cleared in memory.  Then the
    same with learning mode ending at that time (those 600 hold no key before: learning)."""
    K, hit = 1100, np.arange(250, 850)
    snap = bin_store(K, set(), None, seed=9)
    for same in oracle_fixed(snap, 4):  # the data's condition (before the time, with neither mode set)
        assert same.all()
    when = NOW + 7 * W.NS
    if how == "parent expiry":
        snap["parent_expiry_ns"] = np.where(np.isin(np.arange(K), hit), when, W.INT64_MAX).astype(np.int64)
    else:
        snap["learning_end_ns"] = np.where(np.isin(np.arange(K), hit), when, W.INT64_MIN).astype(np.int64)
    P = SweepPair(monkeypatch, snap)
    try:
        for t in range(4):
            parts, before = P.tick(f"tick {t + 1}", 2 * t)
        assert parts > 0 and before == (K if how == "parent expiry" else K - len(hit)), (parts, before)
        parts, after = P.tick("the tick after the time", 8, oracle=True)
        assert parts > 0
        if how == "parent expiry":
            assert before - after >= len(hit), (before, after)
        P.tick("one tick later", 10, oracle=True)
        parts, items = P.tick("two ticks later", 12, oracle=True)
        assert parts > 0 and items >= K - len(hit), (parts, items)
    finally:
        P.close()


def test_every_dense_instance_through_the_fixed_point_events(monkeypatch, store):  # noqa: F811
    """test_fixed_point_gpu's store (first and last row count of every dense instance, bins
    3-6) and its two event sequences (a wants refresh, a release and an arrival, load_config,
    NaN wants and its repair; learning mode ending, a parent expiry passing, a non-writeback,
    a recompute and an alternate-column tick, the 25-s lapse), with A = DM_SWEEP=0 and B =
    the default in place of its engines."""
    monkeypatch.setattr(FP, "engines", sweep_engines)
    monkeypatch.setattr(FP.Pair, "counts", sweep_counts)
    FP.test_keys_engage_and_row_writes_end_them(monkeypatch, store)
    FP.test_ticks_and_times_that_end_a_fixed_point_without_a_call(monkeypatch, store)


@pytest.mark.parametrize("big", [False, True], ids=["capacity there and back", "count beyond the root's range"])
def test_under_the_pipelined_exchange(monkeypatch, big):
    """A leaf of 140 resources of 257-512 rows (one bin: a sweep wave holds pub_first among
    other resources), 30 of 513-1099 and 6 larger ones under the pipelined exchange, as
    test_fixed_point_gpu.test_capacity_there_and_back_under_the_exchange: the capacity of a
    resource at its fixed point halved at the root and restored.  big: one resource's running
    count is beyond the root's 32-bit column (its rows are as the others'), so that every
    tick raises DM_HIER_COUNT_RANGE for it, from a sweep lane once its key holds; the root
    then rejects every round and the leaf keeps the templates it was loaded with, so no
    capacity is halved.  Leases, templates, leaf and root stores and the root's verdict are
    the same bits as with DM_SWEEP=0 at every step; the leaf sweeps wherever its keys are in
    use."""
    import torch
    from doorman_amd import _lib
    from doorman_amd.hierarchy import HierarchicalTick, root_snapshot
    torch.cuda.set_device(0)
    rng = np.random.default_rng(21)
    sizes = np.concatenate([rng.integers(257, 513, 140), rng.integers(513, 1100, 30), rng.integers(1025, 4097, 6)])
    R = len(sizes)
    rcfg = {"kind": rng.choice([W.FAIR_SHARE, W.PROPORTIONAL_SHARE, W.STATIC, W.NO_ALGORITHM], R).astype(np.int32),
            "capacity": rng.choice([100.0, 1000.0, 2500.5], R),
            "lease_length_s": rng.choice([20, 60], R).astype(np.int64),
            "refresh_interval_s": rng.choice([1, 5], R).astype(np.int64),
            "learning_end_ns": np.full(R, W.INT64_MIN, np.int64),
            "parent_expiry_ns": np.full(R, W.INT64_MAX, np.int64),
            "safe_capacity": np.where(rng.random(R) < 0.5, np.nan, rng.uniform(1, 9, R))}
    full = W.make_snapshot(sizes, rng.uniform(0.2, 3.0, int(sizes.sum())) * 1000.0 / np.repeat(sizes, sizes),
                           0.0, 1, NOW + 60 * W.NS, W.FAIR_SHARE, 1000.0)
    BIG = 40
    if big:
        full["agg_count"] = np.array(full["agg_count"])
        full["agg_count"][BIG] = 2 ** 31 + 5
    off = np.concatenate([[0], np.cumsum(sizes)])
    shared = rcfg["kind"] >= W.PROPORTIONAL_SHARE  # the kinds whose gets depend on the capacity
    HALVE, RESTORE, STEPS = 9, 11, 18
    (la, ra), (lb, rb) = sweep_engines(monkeypatch, 2)
    try:
        runs = []
        for leaf, root in ((la, ra), (lb, rb)):
            leaf.load(M.with_config(full, M.default_config(R)))
            root.load(M.with_config(root_snapshot(R, 1, W.FAIR_SHARE, 1.0), rcfg))
            ht = HierarchicalTick(torch, leaf, root, R, 1, 0, None, shard_lo=np.array([0, R]), pipelined=True,
                                  native="local")
            out, info, items, target = [], [], [], None
            for t in range(STEPS):
                now = NOW + 2 * t * W.NS
                if t == HALVE and not big:
                    g1, g2 = out[-1][0][0], out[-2][0][0]
                    target = next(r for r in range(R) if shared[r] and r != BIG and g1[off[r]:off[r + 1]].any() and
                                  g1[off[r]:off[r + 1]].tobytes() == g2[off[r]:off[r + 1]].tobytes())
                    halved = {k: np.array(v) for k, v in rcfg.items()}
                    halved["capacity"][target] *= 0.5
                    root.load_config(halved)
                if t == RESTORE and not big:
                    root.load_config(rcfg)
                ht.tick(now)
                pi = leaf.plan_info()
                info.append((pi["fixed_parts"], pi["sweep_parts"]))
                items.append(leaf.store_stats()["fixed_items"])
                out.append((leaf.leases(), leaf.config(), leaf.read_store(), root.read_store(), ht.status()))
            runs.append((out, info, items, target))
        (oa, pa, ia, ta), (ob, pb, ib, tb) = runs
        assert not any(s for _, s in pa), pa
        assert [f for f, _ in pa] == [f for f, _ in pb], (pa, pb)
        assert all((s > 0) == (f > 0) for f, s in pb), pb
        assert pb[HALVE - 1][1] > 0 and ib[HALVE - 1] > 0 and pb[-1][1] > 0 and ib[-1] > 0, (pb, ib)
        assert ia == ib, (ia, ib)
        assert ta == tb
        if big:  # reported on the last steps too, when the resource's key holds: from a sweep lane
            assert all((np.asarray(o[4]).astype(np.int64) & _lib.DM_HIER_COUNT_RANGE).any() for o in ob[-3:]), \
                [o[4] for o in ob[-3:]]
        else:  # the halving moved the target's leases off their fixed point
            gets = [o[0][0][off[tb]:off[tb + 1]] for o in ob]
            assert any(not np.array_equal(gets[t], gets[HALVE - 1]) for t in range(HALVE, RESTORE + 3)), tb
        for t, (a, b) in enumerate(zip(oa, ob)):
            for x, y in zip(a[0], b[0]):
                assert x.tobytes() == y.tobytes(), f"step {t}: leases"
            for k in W.CFG_FIELDS:
                assert a[1][k].tobytes() == b[1][k].tobytes(), f"step {t}: template {k}"
            for k in COLS:
                assert a[2][k].tobytes() == b[2][k].tobytes(), f"step {t}: leaf {k}"
                assert a[3][k].tobytes() == b[3][k].tobytes(), f"step {t}: root {k}"
            assert a[4].tobytes() == b[4].tobytes(), f"step {t}: the root's verdict on the request"
    finally:
        for e in (la, ra, lb, rb):
            e.close()
