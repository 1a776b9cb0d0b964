"""The fused form of a steady dense tick (dm_tick_fused.hip k_block_fused, dm_split_form.h
PartForm::fused): the sweep (or the cycle form's), the row kernel over
its worklist and the rest kernel as one launch, chosen while the device tells of few listed
items.

Nothing a caller can read may depend on it: engine A (DM_FUSED=0: the launches as they were)
and engine B (the default) hold identical bits after every tick (leases, rows, records,
configuration) and the same number of valid keys, and B matches the oracle on the ticks the
cycle form's tests check (1, 2, 3 and 8).  dm_plan_info's "fused_parts" says whether a part's
last tick ran fused.

The stores are FairShare resources under capacity with wants that are multiples of 2^-10 (each
a fixed point from its second tick on, test_fixed_sweep_gpu.under_wants), with a few
oversubscribed ones among them (listed on some or every tick, whatever the device's summation
order makes of them: no case relies on which).  A workgroup of k_block_fused sweeps G items
(kFusedChunk: its thread count), so the item counts are 1, G - 1, G, G + 1 for every dense
instance, and 2 G + 3 for 128 x 4.
"""
import ctypes

import numpy as np
import pytest

from doorman_amd import _lib
from doorman_amd import workloads as W
from oracle import oracle as O
from parity_util import assert_leases_match
import test_fixed_point_gpu as FP
from test_fixed_sweep_gpu import under_wants
from test_skip_unchanged_gpu import copy_of, host_tick
from test_steady_dense_gpu import assert_same_state

pytestmark = pytest.mark.gpu

NOW = W.NOW_NS
# rows per resource -> the threads of its dense instance (a store of one size: bin 6 runs 512 x 8)
SHAPES = {257: 128, 1000: 128, 1025: 256, 4096: 512}


def fused_engines(monkeypatch, n=1, b_mode=None):
    """n engines with DM_FUSED=0 and n with the default, or DM_FUSED=b_mode (read when the
    context is created)."""
    from doorman_amd.engine import Engine
    for k in ("DM_FIXED", "DM_SWEEP", "DM_STEADY", "DM_CYCLE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DM_FUSED", "0")
    a = [Engine(0) for _ in range(n)]
    monkeypatch.delenv("DM_FUSED")
    if b_mode is not None:
        monkeypatch.setenv("DM_FUSED", str(b_mode))
    try:
        return a, [Engine(0) for _ in range(n)]
    finally:
        monkeypatch.delenv("DM_FUSED", raising=False)


class FusedPair(FP.Pair):
    """test_fixed_point_gpu.Pair with A = DM_FUSED=0 and B = the default; every writeback tick
    on `column` ("inplace": k_block_fused<.., false>; "alternate": <.., true>)."""

    def __init__(self, monkeypatch, snap, column):
        monkeypatch.setattr(FP, "engines", fused_engines)
        super().__init__(monkeypatch, snap)
        self.column = column
        self.t = -2
        self.track = True  # the oracle's host copy follows the ticks

    def counts(self, label):
        """B's fused_parts; A never runs fused, and both hold as many valid keys."""
        assert self.A.plan_info()["fused_parts"] == 0, label
        sa, sb = self.A.store_stats(), self.B.store_stats()
        assert (sa["fixed_items"], sa["cycling_items"]) == (sb["fixed_items"], sb["cycling_items"]), label
        return self.B.plan_info()["fused_parts"]

    def tick(self, label, dt=None, oracle=False, **kw):
        kw.setdefault("writeback", True)
        kw.setdefault("wb_columns", self.column if kw["writeback"] else "auto")
        if dt is None:
            self.t += 2
            dt = self.t
        else:
            self.t = dt
        now = NOW + dt * W.NS
        self.both(lambda e: e.apportion(now, **kw))
        assert_same_state(self.A, self.B, label)
        if oracle:
            assert self.track
            assert_leases_match(self.host, *self.B.leases(), O.apportion(self.host, now), label)
        if kw["writeback"] and self.track:
            host_tick(self.host, now)
        return self.counts(label)

    def settle(self, label="", ticks=8):
        """Eight ticks, the oracle on 1, 2, 3 and 8; B is fused by the last."""
        for t in range(1, ticks + 1):
            out = self.tick(f"{label}tick {t}", oracle=self.track and t in (1, 2, 3, 8))
        assert out > 0, (label, "fused_parts", out)
        self.track = False
        return out

    def more(self, label, n=4, fused=True):
        seen = [self.tick(f"{label}: tick {i + 1} after") for i in range(n)]
        assert not fused or seen[-1] > 0, (label, seen)
        return seen


def store(sizes, over=(), seed=5, parent_expiry=None):
    """FairShare resources of these row counts under capacity (fixed points), those at `over`
    oversubscribed (uniform wants around the fair share of a third of their demand)."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    wants = [rng.uniform(0.5, 1.5, n) * (3.0 * 1000.0 / n) if r in over else under_wants(rng, int(n))
             for r, n in enumerate(sizes)]
    N = int(sizes.sum())
    snap = W.make_snapshot(sizes, np.concatenate(wants), np.zeros(N), np.ones(N, np.int64),
                           NOW + rng.integers(30, 300, N, dtype=np.int64) * W.NS, W.FAIR_SHARE, 1000.0,
                           lease_length_s=20, refresh_interval_s=5)
    if parent_expiry is not None:
        snap["parent_expiry_ns"] = np.asarray(parent_expiry, np.int64)
    return snap


def halve_capacity(P, which):
    P.host["capacity"] = np.array(P.host["capacity"])
    P.host["capacity"][which] *= 0.5
    P.both(lambda e: e.load_config(P.host))


CASES = [(n, k) for n, g in SHAPES.items() for k in (1, g - 1, g, g + 1)] + [(257, 2 * 128 + 3)]


@pytest.mark.parametrize("column", ["inplace", "alternate"])
@pytest.mark.parametrize("n,K", CASES)
def test_every_dense_instance_runs_fused(monkeypatch, n, K, column):
    """K resources of n rows, the first and the last oversubscribed (K > 2).  Eight ticks settle
    B into the form; then a capacity is halved (a new row epoch: the two-kernel forms rewrite
    the keys) and four more ticks bring it back.  After the settle ticks a parent expiry passes
    by time alone in the last but one resource: a fused tick finds its key refuted and decides
    its rows itself.  (The capacity goes through dm_config_load, which starts a row epoch: the
    host knows, and that tick is no misprediction; the parent expiry is one.)"""
    over = {0, K - 1} if K > 2 else set()
    pexp = np.full(K, W.INT64_MAX, np.int64)
    pexp[max(K - 2, 0)] = NOW + 19 * W.NS  # between the ticks at 18 s and 20 s
    P = FusedPair(monkeypatch, store([n] * K, over, parent_expiry=pexp), column)
    try:
        shapes = P.B.plan_info()["bin_shapes"]
        assert (n != 4096 or shapes & 1) and not shapes & 2, shapes  # SHAPES' thread counts
        P.settle()  # ticks at 0 .. 14 s
        assert P.tick("tick 9", 16) > 0 and P.tick("tick 10", 18) > 0
        assert P.tick("the tick after the parent expiry", 20) > 0  # one listed item: still fused
        P.more("parent expiry")
        halve_capacity(P, [K // 2])
        P.more("capacity halved", 6)
    finally:
        P.close()


@pytest.mark.parametrize("column", ["inplace", "alternate"])
@pytest.mark.parametrize("K", [1, 255, 256, 257])
def test_bin_6_on_256_x_16_runs_fused(monkeypatch, K, column):
    """The same for 256 x 16: K resources of 4,096 rows beside enough 1,000-row resources that
    bin 6 holds the smaller half of the rows and keeps its narrow shape.  (64 x 16 is bin 4's
    shape in stream parts only, which run no steady form: no tick can reach that build.)"""
    fill = 5 * K + 5  # (more rows than bin 6's)
    over = {0, K - 1} if K > 2 else set()
    pexp = np.full(K + fill, W.INT64_MAX, np.int64)
    pexp[max(K - 2, 0)] = NOW + 19 * W.NS
    P = FusedPair(monkeypatch, store([4096] * K + [1000] * fill, over, parent_expiry=pexp), column)
    try:
        assert P.B.plan_info()["bin_shapes"] == 0
        assert P.settle() == 2  # ticks at 0 .. 14 s
        assert P.tick("tick 9", 16) == 2 and P.tick("tick 10", 18) == 2
        assert P.tick("the tick after the parent expiry", 20) == 2
        P.more("parent expiry")
    finally:
        P.close()


def test_the_empty_steady_state(monkeypatch):
    """Twenty fused ticks with nothing listed: the told counts (dm_plan_info's told_listed and
    told_queued) stay 0, B stays fused, results equal."""
    P = FusedPair(monkeypatch, store([257] * 300 + [1025] * 40), "inplace")
    try:
        P.settle()
        for i in range(20):
            assert P.tick(f"steady {i}") == 2  # both bins' parts, every tick
            info = P.B.plan_info()
            assert info["told_listed"] == 0 and info["told_queued"] == 0, (i, info)
    finally:
        P.close()


def mixed_sizes():
    """All six dense instances but 64 x 16 and 512 x 8: bin 6's rows are the smaller half, so
    it runs 256 x 16."""
    return [257] * 140 + [1000] * 20 + [1025] * 20 + [4096] * 3


@pytest.mark.parametrize("column", ["inplace", "alternate"])
def test_mispredicted_ticks(monkeypatch, column):
    """With B fused: every capacity halved by a call (dm_config_load starts a row epoch, so the
    host knows and the next tick is the key-rewriting two-kernel form: no misprediction, kept as
    the issue names it); then, by time alone (no call, the same row
    epoch: the host cannot know), the parent expiry of 60 resources passes, so that a fused tick
    finds 60 keys refuted, decides those rows itself and tells the count, after which B leaves
    the form and comes back; at last every follower lapses: a fused tick whose every item is a
    rest item.  Each of those ticks and the four after it equal A's."""
    sizes = mixed_sizes()
    K = len(sizes)
    pexp = np.full(K, W.INT64_MAX, np.int64)
    pexp[40:100] = NOW + 41 * W.NS
    P = FusedPair(monkeypatch, store(sizes, {0, 150, 170, K - 1}, parent_expiry=pexp), column)
    try:
        assert P.B.plan_info()["bin_shapes"] == 0
        assert P.settle() == 4  # every bin's part; ticks at 0 .. 14 s
        halve_capacity(P, slice(None))
        seen = P.more("every capacity halved", 8)  # 16 .. 30 s
        assert seen[0] == 0 and seen[-1] == 4, seen
        for dt in (32, 34, 36, 38, 40):
            assert P.tick(f"tick at {dt} s", dt) == 4
        assert P.tick("the tick after the parent expiries", 42) == 4  # mispredicted: fused, 60 items listed
        assert P.tick("the tick that tells them", 44) == 4
        assert P.B.plan_info()["told_listed"] >= 60  # (the next launch told the last one's count)
        seen = P.more("parent expiries", 8)
        assert min(seen[:3]) == 3 and seen[-1] == 4, seen  # the 128 x 4 part left the form once told, and is back
        assert P.tick("lapse", P.t + 400) == 4  # mispredicted: every item a rest item
        gets, exp = P.B.leases()
        assert not gets.any() and (exp == W.RELEASED).all()
        assert P.B.plan_info()["told_queued"] == K  # the rest count reaches the host within the tick ...
        assert P.tick("after the lapse") == 0  # ... so its next choice is A's: the mixed kernel
        a, b = P.A.plan_info(), P.B.plan_info()
        assert a["steady_parts"] == b["steady_parts"] == 0 and a["told_queued"] == b["told_queued"] == K, (a, b)
        P.more("lapse", fused=False)
    finally:
        P.close()


def test_rest_items_inside_a_fused_tick(monkeypatch):
    """Under dm_keep_keys mode 3 a release and an upsert keep the row epoch and the keys: one
    row released in three resources and a row upserted into one of them (a stale hint, a mask
    bit, an arrival bit) make rest items the host has no count of.  The tick stays fused, equals
    A, as do the four after it, and its rest count reaches the host (dm_plan_info told_queued)."""
    P = FusedPair(monkeypatch, store([257] * 300), "inplace")
    try:
        P.both(lambda e: e.keep_keys(3))
        P.settle()
        rows = np.array([P.row(r, 70) for r in (3, 130, 299)], np.int64)
        P.both(lambda e: e.release(rows))
        assert P.tick("release") > 0
        assert P.B.plan_info()["told_queued"] == 3  # the fused tick's ring, read in place of `queued`
        one = rows[:1]
        ne = NOW + (P.t + 200) * W.NS
        P.both(lambda e: e.upsert(one, np.zeros(1), np.full(1, 0.125), np.ones(1, np.int64), np.full(1, ne)))
        assert P.tick("upsert") > 0
        info = P.B.plan_info()
        assert info["told_queued"] == 3 and info["told_listed"] == 3, info  # (listed: the release tick's, a tick late)
        assert P.more("release and upsert")[-1] > 0
        # (the upsert refilled the row freed in the first resource, and its tick made the arrival
        # a follower: two resources still hold a released row; both slots of the ring have served)
        assert P.B.plan_info()["told_queued"] == 2
    finally:
        P.close()


@pytest.mark.parametrize("column", ["inplace", "alternate"])
def test_switching_forms_keeps_the_rings_sound(monkeypatch, column):
    """fused -> two-kernel -> fused over 12 ticks with an oversubscribed item in every phase: a
    non-writeback tick ends the keys, the two-kernel forms rewrite them and tell their counts,
    and the fused form resumes with its own ring."""
    P = FusedPair(monkeypatch, store([257] * 300, {7, 200}), column)
    try:
        P.settle()
        seen = [P.tick(f"fused {i}") for i in range(3)]
        seen.append(P.tick("no writeback", writeback=False))
        seen += [P.tick(f"after {i}") for i in range(8)]
        assert seen[:3] == [1, 1, 1] and seen[3] == 0 and seen[4] == 0 and seen[-1] == 1, seen
        assert P.more("second round", 3)[-1] == 1
        P.tick("in place" if column == "alternate" else "alternate",
               wb_columns="inplace" if column == "alternate" else "alternate")
        P.more("the other column for a tick", 8)
    finally:
        P.close()


def test_through_the_pipelined_exchange(monkeypatch):
    """test_cycle_gpu's leaf under the pipelined exchange (its templates are rewritten on the
    device every step; B engages the alternate column by itself as bench.py's default line
    does), with A = DM_FUSED=0 and B = DM_FUSED=2 (fused wherever the rule allows, whatever
    count was told: the store's many oversubscribed resources are then decided inside fused
    ticks).  The root halves a capacity and restores it two steps later.  After every step, bit
    for bit: leases, templates, leaf and root stores, the published blocks, the root's verdict."""
    import torch
    import hier_model as M
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
    shared = rcfg["kind"] >= W.PROPORTIONAL_SHARE
    off = np.concatenate([[0], np.cumsum(sizes)])
    HALVE, RESTORE, STEPS = 30, 32, 37
    monkeypatch.setenv("DM_CYCLE_BYTES", "0")
    try:
        (la, ra), (lb, rb) = fused_engines(monkeypatch, 2, b_mode=2)
    finally:
        monkeypatch.delenv("DM_CYCLE_BYTES")
    try:
        runs = []
        for leaf, root in ((la, ra), (lb, rb)):
            leaf.load(M.with_config(full, M.default_config(R)))
            root.load(M.with_config(root_snapshot(R, 1, W.FAIR_SHARE, 1.0), rcfg))
            ht = HierarchicalTick(torch, leaf, root, R, 1, 0, None, shard_lo=np.array([0, R]), pipelined=True,
                                  native="local")
            out, info, target = [], [], None
            for t in range(STEPS):
                now = NOW + t * W.NS // 2
                if t == HALVE:
                    g1 = out[-1][0][0]
                    target = next(r for r in range(R) if shared[r] and g1[off[r]:off[r + 1]].any())
                    halved = {k: np.array(v) for k, v in rcfg.items()}
                    halved["capacity"][target] *= 0.5
                    root.load_config(halved)
                if t == RESTORE:
                    root.load_config(rcfg)
                ht.tick(now)
                leases, cfg = leaf.leases(), leaf.config()
                pub = torch.stack(ht.totals).cpu().numpy().tobytes()
                info.append(leaf.plan_info()["fused_parts"])
                out.append((leases, cfg, leaf.read_store(), root.read_store(), ht.status(), pub))
            runs.append((out, info, target))
        (oa, ia, ta), (ob, ib, tb) = runs
        print(ib)
        assert not any(ia) and ta == tb, ia
        assert ib[HALVE - 1] > 0 and ib[HALVE] > 0 and ib[-1] > 0, ib  # fused when the halved template arrives
        gets = [o[0][0][off[tb]:off[tb + 1]] for o in ob]
        assert any(not np.array_equal(gets[t], gets[t - 2]) for t in range(HALVE, RESTORE + 3)), tb
        for t, (a, b) in enumerate(zip(oa, ob)):
            for x, y in zip(a[0], b[0]):
                assert x.tobytes() == y.tobytes(), f"step {t}: leases"
            for k in W.CFG_FIELDS:
                assert a[1][k].tobytes() == b[1][k].tobytes(), f"step {t}: template {k}"
            for k in ("has", "wants", "subclients", "expiry_ns"):
                assert a[2][k].tobytes() == b[2][k].tobytes(), f"step {t}: leaf {k}"
                assert a[3][k].tobytes() == b[3][k].tobytes(), f"step {t}: root {k}"
            assert a[4].tobytes() == b[4].tobytes(), f"step {t}: the root's verdict on the request"
            assert a[5] == b[5], f"step {t}: the published blocks"
    finally:
        for e in (la, ra, lb, rb):
            e.close()


def test_a_consumer_stream_sees_the_fused_ticks_writes(monkeypatch):
    """The fused launch is its part's last kernel and completes the part's tick event: a torch
    stream that snapshots the published block right after dm_stream_wait sees this tick's
    block.  Under dm_keep_keys mode 1 one wants refresh per tick keeps the row epoch, so the
    ticks stay fused while one resource's published sum changes every tick (after
    test_hierarchy_gpu's test_stream_wait_orders_a_foreign_stream_after_the_tick)."""
    import torch
    from doorman_amd.engine import Engine
    for k in ("DM_FUSED", "DM_FIXED", "DM_SWEEP", "DM_STEADY", "DM_CYCLE"):
        monkeypatch.delenv(k, raising=False)
    torch.cuda.set_device(0)
    L = _lib.lib()
    K = 2000
    snap = store([257] * K)
    off = np.asarray(snap["seg_off"])
    ring = [torch.zeros((K + 1, 2), dtype=torch.float64, device="cuda") for _ in range(3)]
    xs = torch.cuda.Stream()
    torch.cuda.synchronize()
    with Engine(0) as e:
        e.load(snap)
        e.keep_keys(1)
        ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ring])
        _lib.check(L.dm_publish_ring(e._ctx, 3, ptrs), e._ctx)
        for k in range(8):
            e.apportion(NOW + 2 * k * W.NS, writeback=True, wb_columns="inplace")
        assert e.plan_info()["fused_parts"] == 1
        r, row = 1234, int(off[1234]) + 70
        shots, want, fused = [], [], []
        for k in range(8, 16):
            v = (k - 7) / 1024.0
            e.update_wants(np.array([row], np.int64), np.array([v]))
            e.apportion(NOW + 2 * k * W.NS, writeback=True, wb_columns="inplace", asynchronous=True)
            e.stream_wait(xs.cuda_stream)
            with torch.cuda.stream(xs):
                shots.append(ring[k % 3].clone())
            fused.append(e.plan_info()["fused_parts"])
            want.append(v)
        e.sync()
        torch.cuda.synchronize()
    assert all(f == 1 for f in fused), fused
    w = np.array(snap["wants"][off[r]:off[r + 1]])
    for s, v in zip(shots, want):
        w[70] = v
        assert s.cpu().numpy()[1 + r, 0] == w.sum(), "the block of another tick"
