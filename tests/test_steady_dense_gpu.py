"""The steady builds of the dense tick kernel (dm_tick_group.hip group_segment STEADY,
dm_tick.cpp's launch policy).

A bin part whose items are all dense, none with a released row or an arrival, runs outside
recompute mode a build of k_block_dense that takes Clean's result as known (nothing
released, every row live with the hint's subclient count) instead of computing it; an
item it is not known for -- a follower lapse, which only the device can tell -- goes to
the rest kernel that follows every steady launch.  Nothing the caller can read may depend
on which build ran: engine A (DM_STEADY=0, today's builds) and engine B (the default)
must hold identical bits after every tick of a sequence that enters and leaves the steady
state every way there is, and dm_plan_info's "steady_parts" says whether the build was
engaged at all.

The store: two resources at each first and last row count of every dense instance (257 ...
4096, most no multiple of 64), kinds 0-3 in every bin, one of them in learning mode,
subclient counts 1, 3 and 254, 20-s leases, of each pair one under and one over capacity;
and one resource of 255 subclients, which is never dense: among the workgroup bins (its
part then never runs steady and its dense kernel keeps queueing for the rest kernel) or
among the sub-wave bins (every workgroup bin can run steady)."""
import numpy as np
import pytest

from doorman_amd import workloads as W
from oracle import oracle as O
import hier_model as M
from parity_util import assert_leases_match

pytestmark = pytest.mark.gpu

NOW = W.NOW_NS
EDGES = [257, 512, 513, 1000, 1024, 1025, 2048, 2049, 4096]
COLS = ("has", "wants", "subclients", "expiry_ns")
SUBS = (1, 3, 254)
LEARNING = 13  # the second 2048-row resource
R_NAN, R_INF = 7, 11  # FairShare: 1000 rows (bin 4), 1025 rows (bin 5)
R_REL = 16  # 4096 rows (bin 6), Static


def make_store(odd):
    rng = np.random.default_rng(20)
    sizes, kinds, caps, wants, subs = [], [], [], [], []
    for i, n in enumerate(EDGES):
        for j in range(2):
            r = len(sizes)
            s0 = SUBS[r % 3]
            sizes.append(n)
            kinds.append((2 * i + j) % 4)
            C = 4096.0
            # per subclient: under capacity (sum of wants about C / 4) or about twice over
            w = rng.uniform(0.0, 1.0, n) * ((0.5 if j == 0 else 4.0) * C / n)
            caps.append(C)
            wants.append(w)
            subs.append(np.full(n, s0, np.int64))
    sizes.append(odd)
    kinds.append(3)
    caps.append(500.0)
    wants.append(rng.uniform(0.0, 3.0, odd) * (500.0 / odd))
    subs.append(np.full(odd, 255, np.int64))
    assert kinds[R_NAN] == 3 and kinds[R_INF] == 3 and sizes[R_NAN] == 1000 and sizes[R_INF] == 1025
    wants = np.concatenate(wants)
    N = len(wants)
    cap_row = np.repeat(np.asarray(caps), sizes) / np.repeat(np.asarray(sizes, np.float64), sizes)
    has = rng.uniform(0.0, 0.4, N) * cap_row
    exp = NOW + rng.integers(30, 300, N, dtype=np.int64) * W.NS
    learn = np.full(len(sizes), W.INT64_MIN, np.int64)
    learn[LEARNING] = NOW + 1000 * W.NS
    return W.make_snapshot(sizes, wants, has, np.concatenate(subs), exp, np.asarray(kinds, np.int32),
                           np.asarray(caps), lease_length_s=20, refresh_interval_s=5, learning_end_ns=learn)


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


def assert_same_state(A, B, label):
    sa, sb = A.read_store(), B.read_store()
    for k in COLS:
        np.testing.assert_array_equal(sa[k].view(np.int64), sb[k].view(np.int64), err_msg=f"{label}: {k}")
    for x, y, k in zip(A.leases(), B.leases(), ("gets", "expiry")):
        np.testing.assert_array_equal(x.view(np.int64), y.view(np.int64), err_msg=f"{label}: leases {k}")
    for what, ra, rb in (("resources", A.resources(), B.resources()), ("config", A.config(), B.config())):
        for k in ra:
            assert ra[k].tobytes() == rb[k].tobytes(), f"{label}: {what} {k}"


def engines(monkeypatch, n=1):
    """n engines with DM_STEADY=0 and n with the default (read when the context is created)."""
    from doorman_amd.engine import Engine
    monkeypatch.setenv("DM_STEADY", "0")
    a = [Engine(0) for _ in range(n)]
    monkeypatch.delenv("DM_STEADY")
    return a, [Engine(0) for _ in range(n)]


@pytest.mark.parametrize("odd", [300, 40])
def test_steady_and_plain_builds_agree_bit_for_bit(monkeypatch, odd):
    """Engine A with DM_STEADY=0, engine B with the default, identical bits after every tick
    of: three writeback ticks; a wants refresh with a NaN and a +Inf wants in FairShare
    resources, two ticks; a release, a tick; an arrival into the freed slot, a tick; a
    capacity halved, a tick; a non-writeback tick; a recompute tick; a tick 25 s later (every
    follower of the 20-s leases lapses together) and the tick after it.  B engages the steady
    build on the ticks that can be steady (all four workgroup bins with odd = 40, the
    255-subclient resource then in a sub-wave bin; three with odd = 300) and on none after a
    release, an arrival or in recompute mode; A never.  The third tick matches the oracle."""
    snap = make_store(odd)
    off = np.asarray(snap["seg_off"])
    (A,), (B,) = engines(monkeypatch)
    try:
        A.load(snap)
        B.load(snap)
        host = copy_of(snap)

        def both(fn):
            fn(A)
            fn(B)

        def tick(label, dt, steady, writeback=True, recompute=False):
            """steady: True = B's steady_parts positive, False = zero, None = the policy's choice"""
            both(lambda e: e.apportion(NOW + dt * W.NS, writeback=writeback, recompute=recompute))
            assert A.plan_info()["steady_parts"] == 0, label
            got = B.plan_info()["steady_parts"]
            if steady is not None:
                assert (got > 0) == steady, f"{label}: steady_parts {got}"
            assert_same_state(A, B, label)
            return got

        freed = np.array([off[R_REL] + 700], np.int64)
        all_bins = 4 if odd < 257 else 3
        tick("tick 1", 0, False)  # no hints before the first writeback tick
        host_tick(host, NOW)
        assert tick("tick 2", 2, True) == all_bins
        host_tick(host, NOW + 2 * W.NS)
        ref = O.apportion(host, NOW + 4 * W.NS)
        assert tick("tick 3", 4, True) == all_bins
        assert_leases_match(host, *B.leases(), ref, "tick 3")

        rows = np.array([off[R_NAN] + 70, off[R_INF] + 1024, off[0] + 256, off[17] + 4000, off[2] + 100], np.int64)
        nw = np.array([np.nan, np.inf, 0.125, 7.5, 0.0])
        both(lambda e: e.update_wants(rows, nw))
        tick("tick 4 (wants refresh)", 6, False)  # a new row epoch: nothing verified yet
        tick("tick 5", 8, True)
        both(lambda e: e.release(freed))
        tick("tick 6 (release)", 10, False)
        both(lambda e: e.upsert(freed, np.zeros(1), np.full(1, 0.125), np.full(1, SUBS[R_REL % 3], np.int64),
                                np.full(1, NOW + 112 * W.NS)))
        tick("tick 7 (arrival)", 12, False)
        cfg = copy_of(snap)
        cfg["capacity"][9] *= 0.5  # 1000 rows, FairShare, over capacity
        both(lambda e: e.load_config(cfg))
        tick("tick 8 (capacity)", 14, False)  # (a configuration load starts a row epoch too)
        tick("tick 9", 16, True)
        tick("tick 10 (no writeback)", 18, None, writeback=False)
        tick("tick 11 (recompute)", 20, False, recompute=True)
        tick("tick 12", 22, True)
        tick("tick 13 (lapse)", 47, None)
        gets, exp = B.leases()
        assert not gets.any() and (exp == W.RELEASED).all()  # every follower lapsed
        tick("tick 14", 49, None)
    finally:
        A.close()
        B.close()


def test_steady_build_under_the_exchange(monkeypatch):
    """A leaf under the pipelined exchange (dm_hier_step: capacities, lease lengths and parent
    expiries change on the device from step to step, among them 7-s leases that lapse over
    the 8-s gap, which only the device can tell): leases, templates in use, the root's rows
    and its verdict on every request are the same bits with and without the steady builds,
    and the leaf's bins run them before and after the lapse."""
    import torch
    from doorman_amd.hierarchy import HierarchicalTick, root_snapshot
    torch.cuda.set_device(0)
    rng = np.random.default_rng(21)
    sizes = np.concatenate([rng.integers(257, 1100, 60), rng.integers(1025, 4097, 6)])
    R = len(sizes)
    rcfg = {"kind": rng.choice([W.FAIR_SHARE, W.PROPORTIONAL_SHARE, W.STATIC, W.NO_ALGORITHM], R).astype(np.int32),
            "capacity": rng.choice([100.0, 1000.0, 2500.5], R),
            "lease_length_s": rng.choice([7, 20, 60], R).astype(np.int64),
            "refresh_interval_s": rng.choice([1, 5], R).astype(np.int64),
            "learning_end_ns": np.full(R, W.INT64_MIN, np.int64),
            "parent_expiry_ns": np.full(R, W.INT64_MAX, np.int64),
            "safe_capacity": np.where(rng.random(R) < 0.5, np.nan, rng.uniform(1, 9, R))}
    full = W.make_snapshot(sizes, rng.uniform(0.2, 3.0, int(sizes.sum())) * 1000.0 / np.repeat(sizes, sizes),
                           0.0, 1, NOW + 60 * W.NS, W.FAIR_SHARE, 1000.0)
    steps = [NOW + t * W.NS for t in (0, 2, 4, 6, 8, 16, 18, 20)]
    (la, ra), (lb, rb) = engines(monkeypatch, 2)
    try:
        runs = []
        for leaf, root in ((la, ra), (lb, rb)):
            leaf.load(M.with_config(full, M.default_config(R)))
            root.load(M.with_config(root_snapshot(R, 1, W.FAIR_SHARE, 1.0), rcfg))
            ht = HierarchicalTick(torch, leaf, root, R, 1, 0, None, shard_lo=np.array([0, R]), pipelined=True,
                                  native="local")
            out, steady = [], []
            for now in steps:
                ht.tick(now)
                steady.append(leaf.plan_info()["steady_parts"])
                out.append((leaf.leases(), leaf.config(), leaf.read_store(), root.read_store(), ht.status()))
            runs.append((out, steady))
        (oa, sa), (ob, sb) = runs
        assert not any(sa) and sb[2] > 0 and sb[-1] > 0, (sa, sb)
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
