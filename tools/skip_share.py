"""The share of lease rows a writeback tick leaves bit for bit unchanged, from two
`bench.py --dump-outputs` directories taken one timed step apart:

  python bench.py --steps 20 --dump-outputs A
  python bench.py --steps 21 --dump-outputs B
  python tools/skip_share.py A B [ROWS_PER_RESOURCE]

Both dumps sample the same seeded rows (bench.DUMP_SEED).  Rows are grouped by resource
(lease_rows // ROWS_PER_RESOURCE, 1000 for configs[3]): a resource counts as a fixed
point when every sampled row of it is unchanged.

fixed_share() adds what a tick that recognises such a resource before its passes has to
see unchanged besides the rows: the record it reads (the running sums, and with the
exchange the template's capacity and kind, which k_hier_tick rewrites every step).  A
dump without templates (--hier off) has none to change.

cycle_share() takes three dumps one step apart each (--steps 20, 21, 22) and tells the
resources at a fixed point from those in a cycle of period two (the whole sampled state equal
two ticks apart, not one) and those that differ at both distances:

  python tools/skip_share.py --cycle A B C [ROWS_PER_RESOURCE]
"""
import os
import sys

import numpy as np


def _ld(d, n):
    p = os.path.join(d, n + ".npy")
    return np.load(p) if os.path.exists(p) else None


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _rows_by_resource(dir_a, dir_b, per_res):
    rows = _ld(dir_a, "lease_rows").astype(np.int64)
    assert np.array_equal(rows, _ld(dir_b, "lease_rows").astype(np.int64)), "the dumps sample different rows"
    same = _bits(_ld(dir_a, "lease_gets")) == _bits(_ld(dir_b, "lease_gets"))
    ids, inv = np.unique(rows // per_res, return_inverse=True)
    changed = np.bincount(inv, weights=~same, minlength=len(ids))
    return rows, same, ids, inv, changed == 0


def share(dir_a, dir_b, per_res=1000):
    rows, same, ids, inv, fixed = _rows_by_resource(dir_a, dir_b, per_res)
    # the kernel skips a wave's 64-row run: a sampled row's run is unchanged when every
    # sampled row of the same run is (an upper bound per run, exact per resource)
    return {"rows": int(len(rows)), "row_share": float(same.mean()),
            "resources_sampled": int(len(ids)), "resource_share": float(fixed.mean()),
            "rows_in_fixed_resources": float(fixed[inv].mean()),
            "unchanged_rows_outside_fixed_resources": float((same & ~fixed[inv]).mean())}


def fixed_share(dir_a, dir_b, per_res=1000):
    """Per sampled resource: rows unchanged and record unchanged (it could skip its row
    loads), and rows unchanged but record changed (it would pass the hint and fail the
    confirmation), the latter split by what changed."""
    _, _, ids, _, rows_same = _rows_by_resource(dir_a, dir_b, per_res)

    def field_same(name):
        a, b = _ld(dir_a, name), _ld(dir_b, name)
        if a is None or b is None:
            return None
        return (_bits(a) == _bits(b))[ids]

    tmpl = [field_same("template_capacity"), field_same("template_kind")]
    have_tmpl = tmpl[0] is not None and tmpl[1] is not None
    tmpl_same = tmpl[0] & tmpl[1] if have_tmpl else np.ones(len(ids), bool)
    sums_same = np.ones(len(ids), bool)
    for n in ("resource_count", "resource_sum_has", "resource_sum_wants"):
        s = field_same(n)
        if s is not None:
            sums_same &= s
    out = {"resources_sampled": int(len(ids)), "templates_in_dump": bool(have_tmpl),
           "rows_unchanged": float(rows_same.mean()),
           "rows_and_template_unchanged": float((rows_same & tmpl_same).mean()),
           "rows_template_and_sums_unchanged": float((rows_same & tmpl_same & sums_same).mean()),
           "rows_unchanged_template_changed": float((rows_same & ~tmpl_same).mean()),
           "rows_unchanged_sums_changed": float((rows_same & ~sums_same).mean()),
           "template_changed": float((~tmpl_same).mean())}
    if have_tmpl:
        out["rows_unchanged_capacity_changed"] = float((rows_same & ~tmpl[0]).mean())
        out["rows_unchanged_kind_changed"] = float((rows_same & ~tmpl[1]).mean())
    return out


def _record_same(dir_a, dir_b, ids):
    """Per sampled resource: the running sums and, where the dumps hold them, the template's
    capacity and kind are bit-equal between the two dumps."""
    same = np.ones(len(ids), bool)
    for n in ("resource_count", "resource_sum_has", "resource_sum_wants",
              "template_capacity", "template_kind"):
        a, b = _ld(dir_a, n), _ld(dir_b, n)
        if a is not None and b is not None:
            same &= (_bits(a) == _bits(b))[ids]
    return same


def cycle_share(dir_a, dir_b, dir_c, per_res=1000):
    """From three dumps one timed step apart each (A, B, C): per sampled resource, whether
    its whole sampled state (every sampled row's lease_gets, the running sums, the template)
    is bit-equal one tick apart (A = B and B = C: a fixed point), only two ticks apart
    (A = C, A != B: a cycle of period two), or at neither distance."""
    _, _, ids, _, rows_ab = _rows_by_resource(dir_a, dir_b, per_res)
    _, _, ids_bc, _, rows_bc = _rows_by_resource(dir_b, dir_c, per_res)
    _, _, ids_ac, _, rows_ac = _rows_by_resource(dir_a, dir_c, per_res)
    assert np.array_equal(ids, ids_bc) and np.array_equal(ids, ids_ac)
    ab = rows_ab & _record_same(dir_a, dir_b, ids)
    bc = rows_bc & _record_same(dir_b, dir_c, ids)
    ac = rows_ac & _record_same(dir_a, dir_c, ids)
    fixed = ab & bc
    cycle2 = ac & ~ab
    neither = ~ac & ~ab
    not_fixed = ~fixed
    # what differs between A and B in a two-cycle: rows, or only the record
    cyc_rows = cycle2 & ~rows_ab
    return {"resources_sampled": int(len(ids)),
            "fixed_A=B=C": float(fixed.mean()),
            "not_fixed": float(not_fixed.mean()),
            "cycle2_A=C_A!=B": float(cycle2.mean()),
            "cycle2_with_rows_changing": float(cyc_rows.mean()),
            "differs_at_both_distances": float(neither.mean()),
            "A=B_but_B!=C": float((ab & ~bc).mean()),
            "cycle2_share_of_not_fixed": float(cycle2.sum() / max(int(not_fixed.sum()), 1)),
            "rows_only_cycle2_A=C_A!=B": float((rows_ac & ~rows_ab).mean())}


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--cycle":
        per = int(sys.argv[5]) if len(sys.argv) > 5 else 1000
        for k, v in cycle_share(sys.argv[2], sys.argv[3], sys.argv[4], per).items():
            print(f"{k:40s} {v}")
        sys.exit(0)
    per = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    for k, v in share(sys.argv[1], sys.argv[2], per).items():
        print(f"{k:40s} {v}")
    print()
    for k, v in fixed_share(sys.argv[1], sys.argv[2], per).items():
        print(f"{k:40s} {v}")
