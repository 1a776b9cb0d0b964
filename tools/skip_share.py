"""The share of lease rows a writeback tick leaves bit for bit unchanged, from two
`bench.py --dump-outputs` directories taken one timed step apart:

  python bench.py --steps 20 --dump-outputs A
  python bench.py --steps 21 --dump-outputs B
  python tools/skip_share.py A B [ROWS_PER_RESOURCE]

Both dumps sample the same seeded rows (bench.DUMP_SEED).  Rows are grouped by resource
(lease_rows // ROWS_PER_RESOURCE, 1000 for configs[3]): a resource counts as a fixed
point when every sampled row of it is unchanged.
"""
import os
import sys

import numpy as np


def share(dir_a, dir_b, per_res=1000):
    ld = lambda d, n: np.load(os.path.join(d, n + ".npy"))
    rows = ld(dir_a, "lease_rows").astype(np.int64)
    assert np.array_equal(rows, ld(dir_b, "lease_rows").astype(np.int64)), "the dumps sample different rows"
    same = ld(dir_a, "lease_gets").view(np.int64) == ld(dir_b, "lease_gets").view(np.int64)
    res = rows // per_res
    ids, inv = np.unique(res, return_inverse=True)
    changed = np.bincount(inv, weights=~same, minlength=len(ids))
    fixed = changed == 0
    # the kernel skips a wave's 64-row run: a sampled row's run is unchanged when every
    # sampled row of the same run is (an upper bound per run, exact per resource)
    return {"rows": int(len(rows)), "row_share": float(same.mean()),
            "resources_sampled": int(len(ids)), "resource_share": float(fixed.mean()),
            "rows_in_fixed_resources": float(fixed[inv].mean()),
            "unchanged_rows_outside_fixed_resources": float((same & ~fixed[inv]).mean())}


if __name__ == "__main__":
    per = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    for k, v in share(sys.argv[1], sys.argv[2], per).items():
        print(f"{k:40s} {v}")
