"""dm_destroy returns every byte of device memory its context allocated (dm_ctx.h: the
buffers free themselves with the context).  Contexts that load a store, tick and close,
over and over in one process -- a long-lived host re-creating contexts (dm_server, the
cgo binding of INTEGRATION.md) -- must not lose free memory with each one.  Before the
buffers owned their memory, the released-row masks (N/2 + 64 B), the workgroup bins' item
index (4 R B) and the tile list were allocated and never freed: 4.03 MiB per cycle of
the store below, ~24 MiB over a window of six."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

R, ROWS = 8192, 1024  # N = 2^23 rows in a workgroup bin: item_of and rmask are both live
CYCLES = 6
# half of what a leak of the masks and the item index must lose over a window, so that
# allocator granularity cannot hide it
BOUND = 12 << 20

# One process: a warm-up cycle (the stream pool, the code objects and the runtime's first
# allocations), then two windows of CYCLES cycles, free memory read around each.  A leak
# shows in both windows; a neighbour's allocation on a shared GPU is very unlikely to land
# in both, so the smaller drop is what counts.
CHILD = """
import json, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch
from doorman_amd import workloads as W
from doorman_amd.engine import Engine
torch.cuda.set_device(0)
snap = W.make_snapshot(np.full(%(R)d, %(rows)d), 1.0, 0.0, 1, W.NOW_NS + 60 * W.NS, W.FAIR_SHARE, 1000.0)
def cycle():
    e = Engine(0, %(lib)r)
    e.load(snap)
    e.apportion(W.NOW_NS, writeback=True)
    e.sync()
    e.close()
def free():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]
cycle()
drops = []
for w in range(2):
    f0 = free()
    for k in range(%(cycles)d):
        cycle()
    drops.append(f0 - free())
print(json.dumps({"drops": drops}), flush=True)
"""


def window_drops(lib_path=None):
    """Bytes of free device memory lost over each of the child's two windows."""
    code = CHILD % {"root": ROOT, "R": R, "rows": ROWS, "lib": lib_path, "cycles": CYCLES}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])["drops"]


def test_destroyed_contexts_return_their_device_memory():
    drops = window_drops()
    print("free memory lost over %d load-tick-close cycles, two windows: %s MiB"
          % (CYCLES, [round(d / 2**20, 2) for d in drops]))
    assert min(drops) < BOUND, drops
