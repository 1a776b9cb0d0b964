"""CPU checks of the device-memory store calls (no GPU needed): dm_store_load_device and the
three dm_read_*_device calls are declared, exported and bound, the ABI is still 7, a NULL
context is an error, and Engine.load_store_device rejects a bad snapshot before it makes any
library call."""
import ctypes
import re
import subprocess

import pytest

from doorman_amd import _lib

CALLS = ("dm_store_load_device", "dm_read_store_device", "dm_read_store_sums_device", "dm_read_leases_device")


def test_device_io_symbols_are_declared_and_exported():
    syms = _lib.header_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for s in CALLS:
        assert s in syms, s
        assert s in exported, s
        assert s in _lib._SIGS, s


def test_abi_version_is_still_7():
    text = open(_lib.HEADER).read()
    assert re.search(r"^#define DM_ABI_VERSION 7$", text, flags=re.M)
    assert b"abi 7" in _lib.lib().dm_version()


def test_null_context_is_an_error_not_a_crash():
    L = _lib.lib()
    snap = _lib.Snapshot()
    assert L.dm_store_load_device(None, ctypes.byref(snap)) == _lib.DM_E_INVAL
    assert L.dm_read_store_device(None, 0, 0, None, None, None, None) == _lib.DM_E_INVAL
    assert L.dm_read_store_sums_device(None, 0, 0, None, None, None) == _lib.DM_E_INVAL
    assert L.dm_read_leases_device(None, 0, 0, None, None) == _lib.DM_E_INVAL


def test_engine_exposes_the_calls():
    from doorman_amd.engine import Engine
    for name in ("load_store_device", "load_device", "read_store_device", "store_sums_device", "leases_device",
                 "clone_store_to"):
        assert callable(getattr(Engine, name)), name


class _Recorder:
    """Stands where the library, the context or a checked return code would: any use is recorded."""

    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        self._log.append(name)
        raise AssertionError(f"library touched: {name}")

    def __call__(self, *a, **k):
        self._log.append("call")
        raise AssertionError("library touched")


class _StubEngine:
    device = 0

    def __init__(self):
        self.log = []
        self._L = _Recorder(self.log)
        self._ctx = _Recorder(self.log)
        self._chk = _Recorder(self.log)


class _Col:
    """A column as load_store_device takes it: data_ptr(), dtype, device and a length."""

    def __init__(self, n, dtype, device="cuda:0", contiguous=True):
        self.n, self.dtype, self.device, self._contiguous = n, dtype, device, contiguous

    def __len__(self):
        return self.n

    def data_ptr(self):
        raise AssertionError("the pointer is not needed to reject the snapshot")

    def is_contiguous(self):
        return self._contiguous


def _good(R=3, N=10):
    return {"seg_off": _Col(R + 1, "int64"), "wants": _Col(N, "float64"), "has": _Col(N, "float64"),
            "subclients": _Col(N, "int64"), "expiry_ns": _Col(N, "int64")}


def _bad_snapshots():
    import torch
    s = _good()
    s["wants"] = torch.zeros(10, dtype=torch.float64)  # a real tensor, on the CPU
    yield "cpu tensor", s
    s = _good()
    s["has"] = _Col(10, "float64", device="cpu")
    yield "cpu column", s
    s = _good()
    s["expiry_ns"] = _Col(10, "int64", device="cuda:1")
    yield "another device", s
    s = _good()
    s["subclients"] = _Col(10, "int32")
    yield "wrong dtype", s
    s = _good()
    s["wants"] = _Col(10, torch.float32)
    yield "wrong torch dtype", s
    s = _good()
    s["has"] = _Col(9, "float64")
    yield "length mismatch", s
    s = _good()
    s["wants"] = _Col(10, "float64", contiguous=False)
    yield "not contiguous", s
    s = _good()
    s.update(agg_count=_Col(3, "int64"), agg_sum_has=_Col(3, "float64"), agg_sum_wants=_Col(4, "float64"))
    yield "sums of another resource count", s
    s = _good()
    s["seg_off"] = _Col(0, "int64")
    yield "empty seg_off", s


@pytest.mark.parametrize("label", [k for k, _ in _bad_snapshots()])
def test_bad_device_snapshots_are_rejected_before_any_library_call(label):
    from doorman_amd.engine import Engine
    snap = dict(_bad_snapshots())[label]
    stub = _StubEngine()
    stub._device_snapshot = lambda s: Engine._device_snapshot(stub, s)
    stub._DEV_COLS, stub._DEV_AGG = Engine._DEV_COLS, Engine._DEV_AGG
    with pytest.raises(ValueError):
        Engine.load_store_device(stub, snap)
    assert stub.log == [], stub.log


def test_a_good_snapshot_passes_the_contextless_checks():
    """The same stub and columns without a fault: the checks return the shape (so the
    rejections above come from the faults, not from the stub)."""
    from doorman_amd.engine import Engine
    stub = _StubEngine()
    stub._DEV_COLS, stub._DEV_AGG = Engine._DEV_COLS, Engine._DEV_AGG
    R, N, cols = Engine._device_snapshot(stub, _good())
    assert (R, N) == (3, 10) and set(cols) == {"seg_off", "wants", "has", "subclients", "expiry_ns"}
    assert stub.log == []
