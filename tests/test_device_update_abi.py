"""CPU checks of the store updates from device memory (no GPU needed): the six device twins
of the update calls and dm_store_refresh_wants_device are declared, exported and bound, the
ABI is still 7 (calls were only added), a NULL context is an error, and the Engine methods
reject bad columns before they make any library call."""
import ctypes
import re
import subprocess

import pytest

from doorman_amd import _lib

CALLS = ("dm_store_upsert_device", "dm_store_update_wants_device", "dm_store_update_wants_mask_device",
         "dm_store_release_device", "dm_store_apply_device", "dm_store_apply_device_async",
         "dm_store_refresh_wants_device")


def test_device_update_symbols_are_declared_exported_and_bound():
    syms = _lib.header_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    L = _lib.lib()
    for s in CALLS:
        assert s in syms, s
        assert s in exported, s
        assert s in _lib._SIGS, s
        assert getattr(L, s).argtypes == _lib._SIGS[s][1], s


def test_abi_version_is_still_7():
    text = open(_lib.HEADER).read()
    assert re.search(r"^#define DM_ABI_VERSION 7$", text, flags=re.M)
    assert b"abi 7" in _lib.lib().dm_version()


def test_null_context_is_an_error_not_a_crash():
    L = _lib.lib()
    b = _lib.StoreBatch()
    n = ctypes.c_int64(5)
    assert L.dm_store_upsert_device(None, 0, None, None, None, None, None) == _lib.DM_E_INVAL
    assert L.dm_store_update_wants_device(None, 0, None, None) == _lib.DM_E_INVAL
    assert L.dm_store_update_wants_mask_device(None, 0, 0, None, 0, None) == _lib.DM_E_INVAL
    assert L.dm_store_release_device(None, 0, None) == _lib.DM_E_INVAL
    assert L.dm_store_apply_device(None, ctypes.byref(b)) == _lib.DM_E_INVAL
    assert L.dm_store_apply_device_async(None, ctypes.byref(b)) == _lib.DM_E_INVAL
    assert L.dm_store_refresh_wants_device(None, 0, 0, None, ctypes.byref(n)) == _lib.DM_E_INVAL
    assert n.value == 5, "a refused call writes no count"


def test_engine_exposes_the_calls():
    from doorman_amd.engine import Engine
    for name in ("upsert_device", "update_wants_device", "update_wants_mask_device", "release_device", "apply_device",
                 "refresh_wants_device"):
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
        from doorman_amd.engine import Engine
        self.log = []
        self._L = _Recorder(self.log)
        self._ctx = _Recorder(self.log)
        self._chk = _Recorder(self.log)
        self._torch_ready = _Recorder(self.log)
        self._device_cols = lambda *cols: Engine._device_cols(self, *cols)


class _Col:
    """A column as the methods take it: data_ptr(), dtype, device and a length."""

    def __init__(self, n, dtype, device="cuda:0", contiguous=True):
        self.n, self.dtype, self.device, self._contiguous = n, dtype, device, contiguous

    def __len__(self):
        return self.n

    def data_ptr(self):
        raise AssertionError("the pointer is not needed to reject the column")

    def is_contiguous(self):
        return self._contiguous


def _bad_calls():
    """(label, method, args, kwargs): each has exactly one fault."""
    import torch
    f, i = "float64", "int64"
    yield "upsert: cpu tensor", "upsert_device", (_Col(4, i), torch.zeros(4, dtype=torch.float64), _Col(4, f), _Col(4, i), _Col(4, i)), {}
    yield "upsert: wrong dtype", "upsert_device", (_Col(4, i), _Col(4, f), _Col(4, f), _Col(4, "int32"), _Col(4, i)), {}
    yield "upsert: lengths", "upsert_device", (_Col(4, i), _Col(4, f), _Col(3, f), _Col(4, i), _Col(4, i)), {}
    yield "update_wants: another device", "update_wants_device", (_Col(4, i, device="cuda:1"), _Col(4, f)), {}
    yield "update_wants: not contiguous", "update_wants_device", (_Col(4, i), _Col(4, f, contiguous=False)), {}
    yield "update_wants: lengths", "update_wants_device", (_Col(4, i), _Col(5, f)), {}
    yield "mask: float mask", "update_wants_mask_device", (_Col(2, f), _Col(4, f)), {}
    yield "mask: cpu wants", "update_wants_mask_device", (_Col(2, i), _Col(4, f, device="cpu")), {}
    yield "release: wrong dtype", "release_device", (_Col(4, "int32"),), {}
    yield "release: numpy", "release_device", (__import__("numpy").zeros(4, "int64"),), {}
    yield "apply: cpu release rows", "apply_device", (), {"release_rows": _Col(4, i, device="cpu")}
    yield "apply: upsert lengths", "apply_device", (), {"upsert": (_Col(4, i), None, _Col(3, f), _Col(4, "int32"), None), "now_ns": 5}
    yield "apply: narrow without now_ns", "apply_device", (), {"upsert": (_Col(4, i), None, _Col(4, f), _Col(4, "int32"), None)}
    yield "apply: float32 wants", "apply_device", (), {"wants_mask": _Col(2, "uint64"), "wants": _Col(4, torch.float32)}
    yield "apply: wants without a mask", "apply_device", (), {"wants": _Col(4, f)}
    yield "refresh: wrong dtype", "refresh_wants_device", (_Col(64, "float32"),), {}
    yield "refresh: cpu tensor", "refresh_wants_device", (torch.zeros(64, dtype=torch.float64),), {}
    yield "refresh: not contiguous", "refresh_wants_device", (_Col(64, f, contiguous=False),), {}


@pytest.mark.parametrize("label", [c[0] for c in _bad_calls()])
def test_bad_device_columns_are_rejected_before_any_library_call(label):
    from doorman_amd.engine import Engine
    _, method, args, kwargs = next(c for c in _bad_calls() if c[0] == label)
    stub = _StubEngine()
    with pytest.raises(ValueError):
        getattr(Engine, method)(stub, *args, **kwargs)
    assert stub.log == [], stub.log


def test_good_columns_pass_the_contextless_checks():
    """The same stub and columns without a fault: the checks return the length (so the
    rejections above come from the faults, not from the stub)."""
    from doorman_amd.engine import Engine
    stub = _StubEngine()
    n = Engine._device_cols(stub, ("rows", _Col(7, "int64"), "int64"), ("wants", _Col(7, "float64"), "float64"),
                            ("subclients", _Col(7, "int32"), ("int64", "int32")))
    assert n == 7 and stub.log == []
