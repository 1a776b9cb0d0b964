"""CPU checks of dm_decide_assign (no GPU needed): the call is declared in the public header,
exported by the library and bound with its argument types, the ABI is still 7 (a call was only
added), a NULL context is an error that writes no output, and the Engine carries the method."""
import ctypes
import inspect
import re
import subprocess

import numpy as np

from doorman_amd import _lib


def test_decide_assign_is_declared_exported_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "dm_decide_assign" in _lib.header_symbols()
    assert "dm_decide_assign" in exported
    res, args = _lib._SIGS["dm_decide_assign"]
    # ctx, now_ns, n, then rows, has, wants, subclients, gets, expiry_ns, safe_capacity
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_void_p] * 7
    fn = _lib.lib().dm_decide_assign
    assert fn.argtypes == args and fn.restype is ctypes.c_int
    # dm_decide's arguments and one more: the header declares it that way too
    text = open(_lib.HEADER).read()
    decl = re.search(r"int dm_decide_assign\(([^;]*)\);", text).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == [
        "ctx", "now_ns", "n", "rows", "has", "wants", "subclients", "gets", "expiry_ns", "safe_capacity"]


def test_abi_version_is_still_7():
    text = open(_lib.HEADER).read()
    assert re.search(r"^#define DM_ABI_VERSION 7$", text, flags=re.M)
    assert b"abi 7" in _lib.lib().dm_version()


def test_null_context_is_an_error_and_writes_no_output():
    L = _lib.lib()
    rows, sub = np.zeros(2, np.int64), np.ones(2, np.int64)
    has, wants = np.zeros(2), np.ones(2)
    gets, safe, exp = np.full(2, 7.5), np.full(2, 8.5), np.full(2, 9, np.int64)
    p = [a.ctypes.data for a in (rows, has, wants, sub, gets, exp, safe)]
    assert L.dm_decide_assign(None, 5, 2, *p) == _lib.DM_E_INVAL
    assert L.dm_decide_assign(None, 5, 0, *[None] * 7) == _lib.DM_E_INVAL
    assert (gets == 7.5).all() and (safe == 8.5).all() and (exp == 9).all()


def test_engine_exposes_decide_assign():
    from doorman_amd.engine import Engine
    assert callable(Engine.decide_assign)
    params = list(inspect.signature(Engine.decide_assign).parameters)
    assert params == ["self", "now_ns", "rows", "has", "wants", "subclients", "safe"]
    assert inspect.signature(Engine.decide_assign).parameters["safe"].default is False
