"""CPU checks of Clean's C-ABI (no GPU needed): dm_store_clean and dm_read_cleaned are
declared, exported, bound with their prototypes, refuse a NULL context, and the change
only adds to ABI 7."""
import ctypes
import re
import subprocess

from doorman_amd import _lib


def test_clean_symbols_are_declared_and_exported():
    syms = _lib.header_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for s in ("dm_store_clean", "dm_read_cleaned"):
        assert s in syms, s
        assert s in exported, s


def test_clean_prototypes_load():
    L = _lib.lib()
    assert L.dm_store_clean.restype is ctypes.c_int
    assert L.dm_store_clean.argtypes == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32,
                                         ctypes.POINTER(_lib.CleanResult)]
    assert L.dm_read_cleaned.restype is ctypes.c_int
    assert L.dm_read_cleaned.argtypes == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    assert [(n, t) for n, t in _lib.CleanResult._fields_] == [("released", ctypes.c_int64),
                                                              ("next_expiry_ns", ctypes.c_int64)]
    assert ctypes.sizeof(_lib.CleanResult) == 16


def test_clean_null_context_is_an_error_not_a_crash():
    L = _lib.lib()
    res = _lib.CleanResult()
    assert L.dm_store_clean(None, 0, 0, ctypes.byref(res)) == _lib.DM_E_INVAL
    assert L.dm_store_clean(None, 0, _lib.DM_CLEAN_PEEK, None) == _lib.DM_E_INVAL
    rows = (ctypes.c_int64 * 2)()
    assert L.dm_read_cleaned(None, 0, 2, rows) == _lib.DM_E_INVAL
    assert L.dm_read_cleaned(None, 0, 0, None) == _lib.DM_E_INVAL


def test_abi_is_still_7_and_the_constants_agree():
    text = open(_lib.HEADER).read()
    assert re.search(r"^#define DM_ABI_VERSION 7$", text, flags=re.M)
    assert re.search(r"^#define DM_CLEAN_PEEK 1u\b", text, flags=re.M)
    assert re.search(r"^#define DM_NO_EXPIRY INT64_MAX\b", text, flags=re.M)
    assert _lib.DM_CLEAN_PEEK == 1
    assert _lib.DM_NO_EXPIRY == 2**63 - 1
    assert b"abi 7" in _lib.lib().dm_version()
    assert re.search(r"LeaseStore\.Clean\s+go/server/doorman/store\.go:169-181\s+-> dm_store_clean", text)


def test_engine_exposes_the_calls():
    from doorman_amd.engine import Engine
    assert callable(Engine.clean) and callable(Engine.read_cleaned)
