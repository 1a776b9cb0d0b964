"""CPU checks of the re-layout's C-ABI (no GPU needed): dm_store_relayout and
dm_server_stats are declared, exported, bound with their prototypes, and the header, the
library and the binding agree on ABI 7."""
import ctypes
import re
import subprocess

from doorman_amd import _lib


def test_relayout_symbols_are_declared_and_exported():
    syms = _lib.header_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for s in ("dm_store_relayout", "dm_server_stats"):
        assert s in syms, s
        assert s in exported, s


def test_relayout_prototypes_load():
    L = _lib.lib()
    assert L.dm_store_relayout.restype is ctypes.c_int
    assert L.dm_store_relayout.argtypes == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint32,
                                            ctypes.c_void_p]
    assert L.dm_server_stats.restype is ctypes.c_int
    assert L.dm_server_stats.argtypes == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int]


def test_relayout_null_arguments_are_errors_not_crashes():
    L = _lib.lib()
    off = (ctypes.c_int64 * 2)(0, 4)
    assert L.dm_store_relayout(None, 1, off, 0, None) == _lib.DM_E_INVAL
    out = (ctypes.c_int64 * 2)()
    assert L.dm_server_stats(None, out, 2) == _lib.DM_E_INVAL


def test_abi_version_is_7_everywhere():
    text = open(_lib.HEADER).read()
    assert re.search(r"^#define DM_ABI_VERSION 7$", text, flags=re.M)
    assert re.search(r"^#define DM_RELAYOUT_COMPACT 1u$", text, flags=re.M)
    assert _lib.DM_RELAYOUT_COMPACT == 1
    assert b"abi 7" in _lib.lib().dm_version()


def test_engine_and_server_expose_the_calls():
    from doorman_amd.engine import Engine
    from doorman_amd.server import TickServer
    assert callable(Engine.relayout) and callable(TickServer.stats)
