"""CPU checks of dm_keep_keys' C-ABI (no GPU needed): the call is declared, exported, bound
with its prototype, refuses a NULL context, is documented with dm_plan_info's slot 23, and
only adds to ABI 7."""
import ctypes
import re
import subprocess

from doorman_amd import _lib


def test_keep_keys_is_declared_and_exported():
    syms = _lib.header_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "dm_keep_keys" in syms
    assert "dm_keep_keys" in exported


def test_keep_keys_prototype_loads():
    L = _lib.lib()
    assert L.dm_keep_keys.restype is ctypes.c_int
    assert L.dm_keep_keys.argtypes == [ctypes.c_void_p, ctypes.c_int]


def test_keep_keys_null_context_is_an_error_not_a_crash():
    L = _lib.lib()
    assert L.dm_keep_keys(None, 1) == _lib.DM_E_INVAL
    assert L.dm_keep_keys(None, 0) == _lib.DM_E_INVAL


def test_header_documents_the_call_and_abi_is_still_7():
    text = open(_lib.HEADER).read()
    assert re.search(r"^#define DM_ABI_VERSION 7$", text, flags=re.M)
    assert b"abi 7" in _lib.lib().dm_version()
    assert re.search(r"^int dm_keep_keys\(dm_ctx\* ctx, int on\);$", text, flags=re.M)
    doc = text[:text.index("int dm_keep_keys(")].rsplit("/*", 1)[1]
    for phrase in ("dm_store_update_wants", "dm_store_update_wants_mask", "NaN", "row epoch", "Default off",
                   "DM_E_INVAL"):
        assert phrase in doc, phrase
    info = text[:text.index("int dm_plan_info(")].rsplit("/*", 1)[1]
    assert "slot 23" in info and "dm_keep_keys" in info and "returns 24" in info


def test_engine_exposes_the_call_and_names_the_slot():
    from doorman_amd import engine
    assert callable(engine.Engine.keep_keys)
    assert engine._BIN_NAMES[23] == "kept_refreshes"
