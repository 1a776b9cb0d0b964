"""CPU checks of DM_KEEP_UPDATES' C-ABI (no GPU needed): dm_keep_keys' bits are named in the
header and the binding, dm_keep_stats is declared, exported, bound with its prototype and
refuses a NULL context, and the additions leave the ABI at 7."""
import ctypes
import re
import subprocess

from doorman_amd import _lib


def test_the_mode_bits_are_named():
    text = open(_lib.HEADER).read()
    assert re.search(r"^#define DM_KEEP_REFRESH 1$", text, flags=re.M)
    assert re.search(r"^#define DM_KEEP_UPDATES 2$", text, flags=re.M)
    assert (_lib.DM_KEEP_REFRESH, _lib.DM_KEEP_UPDATES) == (1, 2)


def test_keep_stats_is_declared_exported_and_bound():
    assert "dm_keep_stats" in _lib.header_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "dm_keep_stats" in {line.split()[-1] for line in out.splitlines() if " T " in line}
    text = open(_lib.HEADER).read()
    assert re.search(r"^int dm_keep_stats\(dm_ctx\* ctx, int64_t\* out, int max\);$", text, flags=re.M)
    L = _lib.lib()
    assert L.dm_keep_stats.restype is ctypes.c_int
    assert L.dm_keep_stats.argtypes == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int]


def test_keep_stats_null_is_an_error_not_a_crash():
    L = _lib.lib()
    arr = (ctypes.c_int64 * 6)()
    assert L.dm_keep_stats(None, arr, 6) == _lib.DM_E_INVAL
    assert L.dm_keep_keys(None, 3) == _lib.DM_E_INVAL


def test_abi_is_still_7_and_the_header_says_which_writers_start_an_epoch():
    text = open(_lib.HEADER).read()
    assert re.search(r"^#define DM_ABI_VERSION 7$", text, flags=re.M)
    assert b"abi 7" in _lib.lib().dm_version()
    doc = text[:text.index("int dm_keep_keys(")].rsplit("/*", 1)[1]
    for phrase in ("DM_KEEP_REFRESH", "DM_KEEP_UPDATES", "dm_store_release", "dm_store_upsert", "dm_store_apply",
                   "dm_store_apply_async", "dm_decide", "dm_store_clean"):
        assert phrase in doc, phrase
    info = text[:text.index("int dm_plan_info(")].rsplit("/*", 1)[1]
    assert "returns 24" in info  # dm_plan_info is not extended


def test_engine_passes_the_bits_and_reads_the_counters():
    from doorman_amd import engine
    assert callable(engine.Engine.keep_keys) and callable(engine.Engine.keep_stats)
