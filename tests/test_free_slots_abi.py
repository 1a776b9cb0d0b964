"""CPU checks of DM_KEEP_FREE_SLOTS' C-ABI (no GPU needed): the third bit of dm_keep_keys'
argument is named in the header and the binding, described in the one comment block in front
of dm_keep_keys, dm_plan_info's new slot is documented and named, a NULL context is refused
with every bit set, and the additions leave the ABI at 7."""
import re

from doorman_amd import _lib


def test_the_bit_is_named():
    text = open(_lib.HEADER).read()
    assert re.search(r"^#define DM_KEEP_FREE_SLOTS 4$", text, flags=re.M)
    assert _lib.DM_KEEP_FREE_SLOTS == 4
    assert _lib.DM_KEEP_REFRESH | _lib.DM_KEEP_UPDATES | _lib.DM_KEEP_FREE_SLOTS == 7


def test_null_is_an_error_not_a_crash():
    assert _lib.lib().dm_keep_keys(None, 7) == _lib.DM_E_INVAL


def test_abi_is_still_7_and_the_header_describes_the_bit():
    text = open(_lib.HEADER).read()
    assert re.search(r"^#define DM_ABI_VERSION 7$", text, flags=re.M)
    assert b"abi 7" in _lib.lib().dm_version()
    doc = text[:text.index("int dm_keep_keys(")].rsplit("/*", 1)[1]
    for phrase in ("DM_KEEP_REFRESH", "DM_KEEP_UPDATES", "DM_KEEP_FREE_SLOTS", "released rows", "pending arrival",
                   "at least one live row", "keeps a key", "two-tick cycle", "bit for bit"):
        assert phrase in doc, phrase
    info = text[:text.index("int dm_plan_info(")].rsplit("/*", 1)[1]
    assert "returns 24" in info and "slot 25" in info and "DM_KEEP_FREE_SLOTS" in info
    assert info.rstrip().rstrip("*/").rstrip().endswith("returns 26")


def test_engine_names_the_slot_and_the_bit():
    from doorman_amd import engine
    assert engine._BIN_NAMES[25] == "masked_parts" and len(engine._BIN_NAMES) == 26
    assert "DM_KEEP_FREE_SLOTS" in engine.Engine.keep_keys.__doc__
