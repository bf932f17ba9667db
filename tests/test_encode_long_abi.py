"""dgrep_last_encode_stats on a machine without a GPU (include/dgrep.h): the
symbol is declared, exported and listed; the struct mirror has the header's
size and field order; a NULL context, a NULL `out` and out_size 0 are
DGREP_E_INVALID and write nothing; a short out_size writes only that many
bytes; a larger caller struct gets a zeroed tail. The getter reads host state
only, so a context whose device could not be opened serves. What the fields
hold after an encode is test_gpu_encode_long.py's."""
import ctypes
import re

import dgrep
from test_abi import _declared


def _ctx():
    """a context with or without a device behind it: dgrep_open hands it back either way"""
    L = dgrep.lib()
    h = ctypes.c_void_p()
    assert L.dgrep_open(0, ctypes.byref(h)) in (dgrep.DGREP_OK, dgrep.DGREP_E_HIP)
    assert h.value
    return L, h


def test_symbol_declared_exported_and_listed():
    assert "dgrep_last_encode_stats" in _declared()
    assert hasattr(dgrep.lib(), "dgrep_last_encode_stats")
    assert "dgrep_last_encode_stats" in dgrep.EXPORTS
    assert callable(dgrep.Context.encode_stats)


def test_the_struct_mirrors_the_header():
    import os

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dgrep.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} dgrep_encode_stats;", header)
    assert m
    fields = re.findall(r"^\s*(uint64_t|float)\s+(\w+);", m.group(1), re.M)
    assert fields == [("uint64_t", "records"), ("uint64_t", "long_values"), ("uint64_t", "long_chunks"),
                      ("float", "encode_ms")]
    assert [f for f, _ in dgrep._EncodeStats._fields_] == [name for _, name in fields]
    assert [t for _, t in dgrep._EncodeStats._fields_] == [ctypes.c_uint64] * 3 + [ctypes.c_float]
    assert ctypes.sizeof(dgrep._EncodeStats) == 32  # 3 x 8 + 4, padded to the struct's 8-byte alignment
    assert dgrep._EncodeStats.encode_ms.offset == 24


def test_null_and_zero_size_are_invalid():
    L, h = _ctx()
    try:
        st = dgrep._EncodeStats()
        ctypes.memset(ctypes.byref(st), 0xAB, ctypes.sizeof(st))
        before = bytes(st)
        assert L.dgrep_last_encode_stats(None, ctypes.byref(st), ctypes.sizeof(st)) == dgrep.DGREP_E_INVALID
        assert L.dgrep_last_encode_stats(h, None, ctypes.sizeof(st)) == dgrep.DGREP_E_INVALID
        assert L.dgrep_last_encode_stats(h, ctypes.byref(st), 0) == dgrep.DGREP_E_INVALID
        assert bytes(st) == before  # nothing written
    finally:
        L.dgrep_close(h)


def test_sized_getter_writes_the_callers_size():
    L, h = _ctx()
    try:
        own = ctypes.sizeof(dgrep._EncodeStats)
        raw = (ctypes.c_uint8 * (own + 64))()
        out = ctypes.cast(raw, ctypes.POINTER(dgrep._EncodeStats))
        # a fresh context: every field is 0
        for size in (1, 8, 9, 24, own - 1, own):
            ctypes.memset(raw, 0xAB, len(raw))
            assert L.dgrep_last_encode_stats(h, out, size) == dgrep.DGREP_OK, size
            assert bytes(raw[:size]) == bytes(size), size            # the caller's (shorter) layout, written
            assert bytes(raw[size:]) == b"\xab" * (len(raw) - size), size  # and not a byte behind it
        # a larger (newer) caller struct: the library's bytes, then a zeroed tail, then nothing
        ctypes.memset(raw, 0xAB, len(raw))
        assert L.dgrep_last_encode_stats(h, out, own + 40) == dgrep.DGREP_OK
        assert bytes(raw[:own + 40]) == bytes(own + 40)
        assert bytes(raw[own + 40:]) == b"\xab" * 24
    finally:
        L.dgrep_close(h)
