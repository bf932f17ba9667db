"""The windowed scan's C ABI on a machine without a GPU (include/dgrep.h,
dgrep_scan_windowed / dgrep_stream_*): the symbols are declared, exported and
listed; the result struct's layout; every argument check returns its status
with the result zeroed, before any GPU call; well-formed arguments reach
DGREP_E_NO_DFA; free and close accept NULL and a zeroed struct."""
import ctypes

import pytest

import dgrep
from test_abi import _cpu_ctx, _declared

NEW = ("dgrep_scan_windowed", "dgrep_stream_open", "dgrep_stream_feed", "dgrep_stream_finish",
       "dgrep_stream_result_free", "dgrep_stream_close", "dgrep_stream_stats")


def test_symbols_declared_exported_and_listed():
    L = dgrep.lib()
    declared = _declared()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in dgrep.EXPORTS, name


def test_struct_layouts():
    assert ctypes.sizeof(dgrep._StreamResult) == 48
    assert [f for f, _ in dgrep._StreamResult._fields_] == ["count", "line_no", "start", "len", "value_off", "values"]
    assert ctypes.sizeof(dgrep._ScanStats) == 80
    assert dgrep.STREAM_VALUES == 1


def _dirty(struct):
    r = struct()
    ctypes.memset(ctypes.byref(r), 0xAB, ctypes.sizeof(r))
    return r


def _zeroed(r):
    return bytes(r) == bytes(ctypes.sizeof(r))


BAD_WINDOWS = [0, 1, 4095, 4097, 2048, 6144, 8191, (1 << 40) + 4096, 1 << 41, (1 << 64) - 4096]
GOOD_WINDOWS = [4096, 8192, 12288, 64 << 20, 1 << 40]


def test_scan_windowed_argument_checks():
    L, h = _cpu_ctx()
    try:
        data = ctypes.create_string_buffer(b"an error\n", 9)
        r = _dirty(dgrep._Result)
        assert L.dgrep_scan_windowed(None, data, 9, 4096, ctypes.byref(r)) == dgrep.DGREP_E_INVALID
        assert _zeroed(r)
        assert L.dgrep_scan_windowed(h, data, 9, 4096, None) == dgrep.DGREP_E_INVALID
        r = _dirty(dgrep._Result)
        assert L.dgrep_scan_windowed(h, None, 9, 4096, ctypes.byref(r)) == dgrep.DGREP_E_INVALID  # n without data
        assert _zeroed(r)
        for w in BAD_WINDOWS:
            r = _dirty(dgrep._Result)
            assert L.dgrep_scan_windowed(h, data, 9, w, ctypes.byref(r)) == dgrep.DGREP_E_INVALID, w
            assert _zeroed(r), w
            assert b"4096" in L.dgrep_last_error(h)
        for w in GOOD_WINDOWS:
            for ptr, n in ((data, 9), (None, 0)):
                r = _dirty(dgrep._Result)
                assert L.dgrep_scan_windowed(h, ptr, n, w, ctypes.byref(r)) == dgrep.DGREP_E_NO_DFA, w
                assert _zeroed(r), w
    finally:
        L.dgrep_close(h)


def test_stream_open_argument_checks():
    L, h = _cpu_ctx()
    try:
        s = ctypes.c_void_p(0xABAB)
        assert L.dgrep_stream_open(None, 4096, 0, ctypes.byref(s)) == dgrep.DGREP_E_INVALID
        assert s.value is None
        assert L.dgrep_stream_open(h, 4096, 0, None) == dgrep.DGREP_E_INVALID
        for flags in (2, 3, 4, 0x80000000, 0xFFFFFFFF):  # unknown flag bits
            s = ctypes.c_void_p(0xABAB)
            assert L.dgrep_stream_open(h, 4096, flags, ctypes.byref(s)) == dgrep.DGREP_E_INVALID, flags
            assert s.value is None
        for w in BAD_WINDOWS:
            s = ctypes.c_void_p(0xABAB)
            assert L.dgrep_stream_open(h, w, 0, ctypes.byref(s)) == dgrep.DGREP_E_INVALID, w
            assert s.value is None
        for w in GOOD_WINDOWS:
            for flags in (0, dgrep.STREAM_VALUES):
                s = ctypes.c_void_p(0xABAB)
                assert L.dgrep_stream_open(h, w, flags, ctypes.byref(s)) == dgrep.DGREP_E_NO_DFA, w
                assert s.value is None
    finally:
        L.dgrep_close(h)


def test_stream_calls_refuse_null():
    L = dgrep.lib()
    data = ctypes.create_string_buffer(b"x\n", 2)
    r = _dirty(dgrep._StreamResult)
    assert L.dgrep_stream_feed(None, data, 2, ctypes.byref(r)) == dgrep.DGREP_E_INVALID
    assert _zeroed(r)
    r = _dirty(dgrep._StreamResult)
    assert L.dgrep_stream_finish(None, ctypes.byref(r)) == dgrep.DGREP_E_INVALID
    assert _zeroed(r)
    assert L.dgrep_stream_feed(None, data, 2, None) == dgrep.DGREP_E_INVALID
    assert L.dgrep_stream_finish(None, None) == dgrep.DGREP_E_INVALID
    w = ctypes.c_uint64(7)
    assert L.dgrep_stream_stats(None, ctypes.byref(w), None, None, None) == dgrep.DGREP_E_INVALID
    assert w.value == 7


def test_free_and_close_accept_null_and_zeroed():
    L = dgrep.lib()
    L.dgrep_stream_close(None)
    L.dgrep_stream_result_free(None)
    r = dgrep._StreamResult()
    L.dgrep_stream_result_free(ctypes.byref(r))
    L.dgrep_stream_result_free(ctypes.byref(r))
    assert _zeroed(r)


def test_python_surface():
    assert callable(dgrep.MapStream) and callable(dgrep.Context.scan_windowed) and callable(dgrep.Context.stream)
    for m in ("feed", "finish", "stats", "close"):
        assert callable(getattr(dgrep.Stream, m))
