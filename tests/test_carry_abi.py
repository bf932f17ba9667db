"""The bounded windowed scan's C ABI on a machine without a GPU (include/dgrep.h,
DGREP_STREAM_BOUNDED / dgrep_scan_bounded / dgrep_stream_carry_stats): the
symbols are declared, exported and listed; every argument check returns its
status with the result zeroed, before any GPU call."""
import ctypes
import os

import dgrep
from test_abi import ROOT, _cpu_ctx, _declared
from test_window_abi import BAD_WINDOWS, GOOD_WINDOWS, _dirty, _zeroed

NEW = ("dgrep_scan_bounded", "dgrep_stream_carry_stats")


def test_symbols_declared_exported_and_listed():
    L = dgrep.lib()
    declared = _declared()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in dgrep.EXPORTS, name
    assert dgrep.STREAM_BOUNDED == 2 and dgrep.STREAM_VALUES == 1
    with open(os.path.join(ROOT, "include", "dgrep.h")) as f:
        assert "DGREP_STREAM_BOUNDED = 1u << 1" in f.read()


def test_null_arguments():
    L = dgrep.lib()
    data = ctypes.create_string_buffer(b"an error\n", 9)
    r = _dirty(dgrep._Result)
    assert L.dgrep_scan_bounded(None, data, 9, 4096, ctypes.byref(r)) == dgrep.DGREP_E_INVALID
    assert _zeroed(r)
    assert L.dgrep_scan_bounded(None, data, 9, 4096, None) == dgrep.DGREP_E_INVALID
    f = ctypes.c_uint64(7)
    ms = ctypes.c_float(3.0)
    assert L.dgrep_stream_carry_stats(None, ctypes.byref(f), None, None, None, ctypes.byref(ms)) == \
        dgrep.DGREP_E_INVALID
    assert f.value == 7 and ms.value == 3.0
    assert L.dgrep_stream_carry_stats(None, None, None, None, None, None) == dgrep.DGREP_E_INVALID


def test_scan_bounded_argument_checks():
    """dgrep_scan_windowed's checks, in its order"""
    L, h = _cpu_ctx()
    try:
        data = ctypes.create_string_buffer(b"an error\n", 9)
        assert L.dgrep_scan_bounded(h, data, 9, 4096, None) == dgrep.DGREP_E_INVALID
        r = _dirty(dgrep._Result)
        assert L.dgrep_scan_bounded(h, None, 9, 4096, ctypes.byref(r)) == dgrep.DGREP_E_INVALID  # n without data
        assert _zeroed(r)
        for w in BAD_WINDOWS:
            r = _dirty(dgrep._Result)
            assert L.dgrep_scan_bounded(h, data, 9, w, ctypes.byref(r)) == dgrep.DGREP_E_INVALID, w
            assert _zeroed(r), w
            assert b"4096" in L.dgrep_last_error(h)
        for w in GOOD_WINDOWS:
            for ptr, n in ((data, 9), (None, 0)):
                r = _dirty(dgrep._Result)
                assert L.dgrep_scan_bounded(h, ptr, n, w, ctypes.byref(r)) == dgrep.DGREP_E_NO_DFA, w
                assert _zeroed(r), w
    finally:
        L.dgrep_close(h)


def test_stream_open_bounded_flag_checks():
    """bounded with values is refused whatever else holds, with a message; no stream is made"""
    L, h = _cpu_ctx()
    try:
        both = dgrep.STREAM_BOUNDED | dgrep.STREAM_VALUES
        for w in GOOD_WINDOWS + BAD_WINDOWS:
            s = ctypes.c_void_p(0xABAB)
            assert L.dgrep_stream_open(h, w, both, ctypes.byref(s)) == dgrep.DGREP_E_INVALID, w
            assert s.value is None
        assert b"VALUES" in L.dgrep_last_error(h)
        for flags in (4, 6, 0x80000002):  # unknown bits beside the new one
            s = ctypes.c_void_p(0xABAB)
            assert L.dgrep_stream_open(h, 4096, flags, ctypes.byref(s)) == dgrep.DGREP_E_INVALID, flags
            assert s.value is None
    finally:
        L.dgrep_close(h)


def test_python_surface():
    import inspect

    assert "bounded" in inspect.signature(dgrep.Context.scan_windowed).parameters
    assert "bounded" in inspect.signature(dgrep.Context.stream).parameters
    assert inspect.signature(dgrep.Context.stream).parameters["bounded"].default is False
    assert callable(dgrep.Stream.carry_stats)
    assert "bounded" not in inspect.signature(dgrep.MapStream).parameters  # MapStream needs the values
