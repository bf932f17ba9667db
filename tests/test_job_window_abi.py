"""The windowed whole job's C ABI on a machine without a GPU (include/dgrep.h,
dgrep_job_* / dgrep_grep_job_windowed): the symbols are declared, exported and
listed; every argument check that is decided before a GPU call returns its
status with the result zeroed; well-formed arguments reach DGREP_E_NO_DFA; the
sized stats getter refuses a null job and a zero size. The checks that need an
open job -- feed or end without begin, add inside a file, a call after finish,
a load mid-job, the stats getter's sizes -- need a loaded pattern, so a GPU:
test_gpu_job_window.py makes them."""
import ctypes

import dgrep
from test_abi import _cpu_ctx, _declared
from test_window_abi import BAD_WINDOWS, GOOD_WINDOWS, _dirty, _zeroed

NEW = ("dgrep_job_open", "dgrep_job_add", "dgrep_job_file_begin", "dgrep_job_file_feed", "dgrep_job_file_end",
       "dgrep_job_finish", "dgrep_job_close", "dgrep_job_stats_get", "dgrep_grep_job_windowed")


def test_symbols_declared_exported_and_listed():
    L = dgrep.lib()
    declared = _declared()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in dgrep.EXPORTS, name


def test_the_stats_struct_mirrors_the_header():
    assert ctypes.sizeof(dgrep._JobStats) == 12 * 8 + 4 * 4
    assert [f for f, _ in dgrep._JobStats._fields_] == [
        "files", "packs", "files_packed", "files_windowed", "windows", "rows", "segments", "arena_bytes",
        "arena_device_bytes", "window_device_bytes", "long_values", "arena_growths", "scan_ms", "encode_ms",
        "append_ms", "reduce_ms"]
    assert ctypes.sizeof(dgrep._ReduceBatchOut) == 40


def test_job_open_argument_checks():
    L, h = _cpu_ctx()
    try:
        j = ctypes.c_void_p(0xABAB)
        assert L.dgrep_job_open(None, 4096, 10, ctypes.byref(j)) == dgrep.DGREP_E_INVALID
        assert j.value is None
        assert L.dgrep_job_open(h, 4096, 10, None) == dgrep.DGREP_E_INVALID
        for w in BAD_WINDOWS:
            j = ctypes.c_void_p(0xABAB)
            assert L.dgrep_job_open(h, w, 10, ctypes.byref(j)) == dgrep.DGREP_E_INVALID, w
            assert j.value is None and b"4096" in L.dgrep_last_error(h)
        for nreduce in (0, 65536, 1 << 20, 0xFFFFFFFF):
            j = ctypes.c_void_p(0xABAB)
            assert L.dgrep_job_open(h, 4096, nreduce, ctypes.byref(j)) == dgrep.DGREP_E_INVALID, nreduce
            assert j.value is None and b"nreduce" in L.dgrep_last_error(h)
        for w in GOOD_WINDOWS:
            for nreduce in (1, 10, 65535):
                j = ctypes.c_void_p(0xABAB)
                assert L.dgrep_job_open(h, w, nreduce, ctypes.byref(j)) == dgrep.DGREP_E_NO_DFA, (w, nreduce)
                assert j.value is None
    finally:
        L.dgrep_close(h)


def test_one_shot_argument_checks():
    L, h = _cpu_ctx()
    try:
        raw = ctypes.create_string_buffer(b"an error\n", 9)
        data = (ctypes.c_void_p * 2)(ctypes.addressof(raw), ctypes.addressof(raw))
        n = (ctypes.c_size_t * 2)(9, 9)
        names = (ctypes.c_char_p * 2)(b"a", b"b")
        fn = (ctypes.c_size_t * 2)(1, 1)

        def call(ctx, d, nn, f, ff, k, nreduce, w, want):
            r = _dirty(dgrep._ReduceBatchOut)
            assert L.dgrep_grep_job_windowed(ctx, d, nn, f, ff, k, nreduce, w, ctypes.byref(r)) == want, (k, nreduce, w)
            assert _zeroed(r), (k, nreduce, w)

        call(None, data, n, names, fn, 2, 10, 4096, dgrep.DGREP_E_INVALID)
        assert L.dgrep_grep_job_windowed(h, data, n, names, fn, 2, 10, 4096, None) == dgrep.DGREP_E_INVALID
        call(h, None, n, names, fn, 2, 10, 4096, dgrep.DGREP_E_INVALID)
        call(h, data, None, names, fn, 2, 10, 4096, dgrep.DGREP_E_INVALID)
        call(h, data, n, None, fn, 2, 10, 4096, dgrep.DGREP_E_INVALID)
        call(h, data, n, names, None, 2, 10, 4096, dgrep.DGREP_E_INVALID)
        call(h, (ctypes.c_void_p * 2)(ctypes.addressof(raw), None), n, names, fn, 2, 10, 4096,
             dgrep.DGREP_E_INVALID)  # n without data
        call(h, data, n, (ctypes.c_char_p * 2)(b"a", None), fn, 2, 10, 4096, dgrep.DGREP_E_INVALID)  # fn without filename
        for w in BAD_WINDOWS:
            call(h, data, n, names, fn, 2, 10, w, dgrep.DGREP_E_INVALID)
            assert b"4096" in L.dgrep_last_error(h)
        for nreduce in (0, 65536, 0xFFFFFFFF):
            call(h, data, n, names, fn, 2, nreduce, 4096, dgrep.DGREP_E_INVALID)
            assert b"nreduce" in L.dgrep_last_error(h)
        for w in GOOD_WINDOWS:
            call(h, data, n, names, fn, 2, 10, w, dgrep.DGREP_E_NO_DFA)
            call(h, None, None, None, None, 0, 65535, w, dgrep.DGREP_E_NO_DFA)  # a job with no file
    finally:
        L.dgrep_close(h)


def test_job_calls_refuse_null():
    L = dgrep.lib()
    data = ctypes.create_string_buffer(b"x\n", 2)
    assert L.dgrep_job_add(None, data, 2, b"f", 1) == dgrep.DGREP_E_INVALID
    assert L.dgrep_job_file_begin(None, b"f", 1) == dgrep.DGREP_E_INVALID
    assert L.dgrep_job_file_feed(None, data, 2) == dgrep.DGREP_E_INVALID
    assert L.dgrep_job_file_end(None) == dgrep.DGREP_E_INVALID
    r = _dirty(dgrep._ReduceBatchOut)
    assert L.dgrep_job_finish(None, ctypes.byref(r)) == dgrep.DGREP_E_INVALID
    assert _zeroed(r)
    assert L.dgrep_job_finish(None, None) == dgrep.DGREP_E_INVALID
    st = _dirty(dgrep._JobStats)
    before = bytes(st)
    assert L.dgrep_job_stats_get(None, ctypes.byref(st), ctypes.sizeof(st)) == dgrep.DGREP_E_INVALID
    assert bytes(st) == before  # nothing written
    L.dgrep_job_close(None)  # safe


def test_python_surface():
    assert callable(dgrep.GrepJobWindowed) and callable(dgrep.Context.grep_job_windowed)
    assert callable(dgrep.Context.job)
    for m in ("add", "begin", "feed", "end", "finish", "stats", "close", "__enter__", "__exit__"):
        assert callable(getattr(dgrep.Job, m))
    assert dgrep.GrepJobWindowed([], 3) == []  # no file: no C call, no GPU
