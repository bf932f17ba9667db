"""The batch reduce's and the job call's C ABI, without a GPU: declared in
include/dgrep.h, exported by libdgrep.so and listed in dgrep.EXPORTS; every
argument check returns its status before any GPU call (on the context dgrep_open
hands back on a machine with no GPU), with the result struct zeroed or *total =
0; the limits are DGREP_E_UNSUPPORTED with a message that names them;
well-formed arguments reach DGREP_E_NO_DFA in dgrep_grep_job."""
import ctypes

import numpy as np

import dgrep
import test_abi

NEW = ("dgrep_reduce_batch", "dgrep_reduce_batch_free", "dgrep_reduce_batch_device", "dgrep_grep_job",
       "dgrep_last_reduce_ms")
INV = dgrep.DGREP_E_INVALID
UNS = dgrep.DGREP_E_UNSUPPORTED


def test_symbols_declared_exported_and_listed():
    L = dgrep.lib()
    declared = test_abi._declared()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in dgrep.EXPORTS, name
    # u32 nparts (+ 4 padding), u64 total, three pointers
    assert ctypes.sizeof(dgrep._ReduceBatchOut) == 40
    assert ctypes.sizeof(dgrep._ScanStats) == 80  # nothing appended for the reduce


def _dirty():
    res = dgrep._ReduceBatchOut()
    ctypes.memset(ctypes.byref(res), 0xAB, ctypes.sizeof(res))
    return res


def _zeroed(res):
    return bytes(ctypes.string_at(ctypes.byref(res), ctypes.sizeof(res))) == bytes(ctypes.sizeof(res))


def test_reduce_batch_argument_checks():
    L, h = test_abi._cpu_ctx()
    try:
        a = np.frombuffer(b'{"Key":"a","Value":"b"}\n', np.uint8)
        ptrs = (ctypes.c_void_p * 2)(a.ctypes.data, a.ctypes.data)
        lens = (ctypes.c_size_t * 2)(len(a), len(a))

        def call(ctx, data, n, nparts, out="new"):
            res = _dirty()
            rc = L.dgrep_reduce_batch(ctx, data, n, nparts, ctypes.byref(res) if out == "new" else out)
            return rc, res

        rc, res = call(None, ptrs, lens, 2)
        assert rc == INV and _zeroed(res)
        assert call(h, ptrs, lens, 2, out=None)[0] == INV
        bad = [
            (None, lens, 2),
            (ptrs, None, 2),
            (ptrs, lens, 0),
            (ptrs, lens, 65536),
            (ptrs, lens, 1 << 40),
            ((ctypes.c_void_p * 2)(a.ctypes.data, None), lens, 2),           # null data[p], n[p] != 0
            (ptrs, (ctypes.c_size_t * 2)((1 << 64) - 2, 5), 2),              # the lengths overflow
        ]
        for args in bad:
            rc, res = call(h, *args)
            assert rc == INV and _zeroed(res), args[2]
        # all inputs empty: OK with nothing read, no GPU call (this context has no GPU)
        for nparts in (1, 3, 65535):
            rc, res = call(h, (ctypes.c_void_p * nparts)(), (ctypes.c_size_t * nparts)(), nparts)
            assert rc == dgrep.DGREP_OK and res.nparts == nparts and res.total == 0 and not res.bytes
            assert all(res.part_off[p] == 0 for p in (0, nparts // 2, nparts))
            assert all(res.lines_in[p] == 0 for p in (0, nparts // 2, nparts - 1))
            L.dgrep_reduce_batch_free(ctypes.byref(res))
            assert _zeroed(res)
        L.dgrep_reduce_batch_free(ctypes.byref(res))  # a zeroed result frees cleanly
        L.dgrep_reduce_batch_free(None)
        ms = ctypes.c_float(7)
        assert L.dgrep_last_reduce_ms(h, ctypes.byref(ms)) == dgrep.DGREP_OK and ms.value == 0
        assert L.dgrep_last_reduce_ms(None, ctypes.byref(ms)) == INV and L.dgrep_last_reduce_ms(h, None) == INV
    finally:
        L.dgrep_close(h)


def test_reduce_batch_device_argument_checks():
    L, h = test_abi._cpu_ctx()
    try:
        seg = (ctypes.c_uint64 * 7)(0, 10, 10, 25, 25, 25, 40)      # 6 segments, n = 40
        fake = ctypes.c_void_p(4096)  # never dereferenced: every call below fails its checks first
        off = (ctypes.c_uint64 * 65537)()
        lin = (ctypes.c_uint64 * 65536)()
        tot = ctypes.c_uint64(77)
        good = dict(ctx=h, d=fake, n=40, seg=seg, nseg=6, nparts=3, d_out=fake, out_cap=64, off=off, lin=lin,
                    total=ctypes.byref(tot))

        def call(**kw):
            a = dict(good, **kw)
            tot.value = 77
            return L.dgrep_reduce_batch_device(a["ctx"], a["d"], a["n"], a["seg"], a["nseg"], a["nparts"], a["d_out"],
                                               a["out_cap"], a["off"], a["lin"], a["total"])

        assert call(ctx=None) == INV and tot.value == 0
        assert call(total=None) == INV
        bad = [dict(off=None), dict(seg=None), dict(nseg=0), dict(nparts=0),
               dict(nparts=4), dict(nparts=5), dict(nseg=5),                      # nseg % nparts != 0
               dict(seg=(ctypes.c_uint64 * 7)(1, 10, 10, 25, 25, 25, 40)),        # seg_off[0] != 0
               dict(seg=(ctypes.c_uint64 * 7)(0, 10, 9, 25, 25, 25, 40)),         # descending
               dict(n=39), dict(n=41), dict(n=0, d=None),                         # seg_off[nseg] != n
               dict(d=None),                                                      # n without d_data
               dict(d_out=None),                                                  # out_cap without d_out
               dict(d=ctypes.c_void_p(4096 + 8)),                                 # d_data not 16-byte aligned
               ]
        for kw in bad:
            assert call(**kw) == INV and tot.value == 0, sorted(kw)
        # the limits, named by their message, before seg_off is read
        zeros = (ctypes.c_uint64 * 65537)()
        assert call(nparts=65536, nseg=65536, seg=zeros, n=0, d=None) == UNS and tot.value == 0
        assert b"65535" in L.dgrep_last_error(h) and b"nparts" in L.dgrep_last_error(h)
        assert call(nseg=1 << 32, nparts=1) == UNS and tot.value == 0
        assert b"2^32" in L.dgrep_last_error(h) and b"nseg" in L.dgrep_last_error(h)
        assert call(nseg=(1 << 32) + 3, nparts=1) == UNS and tot.value == 0
    finally:
        L.dgrep_close(h)


def test_grep_job_argument_checks():
    L, h = test_abi._cpu_ctx()
    try:
        a = np.frombuffer(b"an error\n", np.uint8)
        ptrs = (ctypes.c_void_p * 2)(a.ctypes.data, a.ctypes.data)
        lens = (ctypes.c_size_t * 2)(len(a), len(a))
        names = (ctypes.c_char_p * 2)(b"a.log", b"b.log")
        fns = (ctypes.c_size_t * 2)(5, 5)

        def call(ctx, data, n, fname, fn, k, nreduce, out="new"):
            res = _dirty()
            rc = L.dgrep_grep_job(ctx, data, n, fname, fn, k, nreduce, ctypes.byref(res) if out == "new" else out)
            return rc, res

        rc, res = call(None, ptrs, lens, names, fns, 2, 10)
        assert rc == INV and _zeroed(res)
        assert call(h, ptrs, lens, names, fns, 2, 10, out=None)[0] == INV
        bad = [
            (None, lens, names, fns, 2, 10),           # the checks of dgrep_map_partitions_batch
            (ptrs, None, names, fns, 2, 10),
            (ptrs, lens, names, fns, 0, 10),
            (ptrs, lens, names, fns, 1 << 32, 10),
            ((ctypes.c_void_p * 2)(a.ctypes.data, None), lens, names, fns, 2, 10),
            (ptrs, (ctypes.c_size_t * 2)((1 << 64) - 2, 5), names, fns, 2, 10),
            (ptrs, lens, None, fns, 2, 10),
            (ptrs, lens, names, None, 2, 10),
            (ptrs, lens, (ctypes.c_char_p * 2)(b"a.log", None), fns, 2, 10),
            (ptrs, lens, names, fns, 2, 0),
            (ptrs, lens, names, fns, 2, 65536),
        ]
        for args in bad:
            rc, res = call(h, *args)
            assert rc == INV and _zeroed(res), args[4:]
        k = 70000                                # 70,000 splits x 65,535 partitions: 2^32 cells and more
        many = (ctypes.c_void_p * k)()
        zero = (ctypes.c_size_t * k)()
        nonames = (ctypes.c_char_p * k)()
        rc, res = call(h, many, zero, nonames, zero, k, 65535)
        assert rc == UNS and _zeroed(res)
        assert b"2^32" in L.dgrep_last_error(h)
        # well-formed arguments get past the checks: no DFA is loaded on this context
        for nreduce in (1, 10, 65535):
            rc, res = call(h, ptrs, lens, names, fns, 2, nreduce)
            assert rc == dgrep.DGREP_E_NO_DFA and _zeroed(res), nreduce
        L.dgrep_reduce_batch_free(ctypes.byref(res))
    finally:
        L.dgrep_close(h)


def test_reduce_batch_and_grep_job_of_nothing_make_no_c_call():
    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("C call " + name)

    ctx = dgrep.Context.__new__(dgrep.Context)  # no device behind it: any use of the library would raise
    ctx._L, ctx._h = NoCalls(), ctypes.c_void_p()
    assert ctx.reduce_batch([]) == []
    assert ctx.reduce_batch(iter(())) == []
    assert ctx.grep_job([], 10) == []
    assert ctx.grep_job(iter(()), 10) == []
