"""The batch partition writer's C ABI, without a GPU: declared in
include/dgrep.h, exported by libdgrep.so and listed in dgrep.EXPORTS; every
argument check is DGREP_E_INVALID before any GPU call (on the context dgrep_open
hands back on a machine with no GPU), with the result struct zeroed or *total
= 0; too many cells is DGREP_E_UNSUPPORTED; well-formed arguments reach
DGREP_E_NO_DFA in the host form."""
import ctypes

import numpy as np

import dgrep
import test_abi

NEW = ("dgrep_map_partitions_batch", "dgrep_batch_partitions_free", "dgrep_encode_batch_device")


def test_symbols_declared_exported_and_listed():
    L = dgrep.lib()
    declared = test_abi._declared()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in dgrep.EXPORTS, name
    # u64 nsplits, u32 nreduce (+ 4 padding), u64 total, two pointers
    assert ctypes.sizeof(dgrep._BatchPartitions) == 40
    assert ctypes.sizeof(dgrep._ScanStats) == 80  # nothing appended for the batch encode


def _dirty():
    res = dgrep._BatchPartitions()
    ctypes.memset(ctypes.byref(res), 0xAB, ctypes.sizeof(res))
    return res


def _zeroed(res):
    return bytes(ctypes.string_at(ctypes.byref(res), ctypes.sizeof(res))) == bytes(ctypes.sizeof(res))


def test_map_partitions_batch_argument_checks():
    L, h = test_abi._cpu_ctx()
    try:
        a = np.frombuffer(b"an error\n", np.uint8)
        ptrs = (ctypes.c_void_p * 2)(a.ctypes.data, a.ctypes.data)
        lens = (ctypes.c_size_t * 2)(len(a), len(a))
        names = (ctypes.c_char_p * 2)(b"a.log", b"b.log")
        fns = (ctypes.c_size_t * 2)(5, 5)
        INV = dgrep.DGREP_E_INVALID

        def call(ctx, data, n, fname, fn, k, nreduce, out="new"):
            res = _dirty()
            rc = L.dgrep_map_partitions_batch(ctx, data, n, fname, fn, k, nreduce,
                                              ctypes.byref(res) if out == "new" else out)
            return rc, res

        rc, res = call(None, ptrs, lens, names, fns, 2, 10)
        assert rc == INV and _zeroed(res)
        assert call(h, ptrs, lens, names, fns, 2, 10, out=None)[0] == INV
        bad = [
            (None, lens, names, fns, 2, 10),           # the checks of dgrep_scan_batch
            (ptrs, None, names, fns, 2, 10),
            (ptrs, lens, names, fns, 0, 10),
            (ptrs, lens, names, fns, 1 << 32, 10),
            (ptrs, lens, names, fns, 1 << 40, 10),
            ((ctypes.c_void_p * 2)(a.ctypes.data, None), lens, names, fns, 2, 10),  # null data[i], n[i] != 0
            (ptrs, (ctypes.c_size_t * 2)((1 << 64) - 2, 5), names, fns, 2, 10),     # the lengths overflow
            (ptrs, lens, None, fns, 2, 10),            # a null filename array
            (ptrs, lens, names, None, 2, 10),          # a null fn array
            (ptrs, lens, (ctypes.c_char_p * 2)(b"a.log", None), fns, 2, 10),        # null filename[i], fn[i] != 0
            (ptrs, lens, names, fns, 2, 0),            # nreduce outside 1..65535
            (ptrs, lens, names, fns, 2, 65536),
            (ptrs, lens, names, fns, 2, 0xFFFFFFFF),
        ]
        for args in bad:
            rc, res = call(h, *args)
            assert rc == INV and _zeroed(res), args[4:]
        # 70,000 splits x 65,535 partitions = 2^32 cells and more: refused by name, not by accident
        k = 70000
        many = (ctypes.c_void_p * k)()
        zero = (ctypes.c_size_t * k)()
        nonames = (ctypes.c_char_p * k)()
        rc, res = call(h, many, zero, nonames, zero, k, 65535)
        assert rc == dgrep.DGREP_E_UNSUPPORTED and _zeroed(res)
        assert b"2^32" in L.dgrep_last_error(h)
        k = 65537                                # 65537 * 65535 = 2^32 - 1: allowed; 65537 * 65536 is not a legal nreduce
        rc, res = call(h, many, zero, nonames, zero, k, 65535)
        assert rc == dgrep.DGREP_E_NO_DFA and _zeroed(res)
        # well-formed arguments get past the checks: no DFA is loaded on this context.
        # A null data[i] / filename[i] is fine for an empty split / name, nreduce 1 and 65535 are legal
        for nreduce in (1, 10, 65535):
            rc, res = call(h, (ctypes.c_void_p * 2)(a.ctypes.data, None), (ctypes.c_size_t * 2)(len(a), 0),
                           (ctypes.c_char_p * 2)(b"a.log", None), (ctypes.c_size_t * 2)(5, 0), 2, nreduce)
            assert rc == dgrep.DGREP_E_NO_DFA and _zeroed(res), nreduce
        L.dgrep_batch_partitions_free(ctypes.byref(res))  # a zeroed result frees cleanly
        L.dgrep_batch_partitions_free(None)
    finally:
        L.dgrep_close(h)


def test_encode_batch_device_argument_checks():
    L, h = test_abi._cpu_ctx()
    try:
        INV = dgrep.DGREP_E_INVALID
        lens = (ctypes.c_uint64 * 3)(10, 0, 5)       # sum + nsplits - 1 == 17
        names = (ctypes.c_char_p * 3)(b"a", b"", b"c.log")
        fns = (ctypes.c_size_t * 3)(1, 0, 5)
        fake = ctypes.c_void_p(4096)  # never dereferenced: every call below fails its checks first
        off = (ctypes.c_uint64 * (3 * 65535 + 1))()
        tot = ctypes.c_uint64(77)
        good = dict(ctx=h, d=fake, n_packed=17, sl=lens, k=3, recs=(fake, fake, fake, fake), count=4, fname=names,
                    fn=fns, nreduce=10, d_out=fake, out_cap=64, cell_off=off, total=ctypes.byref(tot))

        def call(**kw):
            a = dict(good, **kw)
            tot.value = 77
            return L.dgrep_encode_batch_device(a["ctx"], a["d"], a["n_packed"], a["sl"], a["k"], a["recs"][0],
                                               a["recs"][1], a["recs"][2], a["recs"][3], a["count"], a["fname"],
                                               a["fn"], a["nreduce"], a["d_out"], a["out_cap"], a["cell_off"],
                                               a["total"])

        assert call(ctx=None) == INV and tot.value == 0
        assert call(total=None) == INV
        bad = [dict(cell_off=None), dict(sl=None), dict(k=0), dict(k=1 << 32), dict(d=None),
               dict(fname=None), dict(fn=None),
               dict(fname=(ctypes.c_char_p * 3)(b"a", None, None)),   # null filename[2] with fn[2] = 5
               dict(nreduce=0), dict(nreduce=65536),
               dict(n_packed=16), dict(n_packed=18), dict(n_packed=0, d=None),   # lengths that do not add up
               dict(sl=(ctypes.c_uint64 * 3)((1 << 64) - 1, 1, 0)),              # ... or overflow
               dict(d_out=None),                                                  # out_cap without d_out
               ]
        for i in range(4):                                                        # count without a record array
            recs = [fake] * 4
            recs[i] = None
            bad.append(dict(recs=tuple(recs)))
        for kw in bad:
            assert call(**kw) == INV and tot.value == 0, sorted(kw)
        # the limits named by a message
        k = 70000
        assert call(k=k, sl=(ctypes.c_uint64 * k)(), n_packed=k - 1, fname=(ctypes.c_char_p * k)(),
                    fn=(ctypes.c_size_t * k)(), nreduce=65535) == dgrep.DGREP_E_UNSUPPORTED and tot.value == 0
        assert b"2^32" in L.dgrep_last_error(h)
        assert call(count=1 << 32) == dgrep.DGREP_E_UNSUPPORTED and tot.value == 0
        assert b"records" in L.dgrep_last_error(h)
    finally:
        L.dgrep_close(h)


def test_map_partitions_batch_of_nothing_makes_no_c_call():
    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("C call " + name)

    ctx = dgrep.Context.__new__(dgrep.Context)  # no device behind it: any use of the library would raise
    ctx._L, ctx._h = NoCalls(), ctypes.c_void_p()
    assert ctx.map_partitions_batch([], 10) == []
    assert ctx.map_partitions_batch(iter(()), 10) == []
