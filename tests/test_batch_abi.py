"""The batch entry points' C ABI, without a GPU: declared in include/dgrep.h,
exported by libdgrep.so and listed in dgrep.EXPORTS; every argument check is
DGREP_E_INVALID before any GPU call (on the context dgrep_open hands back on a
machine with no GPU), with the result struct zeroed."""
import ctypes

import numpy as np

import dgrep
import test_abi

NEW = ("dgrep_scan_batch", "dgrep_batch_result_free", "dgrep_scan_batch_device", "dgrep_last_batch_ms")


def test_batch_symbols_declared_exported_and_listed():
    L = dgrep.lib()
    declared = test_abi._declared()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in dgrep.EXPORTS, name
    # the C layout: 3 u64 pointers + count, the u32 pointer, nsplits, split_begin
    assert ctypes.sizeof(dgrep._BatchResult) == 56
    assert ctypes.sizeof(dgrep._ScanStats) == 80  # nothing appended for the batch


def _dirty():
    res = dgrep._BatchResult()
    ctypes.memset(ctypes.byref(res), 0xAB, ctypes.sizeof(res))
    return res


def _zeroed(res):
    return bytes(ctypes.string_at(ctypes.byref(res), ctypes.sizeof(res))) == bytes(ctypes.sizeof(res))


def test_scan_batch_argument_checks():
    L, h = test_abi._cpu_ctx()
    try:
        a = np.frombuffer(b"an error\n", np.uint8)
        ptrs = (ctypes.c_void_p * 2)(a.ctypes.data, a.ctypes.data)
        lens = (ctypes.c_size_t * 2)(len(a), len(a))
        INV = dgrep.DGREP_E_INVALID
        res = _dirty()
        assert L.dgrep_scan_batch(None, ptrs, lens, 2, ctypes.byref(res)) == INV and _zeroed(res)
        assert L.dgrep_scan_batch(h, ptrs, lens, 2, None) == INV
        for args in ((None, lens, 2), (ptrs, None, 2), (ptrs, lens, 0), (ptrs, lens, (1 << 32) - 1 + 1),
                     (ptrs, lens, 1 << 40)):
            res = _dirty()
            assert L.dgrep_scan_batch(h, args[0], args[1], args[2], ctypes.byref(res)) == INV, args[2]
            assert _zeroed(res)
        # a null data[i] is fine for an empty split only
        null1 = (ctypes.c_void_p * 2)(a.ctypes.data, None)
        res = _dirty()
        assert L.dgrep_scan_batch(h, null1, lens, 2, ctypes.byref(res)) == INV and _zeroed(res)
        # lengths whose sum overflows
        huge = (ctypes.c_size_t * 2)((1 << 64) - 2, 5)
        res = _dirty()
        assert L.dgrep_scan_batch(h, ptrs, huge, 2, ctypes.byref(res)) == INV and _zeroed(res)
        # well-formed arguments get past the checks: no DFA is loaded on this context
        ok0 = (ctypes.c_size_t * 2)(len(a), 0)
        res = _dirty()
        assert L.dgrep_scan_batch(h, null1, ok0, 2, ctypes.byref(res)) == dgrep.DGREP_E_NO_DFA and _zeroed(res)
        L.dgrep_batch_result_free(ctypes.byref(res))  # a zeroed result frees cleanly
        L.dgrep_batch_result_free(None)
    finally:
        L.dgrep_close(h)


def test_scan_batch_device_argument_checks():
    L, h = test_abi._cpu_ctx()
    try:
        INV = dgrep.DGREP_E_INVALID
        lens = (ctypes.c_uint64 * 3)(10, 0, 5)
        fake = ctypes.c_void_p(4096)  # never dereferenced: every call below fails its checks first
        cnt = ctypes.c_uint64(77)

        def call(ctx, d, n_packed, sl, k, count=ctypes.byref(cnt), cap=0):
            return L.dgrep_scan_batch_device(ctx, d, n_packed, sl, k, None, None, None, None, None, cap, count)

        assert call(None, fake, 17, lens, 3) == INV
        assert call(h, fake, 17, lens, 3, count=None) == INV
        assert call(h, fake, 17, None, 3) == INV
        assert call(h, fake, 17, lens, 0) == INV
        assert call(h, fake, 17, lens, 1 << 32) == INV
        assert call(h, None, 17, lens, 3) == INV
        for wrong in (16, 18, 15, 0):          # sum(split_len) + nsplits - 1 == 17
            cnt.value = 77
            assert call(h, fake, wrong, lens, 3) == INV and cnt.value == 0, wrong
        over = (ctypes.c_uint64 * 2)((1 << 64) - 1, 1)
        assert call(h, fake, 1, over, 2) == INV
        over = (ctypes.c_uint64 * 2)((1 << 64) - 2, 0)   # the sum fits, the closing begin[k] would not
        assert call(h, fake, (1 << 64) - 1, over, 2) == INV
        assert call(h, fake, 17, lens, 3, cap=4) == INV  # capacity without result arrays
        assert call(h, fake, 17, lens, 3) == dgrep.DGREP_E_NO_DFA
        a, b = ctypes.c_float(-1), ctypes.c_float(-1)
        assert L.dgrep_last_batch_ms(None, ctypes.byref(a), ctypes.byref(b)) == INV
        assert L.dgrep_last_batch_ms(h, None, ctypes.byref(b)) == INV
        assert L.dgrep_last_batch_ms(h, ctypes.byref(a), ctypes.byref(b)) == dgrep.DGREP_OK
        assert (a.value, b.value) == (0.0, 0.0)
    finally:
        L.dgrep_close(h)


def test_map_batch_of_nothing_touches_no_gpu():
    assert dgrep.MapBatch([]) == []
    assert dgrep.MapBatch(iter(())) == []
