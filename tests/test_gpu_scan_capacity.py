"""The capacity contract of the device forms (include/dgrep.h, dgrep_scan_device)
on every stepper and every pass of scan_resident, the host form's re-scan at
the true count, the alignment refusal and dgrep_set_stream -- bit-exact against
the oracle (capacity_cases.case / batch_cases.expected).

Every result array is capacity + 64 entries of a sentinel, so a store past
`capacity`, or past the count on a full call, shows. Every test opens its own
context: what a call does depends on the buffers earlier calls grew (the
staging buffer is sized by the largest capacity seen, the host form's first
guess by the largest result), and the session context has grown them all."""
import contextlib

import numpy as np
import pytest

import batch_cases as B
import capacity_cases as K
import oracle_lib as O
from test_gpu_encode import expected_partitions

pytestmark = pytest.mark.gpu

SENT = -7
SENT64, SENT32 = np.uint64(2**64 - 7), np.uint32(2**32 - 7)
GUARD = 64
NAMES = ("line_no", "start", "len")
_compiled = {}


@pytest.fixture(autouse=True)
def _torch_first(gpu_ctx):
    """The session context is opened (and never used) before anything here
    loads libdgrep: torch initialises the GPU first, as for every other GPU
    test, and without a GPU these tests skip like them."""


@contextlib.contextmanager
def _fresh(cfg=None):
    import dgrep

    ctx = dgrep.Context(0)
    try:
        if cfg is not None:
            ctx.set_stepper(cfg.force, cfg.rows)
            if cfg.name not in _compiled:  # the partial blob of [ab]*a[ab]{21} takes seconds to compile
                _compiled[cfg.name] = dgrep.CompiledPattern(cfg.pattern, state_budget=cfg.budget)
            cp = ctx.load(_compiled[cfg.name])
            assert cp.partial == cfg.name.startswith("partial"), (cfg.name, cp.flags)
        yield ctx
    finally:
        ctx.close()


def _upload(data, pad=0):
    import torch

    t = torch.frombuffer(bytearray(data) + bytearray(pad) or bytearray(1), dtype=torch.uint8).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _arrays(cap, dtypes):
    import torch

    out = [torch.full((cap + GUARD,), SENT, dtype=dt, device="cuda") for dt in dtypes]
    torch.cuda.synchronize()
    return out


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint64 if a.dtype == np.int64 else np.uint32)


def _scan_device(ctx, ptr, n, cap):
    """dgrep_scan_device into sentinel-filled arrays of cap + GUARD entries: (count, host copies)."""
    import torch

    outs = _arrays(cap, [torch.int64] * 3)
    count = ctx.scan_device(ptr, n, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), cap)
    return count, [_host(o) for o in outs]


def _assert_contract(ctx, count, got, cap, want, what):
    """What dgrep.h promises after a call with `cap`: the exact count, nothing
    at or past cap, and on a full call the records and nothing past them."""
    total = len(want[0])
    assert count == total, (what, cap, count, total)
    assert ctx.scan_stats()["matches"] == total, (what, cap)
    for name, a, w in zip(NAMES, got, want):
        assert (a[cap:] == SENT64).all(), "%s cap %d: %s written at or past capacity" % (what, cap, name)
        if cap >= total:
            np.testing.assert_array_equal(a[:total], w, err_msg="%s cap %d %s" % (what, cap, name))
            assert (a[total:cap] == SENT64).all(), "%s cap %d: %s written past the count" % (what, cap, name)


def _assert_untouched(got, what):
    for a in got:
        assert (a == (SENT64 if a.dtype == np.uint64 else SENT32)).all(), what


# ---- 1. the capacity matrix ----------------------------------------------------
CASES = [(cfg, shape) for cfg in K.CONFIGS for shape in K.SHAPES]


@pytest.mark.parametrize("cfg,shape", CASES, ids=["%s-%s" % (c.name, s) for c, s in CASES])
def test_capacity_matrix(cfg, shape):
    data, want = K.case(cfg, shape)
    total = len(want[0])
    buf = _upload(data)
    with _fresh(cfg) as ctx:
        ctx.set_lane_chunk(K.lane_chunk(cfg, shape))
        for i, cap in enumerate(K.capacities(total)):
            what = "%s %s call %d" % (cfg.name, shape, i)
            count, got = _scan_device(ctx, buf.data_ptr(), len(data), cap)
            _assert_contract(ctx, count, got, cap, want, what)
            st = ctx.scan_stats()
            assert st["stepper"] == cfg.stepper, (what, st)
            # the pass the shape is for ran, whatever the capacity
            if shape in ("dense", "dense_long"):
                assert st["overflow_lanes"] > 0, (what, st)
            if shape in ("parked", "dense_long") and cfg.parks:
                assert st["pending"] > 0, (what, st)
            if i == 0 and shape == "parked" and cfg.stepper == "filter":
                # a new context's staging holds one line: the candidates outgrow it and the scan runs again
                assert st["scan_attempts"] >= 2, (what, st)


# ---- 2. the empty split and a pattern that matches nothing ---------------------
@pytest.mark.parametrize("pattern,budget,matches", [(b"", 0, True), (b"^$", 0, True), (b"x*$", 0, True),
                                                    (b"^$", 3, True), (b"error", 0, False), (K.C3, 0, False),
                                                    (b"error", 3, False)])
def test_empty_split(pattern, budget, matches):
    """n == 0 is the one empty line; d_data is not read: NULL and unaligned pointers are accepted."""
    import dgrep

    buf = _upload(b"0123456789abcdef" * 2)
    want = tuple(np.array([v] if matches else [], np.uint64) for v in (1, 0, 0))
    assert len(O.grep_map(pattern, b"")[0]) == int(matches)
    with _fresh() as ctx:
        ctx.load(dgrep.CompiledPattern(pattern, state_budget=budget))
        for ptr in (0, buf.data_ptr(), buf.data_ptr() + 1, buf.data_ptr() + 15):
            for cap in (0, 1, 2, 0, 1):
                count, got = _scan_device(ctx, ptr, 0, cap)
                _assert_contract(ctx, count, got, cap, want, "%r n=0 ptr%%16=%d" % (pattern, ptr % 16))
                if cap == 0 or not matches:
                    _assert_untouched(got, (pattern, cap))


def test_match_none_pattern_touches_nothing():
    import dgrep

    cfg = K.CONFIGS[0]
    data, _ = K.case(cfg, "plain")
    buf = _upload(data)
    with _fresh() as ctx:
        cp = ctx.load(b"a**")
        assert cp.flags & dgrep.DFA_MATCH_NONE
        for n in (len(data), 0):
            for cap in (0, 5):
                count, got = _scan_device(ctx, buf.data_ptr(), n, cap)
                assert count == 0 and ctx.scan_stats()["matches"] == 0
                _assert_untouched(got, ("a**", n, cap))
        # and the context scans on with the next pattern
        ctx.load(cfg.pattern)
        want = K.case(cfg, "plain")[1]
        count, got = _scan_device(ctx, buf.data_ptr(), len(data), len(want[0]))
        _assert_contract(ctx, count, got, len(want[0]), want, "after a**")


# ---- 3. the host form's re-scan at the true count -------------------------------
# scan_stats describes the last scan only, so it cannot show that scan_host ran
# twice. The inputs follow from scan_host's formula instead: a new context's
# first guess is max(1024, n / 512) records, and each split marked "retry" below
# holds more matching lines than that, so only the second scan, into arrays
# grown to the true count, can return them all.
def _first_guess(n):
    return max(1024, n // 512)


def _assert_scan(ctx, pattern, data, what, retry):
    want = O.grep_map(pattern, data)
    assert (len(want[0]) > _first_guess(len(data))) == retry, (what, len(want[0]), _first_guess(len(data)))
    got = ctx.scan(data)
    for name, g, w in zip(NAMES, got, want):
        assert len(g) == len(w), (what, name, len(g), len(w))
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (what, name))
    assert ctx.scan_stats()["matches"] == len(want[0])


def test_host_retry_dense():
    with _fresh() as ctx:
        ctx.load(b"")
        _assert_scan(ctx, b"", b"x\n" * 5000, "5,000 one-byte lines", True)
    sheng = K.CONFIGS[0]
    with _fresh(sheng) as ctx:
        _assert_scan(ctx, sheng.pattern, K.case(sheng, "dense")[0], "dense", True)
        assert ctx.scan_stats()["overflow_lanes"] > 0
        # fewer matches into the grown arrays, then the retry's split again
        _assert_scan(ctx, sheng.pattern, K.case(sheng, "plain")[0], "plain after dense", False)
        _assert_scan(ctx, sheng.pattern, K.case(sheng, "parked")[0], "parked after dense", False)
        assert ctx.scan_stats()["pending"] > 0


def test_host_retry_on_the_filter():
    """Forced 4-row filter: the first scan outgrows a new context's staging (a
    re-scan inside scan_resident), its count outgrows the first guess (the
    re-scan of scan_host), and that scan's staging holds the first one's lines."""
    cfg = K.CONFIGS[3]
    assert cfg.name == "filter4"
    with _fresh(cfg) as ctx:
        _assert_scan(ctx, cfg.pattern, K.case(cfg, "dense")[0], "filter4 dense", True)
        assert ctx.scan_stats()["stepper"] == "filter"
        _assert_scan(ctx, cfg.pattern, K.case(cfg, "parked")[0], "filter4 parked after dense", False)
        assert ctx.scan_stats()["pending"] > 0
        _assert_scan(ctx, cfg.pattern, K.case(cfg, "plain")[0], "filter4 plain after dense", False)


def _around_long_line(matching, long_matches):
    """`matching` short matching lines with one 100,000-byte line in their middle."""
    short = [b"x error %d" % i for i in range(matching)]
    long_line = b"q" * 100000 + (b" error" if long_matches else b"")
    return b"\n".join(short[:matching // 2] + [long_line] + short[matching // 2:])


@pytest.mark.parametrize("force,pattern", [("auto", b"error"), ("table", b"error"), ("filter", b"error")])
def test_host_retry_with_a_parked_line(force, pattern):
    """A parked line is staged as one record whether it matches or not, so a
    non-matching one makes the staged lines one more than the count: the arrays
    of the second scan (exactly the count) and, with 1,024 matching lines, of
    the first guess hold every record but not every staged line."""
    for matching, long_matches, retry in ((3000, False, True), (3000, True, True), (1024, False, False),
                                          (1023, True, False), (1025, False, True)):
        with _fresh() as ctx:
            ctx.set_stepper(force, 4 if force == "filter" else 0)
            ctx.load(pattern)
            what = "%s %d lines, long line %s" % (force, matching, "matches" if long_matches else "does not match")
            _assert_scan(ctx, pattern, _around_long_line(matching, long_matches), what, retry)
            assert ctx.scan_stats()["pending"] == 1, (what, ctx.scan_stats())
            _assert_scan(ctx, pattern, _around_long_line(40, not long_matches), what + ", then fewer", False)


def test_host_retry_batch():
    splits = [b"error", b"x\nan error\n", b"", b"no"] * 800 + B.FIXED_SPLITS + [_around_long_line(200, False)]
    total = sum(map(len, splits)) + len(splits) - 1
    with _fresh() as ctx:
        ctx.load(b"error")
        want = B.expected(b"error", splits)
        assert len(want[0]) > _first_guess(total)  # batch_scan_host makes the same first guess from the packed size
        B.assert_same(ctx.scan_batch(splits), want, "batch retry")
        assert ctx.scan_stats()["matches"] == len(want[0]) and ctx.scan_stats()["pending"] >= 1
        fewer = B.FIXED_SPLITS + B.random_splits(3, 50)
        B.assert_same(ctx.scan_batch(fewer), B.expected(b"error", fewer), "fewer after the batch retry")
        B.assert_same(ctx.scan_batch(splits), want, "the batch again")


# ---- 4. alignment ----------------------------------------------------------------
def _batch_device(ctx, ptr, splits, cap):
    import torch

    k = len(splits)
    outs = _arrays(cap, [torch.int64, torch.int64, torch.int64, torch.int32])
    sb = torch.full((k + 1,), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    count = ctx.scan_batch_device(ptr, sum(map(len, splits)) + k - 1, [len(s) for s in splits], outs[0].data_ptr(),
                                  outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), sb.data_ptr(), cap)
    return count, [_host(o) for o in outs] + [_host(sb)]


def test_unaligned_device_split_is_refused():
    import torch

    import dgrep

    cfg = K.CONFIGS[0]
    data, want = K.case(cfg, "plain")
    total = len(want[0])
    splits = data.split(b"\n", 3)  # the same bytes as a packed buffer of four splits
    want_batch = B.expected(cfg.pattern, splits)
    base = _upload(b"\0" * 16 + data, pad=16)
    with _fresh(cfg) as ctx:
        for off in range(1, 16):
            shifted = base[off:off + len(data)]  # len(data) readable bytes, `off` past an aligned address
            assert shifted.data_ptr() % 16 == off
            outs = _arrays(total, [torch.int64] * 3)
            with pytest.raises(dgrep.DgrepError) as ei:
                ctx.scan_device(shifted.data_ptr(), len(data), outs[0].data_ptr(), outs[1].data_ptr(),
                                outs[2].data_ptr(), total)
            assert ei.value.code == dgrep.DGREP_E_INVALID and "16-byte aligned" in str(ei.value), str(ei.value)
            _assert_untouched([_host(o) for o in outs], ("scan_device", off))
            outs = _arrays(total, [torch.int64, torch.int64, torch.int64, torch.int32, torch.int64])
            with pytest.raises(dgrep.DgrepError) as ei:
                ctx.scan_batch_device(shifted.data_ptr(), len(data), [len(s) for s in splits], outs[0].data_ptr(),
                                      outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr(),
                                      total)
            assert ei.value.code == dgrep.DGREP_E_INVALID and "16-byte aligned" in str(ei.value), str(ei.value)
            _assert_untouched([_host(o) for o in outs], ("scan_batch_device", off))
        # the aligned calls that follow are exact
        aligned = base[16:16 + len(data)]
        count, got = _scan_device(ctx, aligned.data_ptr(), len(data), total)
        _assert_contract(ctx, count, got, total, want, "aligned after the refusals")
        count, got = _batch_device(ctx, aligned.data_ptr(), splits, total)
        assert count == total
        B.assert_same([a[:total] for a in got[:4]] + [got[4][:len(splits) + 1]], want_batch, "aligned batch")
        # n_packed == 0 (one empty split): the pointer is not read
        ctx.load(b"")
        for ptr in (0, base.data_ptr() + 3):
            count, got = _batch_device(ctx, ptr, [b""], 1)
            assert count == 1
            B.assert_same([a[:1] for a in got[:4]] + [got[4][:2]], B.expected(b"", [b""]), "empty packed buffer")


# ---- 5. dgrep_set_stream -----------------------------------------------------------
def test_set_stream_orders_the_scan_behind_the_callers_work():
    """The split is filled and patched on a torch stream and scanned, batch
    scanned and encoded with no host synchronisation between: the results are
    those of the final bytes only if the library's work runs on that stream."""
    import torch

    cfg = K.CONFIGS[0]
    first = bytearray(K.case(cfg, "plain")[0])
    n = len(first)
    cut = 150001                      # three '\n' written here: first[cut + 1] separates two splits
    final = bytearray(first)
    final[cut:cut + 3] = b"\n\n\n"
    final[20000:20005] = b"error"
    final[299000:299005] = b"error"
    final = bytes(final)
    splits = [final[:cut + 1], final[cut + 2:]]
    assert B.pack(splits) == final
    want = O.grep_map(cfg.pattern, final)
    total = len(want[0])
    assert [w.tolist() for w in want] != [w.tolist() for w in K.case(cfg, "plain")[1]]  # the patches change the result
    want_batch = B.expected(cfg.pattern, splits)
    want_parts = expected_partitions(cfg.pattern, b"s.log", final, 7)

    pinned = torch.frombuffer(first, dtype=torch.uint8).pin_memory()
    word = torch.tensor(list(b"error"), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with _fresh(cfg) as ctx:
        try:
            ctx.set_stream(stream.cuda_stream)
            with torch.cuda.stream(stream):
                buf = torch.empty(n, dtype=torch.uint8, device="cuda")
                outs = [torch.full((total + GUARD,), SENT, dtype=dt, device="cuda")
                        for dt in [torch.int64] * 6 + [torch.int32, torch.int64]]
                enc = torch.zeros(sum(map(len, want_parts)) + GUARD, dtype=torch.uint8, device="cuda")
                buf.copy_(pinned, non_blocking=True)
                buf[cut:cut + 3].fill_(10)
                buf[20000:20005].copy_(word)
                buf[299000:299005].copy_(word)
                # no host synchronisation from here on
                count = ctx.scan_device(buf.data_ptr(), n, outs[0].data_ptr(), outs[1].data_ptr(),
                                        outs[2].data_ptr(), total)
                assert ctx.last_kernel_ms() > 0
                bcount = ctx.scan_batch_device(buf.data_ptr(), n, [len(s) for s in splits], outs[3].data_ptr(),
                                               outs[4].data_ptr(), outs[5].data_ptr(), outs[6].data_ptr(),
                                               outs[7].data_ptr(), total)
                assert ctx.last_kernel_ms() > 0
                begin, end, nbytes = ctx.encode_device(buf.data_ptr(), n, outs[0].data_ptr(), outs[1].data_ptr(),
                                                       outs[2].data_ptr(), count, b"s.log", 7, enc.data_ptr(),
                                                       enc.numel() - GUARD)
                got = [_host(o) for o in outs]
                raw = enc.cpu().numpy().tobytes()
            _assert_contract(ctx, count, got[:3], total, want, "scan_device on the caller's stream")
            assert bcount == total
            B.assert_same([a[:total] for a in got[3:7]] + [got[7][:3]], want_batch, "scan_batch_device on the stream")
            assert nbytes == sum(map(len, want_parts))
            assert [raw[b:e] for b, e in zip(begin, end)] == want_parts
        finally:
            ctx.set_stream(None)
        # the context's own stream again
        _assert_scan(ctx, cfg.pattern, final, "after set_stream(None)", False)
    del stream
