"""Many splits in one scan (dgrep_scan_batch / dgrep_scan_batch_device /
MapBatch) on the GPU, bit-exact per split against the oracle's Map of that
split alone (batch_cases.expected: records, split ids and per-split ranges all
derived from the per-split oracle results)."""
import math
import random

import numpy as np
import pytest

import batch_cases as B
import oracle_lib as O
from test_gpu_parity import PATTERNS

pytestmark = pytest.mark.gpu

C3 = b"^[0-9]{4}-[0-9]{2}.*(WARN|ERROR) [a-z_]+"

_expected = {}


def _want(name, pattern, splits):
    """the per-split oracle result of a named split list: computed once, shared, never changed"""
    key = (name, bytes(pattern))
    if key not in _expected:
        _expected[key] = B.expected(pattern, splits)
    return _expected[key]


def _check(ctx, name, pattern, splits, load=True):
    if load:
        ctx.load(pattern)
    got = ctx.scan_batch(splits)
    B.assert_same(got, _want(name, pattern, splits), "%s %r" % (name, pattern))
    return len(got[0])


# ---- 1. the emulation test's fixed list, every parity pattern ----------------
@pytest.mark.parametrize("pattern", PATTERNS)
def test_fixed_splits(gpu_ctx, pattern):
    _check(gpu_ctx, "fixed", pattern, B.FIXED_SPLITS)
    for s in (b"", b"\n", b"x\nerror", B.FIXED_SPLITS[-3]):  # a one-split batch is a plain scan
        ln, st, le, sp, sb = gpu_ctx.scan_batch([s])
        for g, w in zip((ln, st, le), gpu_ctx.scan(s)):
            np.testing.assert_array_equal(g, w)
        assert sp.tolist() == [0] * len(ln) and sb.tolist() == [0, len(ln)]


# ---- 2. split boundaries at the scan's chunk and tile edges ------------------
EDGES = [4095, 4096, 4097, 65535, 65536, 65537, 262143, 262144, 262145, 3 * 262144 + 17]


def _edge_splits():
    import dgrep

    lens, at = [], 0
    for e in EDGES:  # begin[i + 1] = begin[i] + len_i + 1 lands on e
        lens.append(e - at - 1)
        at = e
    lens.append(5000)
    corpus = dgrep.synth_corpus_host(sum(lens), 11, 0)
    splits, off = [], 0
    for n in lens:
        splits.append(corpus[off:off + n])
        off += n
    assert B.begins(splits)[1:-1].tolist() == EDGES
    return splits


@pytest.mark.parametrize("chunk", [0, 4224])
@pytest.mark.parametrize("stepper,pattern,force,rows", [("sheng", b"error", "auto", 0), ("pair", C3, "auto", 0),
                                                         ("table", C3, "table", 0), ("filter", b"error", "filter", 4)])
def test_boundaries_at_scan_edges(gpu_ctx, stepper, pattern, force, rows, chunk):
    splits = _edge_splits()
    try:
        gpu_ctx.set_stepper(force, rows)
        gpu_ctx.set_lane_chunk(chunk)
        n = _check(gpu_ctx, "edges", pattern, splits)
        assert n > 0
        st = gpu_ctx.scan_stats()
        assert st["stepper"] == stepper, st
        assert st["matches"] == n
    finally:
        gpu_ctx.set_lane_chunk(0)
        gpu_ctx.set_stepper("auto", 0)


# ---- 3. many tiny splits ------------------------------------------------------
def _tiny_splits():
    rnd = random.Random(5000)
    out = []
    while len(out) < 5000:
        if len(out) == 1200:
            out += [b""] * 300
        elif len(out) == 3100:
            out += [b"\n"] * 300
        else:
            s = b"".join(rnd.choice(B.ALPHABET) for _ in range(rnd.randrange(14)))
            out.append(s[:rnd.randrange(41)])
    return out


@pytest.mark.parametrize("pattern", [b"", b"^$", b"error"])
def test_many_tiny_splits(gpu_ctx, pattern):
    splits = _tiny_splits()
    assert len(splits) == 5000 and max(map(len, splits)) <= 40
    n = _check(gpu_ctx, "tiny", pattern, splits)
    sb = _want("tiny", pattern, splits)[4]
    assert n > 0 and (np.diff(sb.astype(np.int64)) == 0).any() == (pattern != b"")  # splits with empty ranges
    if pattern == b"":
        assert gpu_ctx.scan_stats()["overflow_lanes"] > 0  # every line matches: the overflow pass ran


# ---- 4. mixed sizes: tiny, 3 MiB, one parked 1 MiB line, an unterminated tail --
def _mixed_splits():
    import dgrep

    long_line = b"y" * ((1 << 20) - 12) + b"error at k"
    assert b"\n" not in long_line
    return (B.random_splits(44, 60) + [dgrep.synth_corpus_host(3 << 20, 9, 0)] + [b"", b"k"] + [long_line] +
            B.random_splits(45, 20) + [b"first\nan error without its newline k"])


@pytest.mark.parametrize("pattern", [b"error", b"k$"])
def test_mixed_sizes(gpu_ctx, pattern):
    splits = _mixed_splits()
    _check(gpu_ctx, "mixed", pattern, splits)
    assert gpu_ctx.scan_stats()["pending"] >= 1  # the 1 MiB line was parked
    # the same through a ring of small staging pieces (a piece holds several
    # splits, a split spans several pieces, segments of >= 1 MiB copy threaded)
    try:
        gpu_ctx.set_ingest(3 << 19, 2, 2)
        _check(gpu_ctx, "mixed", pattern, splits, load=False)
        assert gpu_ctx.last_ingest_ms() > 0
        gpu_ctx.set_ingest(0)  # one direct copy of the assembled buffer
        _check(gpu_ctx, "mixed", pattern, splits, load=False)
    finally:
        gpu_ctx.set_ingest(64 << 20, 4, 4)


def test_workgroups_that_stream_several_tiles(gpu_ctx):
    """Above 8 workgroups per CU x 16 KiB the newline kernel's workgroups take
    several consecutive tiles each and carry their counts in registers from one
    to the next: 66 MiB gives an MI355X's 2,048 workgroups three tiles each,
    with split boundaries in first, middle and last ones (the smallest size at
    which that path runs; the oracle reads it with 16 threads)."""
    import dgrep

    m = 22 << 20
    lens = [m + 5, 17, 0, m - 1234, 1, m + 999 + 16384 * 2 + 40]
    corpus = dgrep.synth_corpus_host(sum(lens), 21, 0)
    splits, off = [], 0
    for n in lens:
        splits.append(corpus[off:off + n])
        off += n
    pattern = b"error"
    per = [O.grep_map(pattern, s, threads=16) for s in splits]
    counts = [len(p[0]) for p in per]
    want = tuple(np.concatenate([p[j] for p in per]) for j in range(3)) + (
        np.repeat(np.arange(len(splits), dtype=np.uint32), counts),
        np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64))
    gpu_ctx.load(pattern)
    B.assert_same(gpu_ctx.scan_batch(splits), want, "66 MiB")
    assert sum(counts) > 1000


# ---- 5. the device form -------------------------------------------------------
def _device_call(ctx, packed_t, splits, cap, with_ranges=True, sentinel=-7):
    import torch

    k = len(splits)
    mk = lambda n, dt: torch.full((max(n, 1),), sentinel, dtype=dt, device="cuda")
    ln, st, le, sp = mk(cap + 8, torch.int64), mk(cap + 8, torch.int64), mk(cap + 8, torch.int64), mk(cap + 8, torch.int32)
    sb = mk(k + 1, torch.int64)
    torch.cuda.synchronize()
    count = ctx.scan_batch_device(packed_t.data_ptr(), sum(map(len, splits)) + k - 1, [len(s) for s in splits],
                                  ln.data_ptr(), st.data_ptr(), le.data_ptr(), sp.data_ptr(),
                                  sb.data_ptr() if with_ranges else 0, cap)
    host = lambda t, dt: t.cpu().numpy().view(dt)
    return count, (host(ln, np.uint64), host(st, np.uint64), host(le, np.uint64), host(sp, np.uint32),
                   host(sb, np.uint64))


def test_device_form(gpu_ctx):
    import torch

    import dgrep

    splits = B.FIXED_SPLITS + B.random_splits(77, 400) + [dgrep.synth_corpus_host(300000, 3, 0)]
    pattern = b"error"
    want = _want("device", pattern, splits)
    total = len(want[0])
    assert total > 40
    packed = np.frombuffer(B.pack(splits), np.uint8).copy()
    packed_t = torch.from_numpy(packed).cuda()
    gpu_ctx.load(pattern)
    sent64, sent32 = np.uint64(2**64 - 7), np.uint32(2**32 - 7)

    # capacity below the count: the true count, nothing written past capacity
    cap = total // 3
    count, got = _device_call(gpu_ctx, packed_t, splits, cap)
    assert count == total
    for a in got[:3]:
        assert (a[cap:] == sent64).all()
    assert (got[3][cap:] == sent32).all()
    # a second call with enough capacity is exact
    count, got = _device_call(gpu_ctx, packed_t, splits, total)
    assert count == total
    B.assert_same([a[:total] for a in got[:4]] + [got[4]], want, "device form")
    for a in got[:3]:
        assert (a[total:] == sent64).all()
    assert gpu_ctx.scan_stats()["matches"] == total
    # d_split_begin = NULL
    count, got = _device_call(gpu_ctx, packed_t, splits, total + 5, with_ranges=False)
    assert count == total and (got[4] == sent64).all()
    B.assert_same([a[:total] for a in got[:4]], want[:4], "device form, no ranges")

    # one separator byte overwritten: DGREP_E_INVALID naming the split, then a correct call
    begin = B.begins(splits)
    bad = 37
    broken = packed.copy()
    assert broken[int(begin[bad + 1]) - 1] == 10
    broken[int(begin[bad + 1]) - 1] = ord("x")
    broken_t = torch.from_numpy(broken).cuda()
    with pytest.raises(dgrep.DgrepError) as ei:
        _device_call(gpu_ctx, broken_t, splits, total)
    assert ei.value.code == dgrep.DGREP_E_INVALID and "split %d " % bad in str(ei.value), str(ei.value)
    count, got = _device_call(gpu_ctx, packed_t, splits, total)
    assert count == total
    B.assert_same([a[:total] for a in got[:4]] + [got[4]], want, "device form after a refused buffer")
    # lengths that do not add up to n_packed are refused before any GPU work
    with pytest.raises(dgrep.DgrepError) as ei:
        gpu_ctx.scan_batch_device(packed_t.data_ptr(), len(packed) - 1, [len(s) for s in splits], 0, 0, 0, 0, 0, 0)
    assert ei.value.code == dgrep.DGREP_E_INVALID


# ---- 6. MapBatch ---------------------------------------------------------------
def test_map_batch_equals_map_per_file(gpu_ctx):
    import dgrep

    files = [("a.log", "ok\nan error\n"), ("b.log", b"error\xff\xfe\nfine\n\xe2\x82 error"), ("empty", ""),
             ("empty.bin", b""), ("c.log", "no match here"), ("d.log", "error"), ("e.log", b"\n\nerror\n\n"),
             ("\xe9.log", "caf\xe9 error €\nx"), ("g.log", "error\n" * 50), ("h.log", b"\xe2\x82"),
             ("i.log", b"\xac error"), ("j.log", "last error without newline")]
    try:
        for pat in ("error", "", "^$"):
            dgrep.set_pattern(pat)
            want = [dgrep.Map(f, c) for f, c in files]
            got = dgrep.MapBatch(files)
            assert got == want, pat
            assert sum(map(len, got)) > 0
            for (f, c), kva in zip(files, got):
                assert all(isinstance(kv.Value, str if isinstance(c, str) else bytes) for kv in kva)
        assert dgrep.MapBatch([]) == []
    finally:
        dgrep.set_pattern("")


# ---- 7. nothing leaks from a batch into the next call ----------------------------
def test_stats_times_and_following_scan(gpu_ctx):
    import dgrep

    splits = B.random_splits(9, 200) + [dgrep.synth_corpus_host(200000, 5, 0)] + B.FIXED_SPLITS
    pattern = b"(?i)ERROR"
    n = _check(gpu_ctx, "stats", pattern, splits)
    st = gpu_ctx.scan_stats()
    assert st["matches"] == n and n > 0
    nl_ms, rb_ms = gpu_ctx.last_batch_ms()
    assert math.isfinite(nl_ms) and math.isfinite(rb_ms) and nl_ms >= 0 and rb_ms >= 0
    assert nl_ms > 0 and rb_ms > 0  # both legs ran
    data = b"x\n" + dgrep.synth_corpus_host(150000, 6, 0) + b"\nan ERROR at the end"
    for g, w in zip(gpu_ctx.scan(data), O.grep_map(pattern, data)):
        np.testing.assert_array_equal(g, w)
    assert gpu_ctx.scan_stats()["matches"] == len(O.grep_map(pattern, data)[0])
    # and a batch again after the plain scan
    _check(gpu_ctx, "stats", pattern, splits, load=False)
