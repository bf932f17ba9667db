"""The windowed scan on the GPU (dgrep_scan_windowed, dgrep_stream_*,
MapStream): the windowed result, the stream result (the concatenation of the
feeds and the finish) and Context.scan of the whole split are compared with
each other and with the oracle, bit for bit. Where the split is small the
records of every single call are compared with window_cases.windowed() too: a
feed returns exactly the lines it completed."""
import zlib

import numpy as np
import pytest

import oracle_lib as O
import stepper_cells as SC
import window_cases as WC

pytestmark = pytest.mark.gpu

C3 = b"^[0-9]{4}-[0-9]{2}.*(WARN|ERROR) [a-z_]+"
SHENG8 = b"^[a-j ]*error[a-j ]*$"

_oracle = {}


def _want(key, pattern, data):
    """the oracle's Map of a named split: computed once, shared, never changed"""
    k = (key, bytes(pattern))
    if k not in _oracle:
        _oracle[k] = O.grep_map(pattern, data, threads=16)
    return _oracle[k]


def _same(got, want, msg):
    assert len(got[0]) == len(want[0]), (msg, len(got[0]), len(want[0]))
    for g, w in zip(got[:3], want[:3]):
        np.testing.assert_array_equal(np.asarray(g, np.uint64), np.asarray(w, np.uint64), err_msg=msg)


def _run_stream(ctx, pieces, W, values=False, each=None):
    """feeds and finish: (the per-call results, the concatenated records, the stream's stats)"""
    with ctx.stream(W, values=values) as st:
        calls = []
        for p in pieces:
            calls.append(st.feed(p))
            if each:
                each(st)
        calls.append(st.finish())
        stats = st.stats()
    cat = [np.concatenate([c[k] for c in calls]) for k in range(3)]
    if values:
        cat.append([v for c in calls for v in c[3]])
    return calls, cat, stats


def _check(ctx, key, pattern, data, pieces, W, values=False, model=None):
    """all three ways against the oracle; returns (record count, stream stats)"""
    want = _want(key, pattern, data)
    whole = ctx.scan(data)
    _same(whole, want, "%s resident" % key)
    win = ctx.scan_windowed(data, W)
    _same(win, want, "%s windowed w=%d" % (key, W))
    assert ctx.scan_stats()["matches"] == len(want[0]), key  # the stats are the sum over the windows
    calls, cat, stats = _run_stream(ctx, pieces, W, values)
    _same(cat, want, "%s stream w=%d" % (key, W))
    if values:
        assert len(cat[3]) == len(want[0])
        for s, l, v in zip(want[1].tolist(), want[2].tolist(), cat[3]):
            assert v == data[s:s + l], (key, s, l)
    if model is not None:
        assert len(calls) == len(model)
        for i, (c, m) in enumerate(zip(calls, model)):
            _same(c, [[r[k] for r in m] for k in range(3)], "%s call %d w=%d" % (key, i, W))
    # the windowed calls leave nothing behind: a resident scan right after is still exact
    _same(ctx.scan(data), want, "%s resident after" % key)
    return len(want[0]), stats


# ---- 1. where the '\n' falls, and the feed patterns ---------------------------
@pytest.mark.parametrize("W", WC.WINDOWS)
@pytest.mark.parametrize("pattern", [b"error", b"^$", b"", b"("])
def test_newline_positions_and_feed_patterns(gpu_ctx, pattern, W):
    import dgrep

    cp = gpu_ctx.load(pattern)
    assert bool(cp.flags & dgrep.DFA_MATCH_NONE) == (pattern == b"(")
    assert bool(cp.flags & dgrep.DFA_MATCH_ALL) == (pattern == b"")
    rx = O.Regexp(pattern)
    total = 0
    for case in (c for c in WC.CASES if c.window == W):
        pieces = WC.pieces_of(case.data, case.cuts)
        model, _ = WC.windowed(pieces, W, rx.match)
        n, stats = _check(gpu_ctx, case.name, pattern, case.data, pieces, W, values=pattern in (b"error", b""),
                          model=model)
        total += n
        if pattern == b"(":
            assert stats["windows"] == 0 and stats["data_bytes"] == 0, stats  # nothing was copied
    assert (total > 0) == (pattern != b"(")


# ---- 2. a line of 3.5 windows: the buffers must grow ---------------------------
@pytest.mark.parametrize("W", WC.WINDOWS)
@pytest.mark.parametrize("at_start", [True, False], ids=["hit_first", "hit_last"])
def test_long_line_grows_the_buffers(gpu_ctx, at_start, W):
    gpu_ctx.load(SHENG8)
    data, n = WC.long_line(W, at_start)
    key = "long/%d/%d" % (at_start, W)
    for cuts in ([], WC.random_cuts(key, len(data), 6)):
        count, stats = _check(gpu_ctx, key, SHENG8, data, WC.pieces_of(data, cuts), W, values=True)
        assert n in _want(key, SHENG8, data)[2].tolist() and count >= 2
        assert stats["max_carry"] >= n, stats
        assert stats["data_bytes"] >= n, stats
    assert gpu_ctx.scan_stats()["stepper"] == "sheng"


# ---- 3. every stepper ------------------------------------------------------------
@pytest.mark.parametrize("cell", SC.CELLS, ids=lambda c: c.name)
def test_every_stepper(gpu_ctx, cell):
    ctx, W = gpu_ctx, 8192
    try:
        ctx.set_stepper(cell.force)
        ctx.load(cell.pattern)
        ctx.set_lane_chunk(0)
        ctx.scan(b"probe\n")
        st = ctx.scan_stats()
        base = SC.geometry(cell, st["lane_chunk"], st["lane_slots"])
        for gen in SC.GENERATORS:
            geo, cases = SC.cases(cell, gen, base)
            ctx.set_lane_chunk(geo.force_chunk)
            for case in cases:
                key = "%s/%s" % (cell.name, case.name)
                want = _want(key, cell.pattern, case.data)
                SC.check_planted(case, geo, want)
                _same(ctx.scan_windowed(case.data, W), want, key + " windowed")
                st = ctx.scan_stats()
                assert st["stepper"] == cell.expected["stepper"], (key, st)
                assert st["matches"] == len(want[0]), (key, st)
                cuts = WC.random_cuts(key, len(case.data), 3)
                _, cat, _ = _run_stream(ctx, WC.pieces_of(case.data, cuts), W)
                _same(cat, want, key + " stream")
    finally:
        ctx.set_lane_chunk(0)
        ctx.set_stepper("auto")


def _corpus(n, seed):
    import dgrep

    return dgrep.synth_corpus_host(n, seed, 0)


@pytest.mark.parametrize("W", WC.WINDOWS)
@pytest.mark.parametrize("partial", [False, True], ids=["c3", "c3_partial"])
def test_c3_and_nfa_verify(gpu_ctx, partial, W):
    import dgrep

    data = _corpus(200 * 1000, 21)
    cp = gpu_ctx.load(dgrep.CompiledPattern(C3, state_budget=16) if partial else C3)
    assert cp.partial == partial
    key = "c3/%d" % len(data)
    n, _ = _check(gpu_ctx, key, C3, data, WC.pieces_of(data, WC.random_cuts(key, len(data), 4)), W, values=True)
    assert n > 0
    st = gpu_ctx.scan_stats()
    assert st["stepper"] == ("filter" if partial else "pair"), st


# ---- 4. a window larger than a scan tile -----------------------------------------
@pytest.mark.parametrize("stepper,pattern", [("sheng", b"error"), ("pair", C3)])
def test_window_spans_several_tiles(gpu_ctx, stepper, pattern):
    data, W = _corpus(1 << 20, 22), 320 << 10
    gpu_ctx.load(pattern)
    key = "tiles/%d" % len(data)
    n, stats = _check(gpu_ctx, key, pattern, data, [data[:700001], data[700001:]], W, values=True)
    assert n > 0
    gpu_ctx.scan_windowed(data, W)
    st = gpu_ctx.scan_stats()
    assert st["stepper"] == stepper, st
    assert stats["windows"] >= 4 and st["tiles"] > stats["windows"], (st, stats)
    assert st["matches"] == n and st["scan_attempts"] >= 4, st


# ---- 5. the staging ring ------------------------------------------------------------
def test_staging_ring(gpu_ctx):
    data, W = _corpus(9 << 20, 23), 4 << 20
    gpu_ctx.load(b"error")
    try:
        gpu_ctx.set_ingest(1 << 20, 2, 2)
        key = "ring/%d" % len(data)
        n, stats = _check(gpu_ctx, key, b"error", data, [data[:5 << 20], data[5 << 20:]], W)
        assert n > 0 and stats["windows"] >= 3
    finally:
        gpu_ctx.set_ingest(64 << 20, 4, 4)


# ---- 6. the footprint condition -------------------------------------------------------
def test_footprint_is_set_by_the_window(gpu_ctx):
    W, n = 8192, 2 << 20
    data = WC.lines(n, 24, longest=200)
    longest = max(map(len, data.split(b"\n")))
    assert 150 <= longest <= 200
    bound = 4 * (W + longest + 64)
    gpu_ctx.load(b"error")
    seen = []

    def each(st):
        seen.append(st.stats()["data_bytes"])

    pieces = [data[o:o + 100 * 1000] for o in range(0, n, 100 * 1000)]
    _, cat, stats = _run_stream(gpu_ctx, pieces, W, each=each)
    _same(cat, _want("footprint", b"error", data), "footprint")
    assert max(seen) <= bound and stats["data_bytes"] <= bound, (max(seen), stats, bound)
    assert stats["windows"] >= n // W, stats
    assert stats["max_carry"] <= longest, stats
    assert stats["cut_ms"] > 0, stats


# ---- 7. everything else ---------------------------------------------------------------
def test_load_mid_stream_and_feed_after_finish(gpu_ctx):
    import dgrep

    ctx = gpu_ctx
    ctx.load(b"error")
    with ctx.stream(4096) as st:
        assert st.feed(b"an error\nand")[0].tolist() == [1]
        ctx.load(b"and")
        with pytest.raises(dgrep.DgrepError) as e:
            st.feed(b" more\n")
        assert e.value.code == dgrep.DGREP_E_INVALID and "pattern" in str(e.value)
        with pytest.raises(dgrep.DgrepError) as e:
            st.finish()
        assert e.value.code == dgrep.DGREP_E_INVALID
    with ctx.stream(4096, values=True) as st:
        assert st.feed(b"")[0].tolist() == []
        assert st.feed(b"x\nand y")[0].tolist() == []
        ln, s, l, v = st.finish()
        assert (ln.tolist(), s.tolist(), l.tolist(), v) == ([2], [2], [5], [b"and y"])
        with pytest.raises(dgrep.DgrepError) as e:
            st.feed(b"z\n")
        assert e.value.code == dgrep.DGREP_E_INVALID and "finish" in str(e.value)
    _same(ctx.scan(b"x\nand y"), ([2], [2], [5]), "resident after streams")


def test_map_stream_equals_map(gpu_ctx):
    import dgrep

    data = WC.lines(50 * 1000, 25) + b"\n\nthe last error"  # two empty lines for ^$
    cuts = WC.random_cuts("mapstream", len(data), 7)
    pieces = WC.pieces_of(data, cuts)
    old = dgrep.pattern
    try:
        for pat in ("error", "", "^$"):
            dgrep.set_pattern(pat)
            want = dgrep.Map("f.txt", data)
            assert dgrep.MapStream("f.txt", pieces, window=4096) == want
            assert dgrep.MapStream("f.txt", iter([data]), window=8192) == want
            assert len(want) > 0
        text = data.decode()
        assert dgrep.MapStream("f", [text[:999], text[999:]], window=4096) == dgrep.Map("f", text)
    finally:
        dgrep.set_pattern(old)
