"""The bounded windowed scan on the GPU (DGREP_STREAM_BOUNDED,
dgrep_scan_bounded, dgrep_stream_carry_stats): a line longer than the window
is folded into its DFA state, so the two window buffers never hold two windows
or more each. The one-shot, the stream (every call's records against the model
of carry_cases.bounded) and Context.scan of the whole split are compared with
each other and with the oracle, bit for bit."""
import random
import zlib

import numpy as np
import pytest

import carry_cases as CC
import oracle_lib as O
import stepper_cells as SC
import window_cases as WC

pytestmark = pytest.mark.gpu

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


def _footprint(W):
    """both buffers: fewer than 2 W bytes each, rounded up to 256, plus 64 (win_reserve)"""
    return 2 * (2 * W + 320)


def _run_stream(ctx, pieces, W, bounded=True):
    """feeds and finish: (the per-call results, the concatenated records, stats + carry stats, data_bytes after
    every feed)"""
    seen = []
    with ctx.stream(W, bounded=bounded) as st:
        calls = []
        for p in pieces:
            calls.append(st.feed(p))
            seen.append(st.stats()["data_bytes"])
        calls.append(st.finish())
        stats = dict(st.stats(), **st.carry_stats())
    cat = [np.concatenate([c[k] for c in calls]) for k in range(3)]
    return calls, cat, stats, seen


def _check(ctx, key, pattern, data, pieces, W, model=None):
    """resident, one-shot bounded and bounded stream against the oracle; returns (record count, stats)"""
    want = _want(key, pattern, data)
    _same(ctx.scan(data), want, "%s resident" % key)
    _same(ctx.scan_windowed(data, W, bounded=True), want, "%s bounded w=%d" % (key, W))
    assert ctx.scan_stats()["matches"] == len(want[0]), key  # the true count: the dropped head record is not in it
    calls, cat, stats, seen = _run_stream(ctx, pieces, W)
    _same(cat, want, "%s bounded stream w=%d" % (key, W))
    assert max(seen + [stats["data_bytes"]]) <= _footprint(W), (key, seen, stats)
    if model is not None:
        assert len(calls) == len(model)
        for i, (c, m) in enumerate(zip(calls, model)):
            _same(c, [[r[k] for r in m] for k in range(3)], "%s call %d w=%d" % (key, i, W))
    # the bounded calls leave nothing behind: a resident scan right after is still exact
    _same(ctx.scan(data), want, "%s resident after" % key)
    return len(want[0]), stats


# ---- 1. the windowed cases under the flag ---------------------------------------
@pytest.mark.parametrize("W", WC.WINDOWS)
@pytest.mark.parametrize("pattern", [b"error", b"^$", b"", b"("])
def test_window_cases_bounded(gpu_ctx, pattern, W):
    import dgrep

    cp = gpu_ctx.load(pattern)
    dfa, rx = CC.Dfa(cp), O.Regexp(pattern)
    total = folds = 0
    for case in (c for c in WC.CASES if c.window == W):
        pieces = WC.pieces_of(case.data, case.cuts)
        model, info = CC.bounded(pieces, W, dfa, rx.match)
        n, stats = _check(gpu_ctx, case.name, pattern, case.data, pieces, W, model=model)
        total += n
        if pattern == b"(":
            assert bool(cp.flags & dgrep.DFA_MATCH_NONE)
            assert stats["windows"] == 0 and stats["data_bytes"] == 0 and stats["folds"] == 0, stats
        else:
            assert stats["folds"] == info["folds"] and stats["folded_bytes"] == info["folded_bytes"], (case.name, stats)
            assert stats["max_carry"] == info["max_carry"], (case.name, stats, info)
            folds += stats["folds"]
    assert (total > 0) == (pattern != b"(") and (folds > 0) == (pattern != b"(")


# ---- 2. lines longer than the window ----------------------------------------------
@pytest.mark.parametrize("case", CC.LONG, ids=lambda c: c.name)
def test_long_lines_stay_bounded(gpu_ctx, case):
    W = case.window
    cp = gpu_ctx.load(case.pattern)
    pieces = WC.pieces_of(case.data, case.cuts)
    model, info = CC.bounded(pieces, W, CC.Dfa(cp), O.Regexp(case.pattern).match)
    key = "carry/" + case.name.rsplit("/", 2)[0] + "/w%d" % W
    n, stats = _check(gpu_ctx, key, case.pattern, case.data, pieces, W, model=model)
    assert stats["folds"] >= 1 and stats["folds"] == info["folds"], stats
    assert stats["max_carry"] >= case.longest and stats["max_carry"] == info["max_carry"], (stats, info)
    assert stats["chunks"] >= stats["folds"] * (W // 256), stats
    assert stats["walk_ms"] > 0, stats
    # the same split with the flag off still grows: the existing behaviour, unchanged
    _, cat, plain, seen = _run_stream(gpu_ctx, pieces, W, bounded=False)
    _same(cat, _want(key, case.pattern, case.data), key + " unbounded stream")
    assert max(seen + [plain["data_bytes"]]) >= case.longest, (plain, seen)
    assert plain["folds"] == 0 and plain["chunks"] == 0 and plain["guess_misses"] == 0, plain
    assert plain["max_carry"] >= case.longest, plain


def test_long_line_verdict_is_the_whole_lines(gpu_ctx):
    """hit_middle / miss_middle differ in one byte of a middle window: the record follows it"""
    gpu_ctx.load(CC.SHENG8)
    for W in WC.WINDOWS:
        by = {c.name: c for c in CC.LONG}
        hit, miss = by["hit_middle/whole/w%d" % W], by["miss_middle/whole/w%d" % W]
        got = gpu_ctx.scan_windowed(hit.data, W, bounded=True)
        assert 13 * W // 2 in got[2].tolist()
        got = gpu_ctx.scan_windowed(miss.data, W, bounded=True)
        assert got[2].size and int(got[2].max()) < W
        assert gpu_ctx.scan_stats()["stepper"] == "sheng"


# ---- 3. every stepper's pattern ------------------------------------------------------
@pytest.mark.parametrize("cell", SC.CELLS, ids=lambda c: c.name)
def test_every_stepper(gpu_ctx, cell):
    """A line of 5.25 windows of the cell's `miss` byte with its `hit` planted at the end (the last window), in
    the first window, in a middle one, or across a fold (its first bytes end the part a fold swallows, the rest
    stays as bytes); and one byte of a planted hit put back to `miss`, in the folded part or in the kept one.
    Whether the line matches follows the plant, as the oracle says; both verdicts occur."""
    ctx, W = gpu_ctx, 8192
    hit, m = cell.hit, cell.miss
    n = 5 * W + W // 4
    across = 4 * W - 300 - len(hit) // 2  # the line starts at 300: a whole feed folds at 4 W - 300 of it
    try:
        ctx.set_stepper(cell.force)
        cp = ctx.load(cell.pattern)
        assert not cp.partial
        dfa, rx = CC.Dfa(cp), O.Regexp(cell.pattern)
        verdicts = {}
        for name, at, broken in (("end", n - len(hit), None), ("end_broken", n - len(hit), len(hit) - 1),
                                 ("across", across, None), ("across_broken_folded", across, 0),
                                 ("across_broken_kept", across, len(hit) - 1),
                                 ("first", 100, None), ("middle", 2 * W + 77, None), ("none", None, None)):
            line = bytearray(m * n)
            if at is not None:
                line[at:at + len(hit)] = hit
                if broken is not None:
                    line[at + broken:at + broken + 1] = m
            data = bytes(SC.pad(300, cell)) + bytes(line) + b"\n" + bytes(SC.pad(200, cell)) + hit
            key = "carry-cell/%s/%s" % (cell.name, name)
            want = _want(key, cell.pattern, data)
            verdicts[name] = n in want[2].tolist()
            got = ctx.scan_windowed(data, W, bounded=True)
            _same(got, want, key + " bounded")
            st = ctx.scan_stats()
            assert st["stepper"] == cell.expected["stepper"], (key, st)
            assert st["matches"] == len(want[0]), (key, st)
            pieces = WC.pieces_of(data, WC.random_cuts(key, len(data), 3))
            _, cat, stats, seen = _run_stream(ctx, pieces, W)
            _same(cat, want, key + " bounded stream")
            # a fold and the line's last part take fewer than two windows each: 5.25 windows need two folds or more
            folds = CC.bounded(pieces, W, dfa, rx.match)[1]["folds"]
            assert stats["folds"] == folds >= 2 and max(seen) <= _footprint(W), (key, stats, seen)
        assert verdicts["end"] and not verdicts["end_broken"] and not verdicts["none"], verdicts
        assert not verdicts["across_broken_folded"] and not verdicts["across_broken_kept"], verdicts
        assert verdicts["across"] == verdicts["first"] == verdicts["middle"], verdicts  # anywhere, or only at the end
    finally:
        ctx.set_stepper("auto")


# ---- 4. automata that never forget --------------------------------------------------
def _mod(p):
    return b"^(([^k]*k){%d})*[^k]*$" % p


@pytest.mark.parametrize("W", WC.WINDOWS)
@pytest.mark.parametrize("p", [2, 3, 7])
def test_k_count_modulo(gpu_ctx, p, W):
    """The DFA of `the number of k is divisible by p` keeps the count for the whole line: a chunk's entry state
    is one of p memory classes whatever the lookback saw. Seven classes exceed the four guesses, so the fix
    kernel must walk chunks again."""
    pattern = _mod(p)
    cp = gpu_ctx.load(pattern)
    dfa, rx = CC.Dfa(cp), O.Regexp(pattern)
    verdicts, misses = set(), 0
    for seed in range(4):
        data, nk = CC.memory_line(W, seed + (0 if W == 4096 else 7))  # 40 .. 43 k: 42 is divisible by 2, 3 and 7
        key = "mod/%d/%d" % (W, seed)
        pieces = WC.pieces_of(data, WC.random_cuts(key, len(data), 3))
        model, info = CC.bounded(pieces, W, dfa, rx.match)
        _, stats = _check(gpu_ctx, key, pattern, data, pieces, W, model=model)
        want = _want(key, pattern, data)
        assert (12 * W + W // 3 in want[2].tolist()) == (nk % p == 0), (key, nk)
        verdicts.add(nk % p == 0)
        # 12.3 windows in folds of fewer than two; every fold spans 16 chunks or more
        assert stats["folds"] == info["folds"] >= 6 and stats["chunks"] >= 8 * stats["folds"], stats
        assert stats["guess_misses"] <= stats["chunks"], stats
        misses += stats["guess_misses"]
    assert verdicts == {True, False}
    if p == 7:
        assert misses > 0  # the re-run path ran


def test_keyword_before_the_lookback_is_absorbing(gpu_ctx):
    """a keyword at the line's start puts the DFA in its absorbing accepting state: no lookback can know, the
    fix kernel stops there, and the line still matches; without it, it does not"""
    pattern = b"alpha|bravo|charlie"
    cp = gpu_ctx.load(pattern)
    for W in WC.WINDOWS:
        n = 12 * W + 5
        for name, line in (("hit", b"xx bravo " + CC.body(n - 9)), ("miss", b"xx bravx " + CC.body(n - 9)),
                           ("late", CC.body(n - 7) + b"charlie")):
            data = WC.lines(500, 41) + line + b"\nalpha\n" + CC.body(3 * W) + b"\n"
            key = "kw/%s/%d" % (name, W)
            pieces = WC.pieces_of(data, WC.random_cuts(key, len(data), 2))
            model, info = CC.bounded(pieces, W, CC.Dfa(cp), O.Regexp(pattern).match)
            _, stats = _check(gpu_ctx, key, pattern, data, pieces, W, model=model)
            assert stats["folds"] == info["folds"], (stats, info)
            assert (n in _want(key, pattern, data)[2].tolist()) == (name != "miss")
            assert stats["folds"] >= 7, stats  # 12 windows and 3 windows, in folds of fewer than two


def test_u32_state_ids(gpu_ctx):
    """a[ab]{16}$: 131073 states, so the walk's table has u32 entries and its rows stay in global memory"""
    pattern = b"a[ab]{16}$"
    cp = gpu_ctx.load(pattern)
    assert cp.nstates > 65535 and not cp.partial
    W = 4096
    rnd = random.Random(zlib.crc32(b"carry u32"))
    verdicts = set()
    for i in range(2):
        line = bytearray(rnd.choice(b"ab") for _ in range(5 * W + 123))
        line[-17] = ord("a") if i == 0 else ord("b")
        data = b"ab\n" + bytes(line) + b"\n" + b"a" * 17 + b"\nb"
        key = "u32/%d" % i
        want = _want(key, pattern, data)
        verdicts.add(len(line) in want[2].tolist())
        _same(gpu_ctx.scan_windowed(data, W, bounded=True), want, key)
        _, cat, stats, seen = _run_stream(gpu_ctx, [data[:7777], data[7777:]], W)
        _same(cat, want, key + " stream")
        assert stats["folds"] >= 4 and max(seen) <= _footprint(W), (stats, seen)
    assert verdicts == {True, False}
    assert gpu_ctx.scan_stats()["stepper"] == "filter"


# ---- 5. refusals and hygiene -----------------------------------------------------------
def test_refusals(gpu_ctx):
    import dgrep

    ctx = gpu_ctx
    ctx.load(b"error")
    with pytest.raises(dgrep.DgrepError) as e:
        ctx.stream(4096, values=True, bounded=True)
    assert e.value.code == dgrep.DGREP_E_INVALID and "VALUES" in str(e.value)
    C3 = b"^[0-9]{4}-[0-9]{2}.*(WARN|ERROR) [a-z_]+"
    cp = ctx.load(dgrep.CompiledPattern(C3, state_budget=16))
    assert cp.partial
    with pytest.raises(dgrep.UnsupportedPattern) as e:
        ctx.stream(4096, bounded=True)
    assert e.value.code == dgrep.DGREP_E_UNSUPPORTED and "PARTIAL" in str(e.value)
    with pytest.raises(dgrep.UnsupportedPattern) as e:
        ctx.scan_windowed(b"2024-01 ERROR io_wait\n", 4096, bounded=True)
    assert "PARTIAL" in str(e.value)
    # the partial pattern still streams without the flag
    assert ctx.scan_windowed(b"2024-01 ERROR io_wait\n", 4096)[0].tolist() == [1]


def test_load_mid_stream_and_feed_after_finish(gpu_ctx):
    import dgrep

    ctx, W = gpu_ctx, 4096
    ctx.load(b"error")
    with ctx.stream(W, bounded=True) as st:
        assert st.feed(b"an error\n" + b"and " * 2000)[0].tolist() == [1]
        assert st.carry_stats()["folds"] == 1
        ctx.load(b"and")
        with pytest.raises(dgrep.DgrepError) as e:
            st.feed(b" more\n")
        assert e.value.code == dgrep.DGREP_E_INVALID and "pattern" in str(e.value)
        with pytest.raises(dgrep.DgrepError) as e:
            st.finish()
        assert e.value.code == dgrep.DGREP_E_INVALID
    with ctx.stream(W, bounded=True) as st:
        assert st.feed(b"")[0].tolist() == []
        assert st.feed(b"x\n" + b"and " * 3000)[0].tolist() == []
        ln, s, l = st.finish()
        assert (ln.tolist(), s.tolist(), l.tolist()) == ([2], [2], [12000])
        with pytest.raises(dgrep.DgrepError) as e:
            st.feed(b"z\n")
        assert e.value.code == dgrep.DGREP_E_INVALID and "finish" in str(e.value)
    _same(ctx.scan(b"x\nand y"), ([2], [2], [5]), "resident after bounded streams")
