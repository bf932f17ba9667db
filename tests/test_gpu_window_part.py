"""The windowed partition writer on the GPU (dgrep_stream_*_partitions,
dgrep_map_partitions_windowed, MapPartitionsStream). The reference for every
test is Context.map_partitions on the whole split -- the resident writer, which
this feature leaves as it is: the rows of all calls, joined per partition, are
compared with it bit for bit. Where the split is small the rows of every single
call are compared with window_part_cases.windowed_partitions() too."""
import pytest

import oracle_lib as O
import stepper_cells as SC
import window_cases as WC
import window_part_cases as PC

pytestmark = pytest.mark.gpu

C3 = b"^[0-9]{4}-[0-9]{2}.*(WARN|ERROR) [a-z_]+"
FILENAME = b"pg-\"quoted\".txt"

_ref = {}


def _want(ctx, key, fname, data, R):
    """Context.map_partitions of a named split under the loaded pattern: computed once, shared, never changed"""
    k = (key, bytes(ctx.pattern.pattern), bytes(fname), R)
    if k not in _ref:
        _ref[k] = ctx.map_partitions(fname, data, R)
    return _ref[k]


def _run(ctx, pieces, W, fname, R, each=None):
    """feeds and finish: (every call's rows, the stream's stats)"""
    with ctx.partition_stream(W, fname, R) as st:
        calls = []
        for p in pieces:
            calls.append(st.feed(p))
            if each:
                each(st)
        calls.append(st.finish())
        stats = st.stats()
    assert all(len(row) == R for rows in calls for row in rows)
    assert stats["rows"] == sum(len(rows) for rows in calls)
    assert stats["out_bytes"] == sum(len(c) for rows in calls for row in rows for c in row)
    return calls, stats


def _check(ctx, key, fname, data, pieces, W, R, model=None):
    """the stream and the one-shot against the resident writer (and the model, call by call)"""
    want = _want(ctx, key, fname, data, R)
    calls, stats = _run(ctx, pieces, W, fname, R)
    assert PC.joined(calls, R) == want, (key, W, R)
    assert ctx.map_partitions_windowed(fname, data, R, W) == want, (key, W, R)
    if model is not None:
        assert calls == model, (key, W, R)
        assert PC.joined(model, R) == want, (key, W, R)
    return want, stats


# ---- 1. where the '\n' falls, the feed patterns, the digit crossings -------------
@pytest.mark.parametrize("W", WC.WINDOWS)
@pytest.mark.parametrize("pattern", [b"error", b"^$", b"", b"("])
def test_newline_positions_and_feed_patterns(gpu_ctx, pattern, W):
    gpu_ctx.load(pattern)
    match = O.Regexp(pattern).match
    total = 0
    for case in (c for c in PC.CASES if c.window == W):
        pieces = WC.pieces_of(case.data, case.cuts)
        for R in (1, 10, 65535):
            if R == 65535 and len(case.data) >= 1024:
                continue
            model = PC.windowed_partitions(pieces, W, match, FILENAME, R)
            want, stats = _check(gpu_ctx, case.name, FILENAME, case.data, pieces, W, R, model=model)
            total += sum(map(len, want))
            if pattern == b"(":
                assert stats["windows"] == 0 and stats["data_bytes"] == 0 and stats["rows"] == 0, stats
    assert (total > 0) == (pattern != b"(")


# ---- 2. every stepper; the NFA verify ---------------------------------------------
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
                want = _want(ctx, key, FILENAME, case.data, 10)
                assert ctx.map_partitions_windowed(FILENAME, case.data, 10, W) == want, key
                st = ctx.scan_stats()
                assert st["stepper"] == cell.expected["stepper"], (key, st)
                assert st["matches"] == sum(p.count(b"\n") for p in want), (key, st)
                cuts = WC.random_cuts(key, len(case.data), 3)
                calls, _ = _run(ctx, WC.pieces_of(case.data, cuts), W, FILENAME, 10)
                assert PC.joined(calls, 10) == want, key
    finally:
        ctx.set_lane_chunk(0)
        ctx.set_stepper("auto")


@pytest.mark.parametrize("partial", [False, True], ids=["c3", "c3_partial"])
def test_c3_and_nfa_verify(gpu_ctx, partial):
    import dgrep

    data = dgrep.synth_corpus_host(200 * 1000, 21, 0)
    cp = gpu_ctx.load(dgrep.CompiledPattern(C3, state_budget=16) if partial else C3)
    assert cp.partial == partial
    key = "c3/%d/%d" % (len(data), partial)
    for W in WC.WINDOWS:
        want, stats = _check(gpu_ctx, key, FILENAME, data, WC.pieces_of(data, WC.random_cuts(key, len(data), 4)), W, 10)
        assert sum(map(len, want)) > 0 and stats["rows"] > 1
    assert gpu_ctx.scan_stats()["stepper"] == ("filter" if partial else "pair")


# ---- 3. file names -----------------------------------------------------------------
NAMES = [b"", b"plain.txt", b'q"uo\\te<s>&.log', b"bad-\xff\xc0\x80-utf8", b"u2028-\xe2\x80\xa8-\xc3\xa9",
         b"d/" * 1100 + b"past-the-lds-head.txt", b'"' * 1030]


@pytest.mark.parametrize("name", NAMES, ids=lambda n: "name%d" % len(n))
def test_file_names(gpu_ctx, name):
    import dgrep

    ctx = gpu_ctx
    ctx.load(b"")
    # short and long values, plain and escaped, so that the per-thread writer takes every branch
    data = (WC.lines(3000, 31) + b'a "long" \xe2\x80\xa8 value ' + b'<"\xff>' * 100 + b"\n" + b"p" * 700 + b"\n" +
            WC.lines(6000, 32) + b'the last "line" \xf0\x9f\x98')
    pieces = WC.pieces_of(data, WC.random_cuts("names", len(data), 3))
    match = O.Regexp(b"").match
    longest = max(len(v) for v in data.split(b"\n") if b'"' in v)
    assert 256 <= longest < 1024
    try:
        for lv in (256, 1 << 30, 0):  # the chunked path, the one-lane path, the default
            ctx.set_long_value(lv)
            for R in (1, 10):
                model = PC.windowed_partitions(pieces, 4096, match, name, R)
                _, stats = _check(ctx, "names", name, data, pieces, 4096, R, model=model)
                assert stats["long_values"] == (1 if longest >= (lv or dgrep.LONG_VALUE_DEFAULT) else 0), stats
    finally:
        ctx.set_long_value(0)
    if len(name) > 2048:
        assert len(O.json_kv(name, b"")) > 2048 + 30  # the escaped head is past the line writer's LDS copy


# ---- 4. the long path ---------------------------------------------------------------
SEQS = [b"\xe2\x80\xa8", b"\xf0\x9f\x98\x80", b"\xed\xa0\x80", b"\xc0\x80", b"\xf0\x9f\x98"]
_NO_NL = bytes(b for b in range(256) if b != 0x0A)


def _long_values(L):
    """the values of one length. A sequence padded to 4
    bytes and repeated, at shifts 0..3, straddles EVERY 4-byte boundary at every
    phase -- so every 16-, 256-, 1024-byte and chunk boundary too, wherever the
    value starts in its window."""
    out = []
    for off in range(16):  # every byte value in turn, at every offset within a 16-byte block
        out.append((b"a" * off + _NO_NL * (L // 255 + 1))[:L])
    for seq in SEQS:
        unit = seq + b"a" * (4 - len(seq))
        for shift in range(4):
            out.append((b"a" * shift + unit * (L // 4 + 1))[:L])
        out.append(b"a" * (L - len(seq)) + seq)  # at the value's very end
        out.append(seq + b"a" * (L - len(seq)))  # at its very start
    out += [b'"' * L, b"\xff" * L, b"a" * L]
    assert all(len(v) == L and b"\n" not in v for v in out)
    return out


def _needs_escape(v):
    return any(b < 0x20 or b >= 0x80 or b in b'"\\<>&' for b in v)


def _long_lengths():
    import dgrep

    return [255, 256, 257, 4095, 4096, 4097, 3 * dgrep.LONG_CHUNK + 1]


@pytest.mark.parametrize("which", range(7), ids=["255", "256", "257", "4095", "4096", "4097", "3chunks+1"])
def test_long_values(gpu_ctx, which):
    ctx = gpu_ctx
    L = _long_lengths()[which]
    values = _long_values(L)
    data = b"short first line\n" + b"\n".join(values) + b"\nlast"
    planted = sum(1 for v in values if len(v) >= 256 and _needs_escape(v))
    assert planted == (0 if L < 256 else len(values) - 1)
    ctx.load(b"")
    try:
        ctx.set_long_value(256)
        # a window that holds at least three of the lines, and the smallest one (a line per window from 4095 on)
        for W in (4096, max(4096, (4 * L + 4095) // 4096 * 4096)):
            key = "long/%d" % L
            want = _want(ctx, key, FILENAME, data, 10)
            calls, stats = _run(ctx, WC.pieces_of(data, WC.random_cuts(key, len(data), 2)), W, FILENAME, 10)
            assert PC.joined(calls, 10) == want, (L, W)
            assert stats["long_values"] == planted, (L, W, stats)
            assert ctx.map_partitions_windowed(FILENAME, data, 10, W) == want, (L, W)
    finally:
        ctx.set_long_value(0)
    if L == 255:  # the default threshold, and a split whose longest value lies below it
        import dgrep

        assert L < dgrep.LONG_VALUE_DEFAULT
        calls, stats = _run(ctx, [data], 8192, FILENAME, 10)
        assert PC.joined(calls, 10) == _want(ctx, "long/255", FILENAME, data, 10)
        assert stats["long_values"] == 0, stats


def test_long_values_against_the_oracle(gpu_ctx):
    """the reference above is the resident writer; once, for the shortest long length, the oracle as well"""
    values = _long_values(257)
    data = b"\n".join(values)
    gpu_ctx.load(b"")
    try:
        gpu_ctx.set_long_value(256)
        got = gpu_ctx.map_partitions_windowed(FILENAME, data, 3, 4096)
    finally:
        gpu_ctx.set_long_value(0)
    assert got == PC.whole_partitions(data, lambda line: True, FILENAME, 3)


@pytest.mark.parametrize("seq", [b"\xf0\x9f\x98", b"\xe2\x80", b"\xf4\x8f", b"\xdf"], ids=lambda s: s.hex())
def test_the_stream_ends_inside_a_sequence(gpu_ctx, seq):
    """The stream's last line ends in a truncated sequence, and what the window
    buffers hold behind it -- two earlier windows' bytes -- are continuation
    bytes that would complete it: `i + need <= L` is counted within the value."""
    W = 4096
    filler = b"\xbf" * (W - 1) + b"\n"
    last = b'"' + b"a" * 300 + seq
    data = filler + filler + b"x\n" + last
    gpu_ctx.load(b"")
    want = _want(gpu_ctx, "trunc/" + seq.hex(), FILENAME, data, 3)
    assert want == PC.whole_partitions(data, lambda line: True, FILENAME, 3)
    try:
        for lv in (256, 1 << 30):
            gpu_ctx.set_long_value(lv)
            for pieces in ([data], [filler, filler, b"x\n" + last], [data[:2 * W + 2], last]):
                calls, stats = _run(gpu_ctx, pieces, W, FILENAME, 3)
                assert PC.joined(calls, 3) == want, (lv, len(pieces))
                assert stats["long_values"] == (3 if lv == 256 else 0), stats
    finally:
        gpu_ctx.set_long_value(0)


# ---- 5. a line of 3.5 windows that needs escaping -----------------------------------
@pytest.mark.parametrize("W", WC.WINDOWS)
def test_long_escaped_line_grows_the_buffers(gpu_ctx, W):
    import dgrep

    data, n = WC.long_line(W, True)
    at = data.index(b"error" + b"abcdefghij"[:4])
    line = bytearray(data[at:at + n])
    line[9::10] = b'"' * len(line[9::10])
    data = data[:at] + bytes(line) + data[at + n:]
    assert data[at + n] == 0x0A and data[at - 1] == 0x0A and line.count(b'"') == n // 10
    gpu_ctx.load(b"error")
    key = "longline/%d" % W
    try:
        for lv in (0, 256):
            gpu_ctx.set_long_value(lv)
            for cuts in ([], WC.random_cuts(key, len(data), 6)):
                want, stats = _check(gpu_ctx, key, FILENAME, data, WC.pieces_of(data, cuts), W, 10)
                assert stats["max_carry"] >= n and stats["data_bytes"] >= n, stats
                assert stats["long_values"] == (1 if n >= (lv or dgrep.LONG_VALUE_DEFAULT) else 0), (lv, stats)
    finally:
        gpu_ctx.set_long_value(0)


# ---- 6. the footprint condition -------------------------------------------------------
def test_footprint_is_set_by_the_window(gpu_ctx):
    W, n = 8192, 2 << 20
    data = WC.lines(n, 24, longest=200)
    longest = max(map(len, data.split(b"\n")))
    assert 150 <= longest <= 200
    escaped_name = len(O.json_kv(FILENAME, b"")) - len(O.json_kv(b"", b""))
    # every byte widens to at most 6; every record (at least one byte of the window each) adds the fixed bytes,
    # the digits and the escaped filename
    enc_bound = 6 * (W + longest) + (W + longest + 1) * (36 + 20 + escaped_name)
    data_bound = 4 * (W + longest + 64)
    gpu_ctx.load(b"")
    seen = []

    def each(st):
        seen.append(st.stats())

    pieces = [data[o:o + 100 * 1000] for o in range(0, n, 100 * 1000)]
    calls, stats = _run(gpu_ctx, pieces, W, FILENAME, 10, each=each)
    assert PC.joined(calls, 10) == _want(gpu_ctx, "footprint", FILENAME, data, 10)
    seen.append(stats)
    assert max(s["enc_device_bytes"] for s in seen) <= enc_bound, (max(s["enc_device_bytes"] for s in seen), enc_bound)
    assert max(s["data_bytes"] for s in seen) <= data_bound, (max(s["data_bytes"] for s in seen), data_bound)
    assert stats["enc_device_bytes"] > 0 and stats["rows"] >= n // (W + longest), stats
    assert stats["encode_ms"] > 0 and stats["long_values"] == 0, stats


# ---- 7. composition ---------------------------------------------------------------------
def test_cells_feed_the_batch_reduce(gpu_ctx):
    data = WC.lines(60 * 1000, 26) + b"the last error"
    gpu_ctx.load(b"error")
    for R in (1, 7):
        job = gpu_ctx.grep_job([(FILENAME, data)], R)
        assert gpu_ctx.reduce_batch(gpu_ctx.map_partitions_windowed(FILENAME, data, R, 4096)) == job
        assert sum(map(len, job)) > 0


def test_map_partitions_stream_equals_map_partitions(gpu_ctx):
    import dgrep

    data = WC.lines(50 * 1000, 25) + b"\n\nthe last error"  # two empty lines for ^$
    pieces = WC.pieces_of(data, WC.random_cuts("mapstream", len(data), 7))
    old = dgrep.pattern
    try:
        for pat in ("error", "", "^$"):
            dgrep.set_pattern(pat)
            gpu_ctx.load(pat.encode())
            want = gpu_ctx.map_partitions("f.txt", data, 10)
            assert dgrep.MapPartitionsStream("f.txt", pieces, 10, window=4096) == want
            assert dgrep.MapPartitionsStream(b"f.txt", iter([data]), 10, window=8192) == want
            assert sum(map(len, want)) > 0
    finally:
        dgrep.set_pattern(old)


# ---- 8. everything else -------------------------------------------------------------------
def test_load_mid_stream_feed_after_finish_and_the_other_kind_of_stream(gpu_ctx):
    import ctypes

    import dgrep

    ctx = gpu_ctx
    ctx.load(b"error")
    one = O.json_kv(O.format_key(b"f", 1), b"an error")
    with ctx.partition_stream(4096, b"f", 1) as st:
        assert st.feed(b"an error\nand") == [[one]]
        ctx.load(b"and")
        with pytest.raises(dgrep.DgrepError) as e:
            st.feed(b" more\n")
        assert e.value.code == dgrep.DGREP_E_INVALID and "pattern" in str(e.value)
        with pytest.raises(dgrep.DgrepError) as e:
            st.finish()
        assert e.value.code == dgrep.DGREP_E_INVALID
    with ctx.partition_stream(4096, b"f", 2) as st:
        assert st.feed(b"") == [] and st.feed(b"x\nand y") == []
        rows = st.finish()
        assert len(rows) == 1 and b"".join(rows[0]) == O.json_kv(O.format_key(b"f", 2), b"and y")
        with pytest.raises(dgrep.DgrepError) as e:
            st.feed(b"z\n")
        assert e.value.code == dgrep.DGREP_E_INVALID and "finish" in str(e.value)
    # each kind of stream refuses the other kind's calls, names the mismatch and stays usable
    L = dgrep.lib()
    buf = ctypes.create_string_buffer(b"and\n", 4)
    with ctx.partition_stream(4096, b"f", 2) as st:
        r = dgrep._StreamResult()
        ctypes.memset(ctypes.byref(r), 0xAB, ctypes.sizeof(r))
        assert L.dgrep_stream_feed(st._h, buf, 4, ctypes.byref(r)) == dgrep.DGREP_E_INVALID
        assert bytes(r) == bytes(ctypes.sizeof(r)) and "partition stream" in ctx._err()
        assert L.dgrep_stream_finish(st._h, ctypes.byref(r)) == dgrep.DGREP_E_INVALID
        assert "partition stream" in ctx._err()
        assert len(st.feed(b"and\n")) == 1 and st.finish() == []
    with ctx.stream(4096) as st:
        r = dgrep._BatchPartitions()
        ctypes.memset(ctypes.byref(r), 0xAB, ctypes.sizeof(r))
        assert L.dgrep_stream_feed_partitions(st._h, buf, 4, ctypes.byref(r)) == dgrep.DGREP_E_INVALID
        assert bytes(r) == bytes(ctypes.sizeof(r)) and "record stream" in ctx._err()
        assert L.dgrep_stream_finish_partitions(st._h, ctypes.byref(r)) == dgrep.DGREP_E_INVALID
        assert "record stream" in ctx._err()
        assert st.feed(b"and\n")[0].tolist() == [1]
        assert st.stats()["windows"] == 1
    # the streams leave nothing behind: the resident writer right after is still exact
    assert ctx.map_partitions(b"f", b"x\nand y", 2) == PC.whole_partitions(b"x\nand y", O.Regexp(b"and").match, b"f", 2)
