"""The Sheng stepper's per-word path (scan_dfa.hip: StepSheng8, run_block,
word_events, word_emit, the lnl line-start encoding) against the CPU oracle.

Every pattern here compiles to at most 8 DFA states, so the Sheng stepper
runs; every input is built by hand for one shape of the word path -- where in
a word, a word pair or a 128-byte block a matching line's '\\n' falls, how
many '\\n' share a word, where the line started -- and each test first checks
on the oracle's output that the input really holds the events it is about,
so a slip in a generator cannot turn a case into a no-op. Each case runs at
the default lane chunk (4 KiB at these sizes) and at 4224 B (33 blocks: an
odd block count, chunk edges that are no power of two).
"""
import random
import zlib

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

CHUNKS = [0, 4224]
DEFAULT_CHUNK = 4096


@pytest.fixture
def sheng_ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_lane_chunk(0)


def _chunk_bytes(chunk):
    return chunk or DEFAULT_CHUNK


def _ends(rec):
    """Positions of the terminating '\\n' (or the split's end) of the records."""
    return set((rec[1] + rec[2]).tolist())


def _records(rec):
    return set(zip(rec[1].tolist(), rec[2].tolist()))


def _scan_check(ctx, pattern, data, chunk):
    """ctx.scan(data) bit-exact against the oracle, on the Sheng stepper at the
    asked chunk; returns the oracle's records."""
    cp = ctx.load(pattern)
    assert cp.nstates <= 8, (pattern, cp.nstates)
    ctx.set_lane_chunk(chunk)
    got = ctx.scan(data)
    want = O.grep_map(pattern, data)
    assert len(got[0]) == len(want[0]), (pattern, chunk, len(got[0]), len(want[0]))
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    st = ctx.scan_stats()
    assert st["stepper"] == "sheng", st
    assert st["lane_chunk"] == _chunk_bytes(chunk), st
    return want


# ---- 1. where in a word pair the event falls --------------------------------
def placement_input(plant):
    """'x' filler (no '\\n', no match) with `plant` ending on byte offset o of a
    16-byte window, o = 0..15; the windows step through the 128-byte block."""
    n = 272 * 17 + 64
    d = bytearray(b"x" * n)
    last = []
    for o in range(16):
        q = 272 * (o + 1) + o
        assert q % 16 == o
        d[q - len(plant) + 1:q + 1] = plant
        last.append(q)
    return bytes(d), last


PLACEMENT = [
    # plant, pattern, event positions relative to the plant's last byte
    (b"error\n", b"error", (0,)),
    (b"error\n", b"", (0,)),
    (b"error\n", b"^$", ()),
    (b"error\n\n", b"error", (-1,)),
    (b"error\n\n", b"", (-1, 0)),
    (b"error\n\n", b"^$", (0,)),
]


@pytest.mark.parametrize("chunk", CHUNKS)
def test_event_at_every_byte_of_a_word_pair(sheng_ctx, chunk):
    for plant, pattern, rel in PLACEMENT:
        data, last = placement_input(plant)
        want = _scan_check(sheng_ctx, pattern, data, chunk)
        ends = _ends(want)
        expect = {q + r for q in last for r in rel}
        assert expect <= ends, (plant, pattern)
        if rel:
            assert {e % 16 for e in expect} == set(range(16)), (plant, pattern)
            assert len(ends - {len(data)}) == len(expect), (plant, pattern)
        else:
            assert not ends, (plant, pattern)


def two_events_input():
    """For each (i, j): a line of 'e' ending at byte i of an even word and a
    second one ending at byte j of the next word, 16 cases."""
    d = bytearray(b"x" * (40 * 18))
    pairs = []
    for i in range(4):
        for j in range(4):
            p = 40 * (4 * i + j + 1)
            assert p % 8 == 0
            d[p + i - 4] = 0x0A
            d[p + i - 3:p + i] = b"eee"
            d[p + i] = 0x0A
            d[p + i + 1:p + 4 + j] = b"e" * (3 + j - i)
            d[p + 4 + j] = 0x0A
            pairs.append((p + i, p + 4 + j))
    return bytes(d), pairs


@pytest.mark.parametrize("chunk", CHUNKS)
def test_two_events_in_one_word_pair(sheng_ctx, chunk):
    data, pairs = two_events_input()
    for pattern in (b"^e*$", b"", b"e"):
        want = _scan_check(sheng_ctx, pattern, data, chunk)
        ends = _ends(want)
        for a, b in pairs:
            assert a in ends, (pattern, a)
            # (the second line is empty when the two '\n' are adjacent)
            assert b in ends or (pattern == b"e" and b == a + 1), (pattern, a, b)
        if pattern == b"^e*$":
            assert len(want[0]) == 32
    assert {(a % 4, b % 4) for a, b in pairs} == {(i, j) for i in range(4) for j in range(4)}
    assert all(a // 8 == b // 8 and a // 4 + 1 == b // 4 for a, b in pairs)


# ---- 2. several '\n' per word, pairs of nothing but '\n' -------------------
def newline_runs_input():
    d = bytearray(b"x" * (48 * 66))
    runs = []
    idx = 0
    for n in range(2, 10):
        for a in range(8):
            idx += 1
            base = 48 * idx + a
            d[base:base + n] = b"\n" * n
            runs.append((base, n))
    return bytes(d), runs


@pytest.mark.parametrize("chunk", CHUNKS)
def test_newline_runs_at_every_alignment(sheng_ctx, chunk):
    data, runs = newline_runs_input()
    assert {(b % 8, n) for b, n in runs} == {(a, n) for a in range(8) for n in range(2, 10)}
    for pattern in (b"^$", b""):
        want = _scan_check(sheng_ctx, pattern, data, chunk)
        ends = _ends(want)
        first = 1 if pattern == b"^$" else 0  # the run's first '\n' ends the 'x' line before it
        expect = {base + k for base, n in runs for k in range(first, n)}
        assert expect <= ends, pattern
        assert len(ends - {len(data)}) == len(expect), pattern


# ---- 3. short lines ---------------------------------------------------------
def short_lines_input():
    rnd = random.Random(zlib.crc32(b"sheng short lines"))
    out = bytearray()
    while len(out) < (64 << 10):
        out += bytes(rnd.choice(b"erox") for _ in range(rnd.randint(0, 9))) + b"\n"
    return bytes(out[:64 << 10])


@pytest.mark.parametrize("chunk", CHUNKS)
def test_short_random_lines(sheng_ctx, chunk):
    data = short_lines_input()
    for pattern in (b"error", b"e", b"o$", b""):
        want = _scan_check(sheng_ctx, pattern, data, chunk)
        assert len(want[0]) > 0, pattern
        if pattern == b"":
            assert len(want[0]) == data.count(b"\n") + 1


# ---- 4. block and chunk edges ----------------------------------------------
def block_edge_input():
    """'error\\n' ending in word 31 of a block, then a line of j 'e' ending in
    word 0 of the next block."""
    d = bytearray(b"x" * (128 * 10))
    ev = []
    for k in range(1, 9):
        j = (k - 1) % 4
        d[128 * k - 6:128 * k] = b"error\n"
        d[128 * k:128 * k + j] = b"e" * j
        d[128 * k + j] = 0x0A
        ev.append((128 * k - 1, 128 * k + j))
    return bytes(d), ev


@pytest.mark.parametrize("chunk", CHUNKS)
def test_events_across_a_block_edge(sheng_ctx, chunk):
    data, ev = block_edge_input()
    for pattern in (b"", b"e", b"error"):
        ends = _ends(_scan_check(sheng_ctx, pattern, data, chunk))
        for a, b in ev:
            assert a in ends, (pattern, a)
            if pattern == b"" or (pattern == b"e" and b % 128):
                assert b in ends, (pattern, b)
    assert {b % 128 for _, b in ev} == {0, 1, 2, 3}


def chunk_edge_input():
    """For both chunk sizes C and lanes k = 1..8: a line of 'e' that starts in
    the last word of lane k - 1's chunk (at k C - 1) and ends on byte k - 1 of
    the first word pair past it."""
    n = 9 * 4224 + 100
    d = bytearray((b"x" * 60 + b"\n") * (n // 61 + 1))[:n]
    ev = []
    for C in (DEFAULT_CHUNK, 4224):
        for k in range(1, 9):
            e = k - 1
            d[k * C - 16:k * C + 16] = b"x" * 32
            d[k * C - 2] = 0x0A
            d[k * C - 1:k * C + e] = b"e" * (e + 1)
            d[k * C + e] = 0x0A
            ev.append((k * C - 1, e + 1))
    return bytes(d), ev


@pytest.mark.parametrize("chunk", CHUNKS)
def test_line_from_last_word_of_chunk_into_first_pair_past_it(sheng_ctx, chunk):
    data, ev = chunk_edge_input()
    for pattern in (b"^e+$", b"e", b""):
        want = _scan_check(sheng_ctx, pattern, data, chunk)
        assert set(ev) <= _records(want), pattern
        if pattern == b"^e+$":
            assert len(want[0]) == len(ev)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_unterminated_last_line_and_split_sizes(sheng_ctx, chunk):
    import dgrep

    data = b"ok\n" * 50 + b"x" * 77 + b"\nthe last error"
    want = _scan_check(sheng_ctx, b"error", data, chunk)
    assert _records(want) == {(len(data) - 14, 14)}
    base = dgrep.synth_corpus_host(64 * 4224 + 1, 5, 0)
    for size in (4224 - 1, 4224 + 1, 64 * 4224 - 1, 64 * 4224 + 1):
        for pattern in (b"error", b""):
            want = _scan_check(sheng_ctx, pattern, base[:size], chunk)
            if pattern == b"":
                assert size in _ends(want)  # the last line, closed by the split's end


# ---- 5. where the matching line started -------------------------------------
def line_start_cases(C):
    """(name, pattern, data, (start, len)) with the matching line's start in the
    same word as its '\\n', the same word pair, an earlier word of the block,
    an earlier block, before the chunk (the lane before owns it), and at the
    split's first byte (lane 0 owns it without having seen a '\\n'); the first
    four once in lane 0's chunk and once in lane 1's."""
    cases = []
    for off in (0, C):
        pre = b"y" * (off - 1) + b"\n" if off else b""
        x = lambda n: b"x" * n
        cases += [
            ("same word @%d" % off, b"e", pre + x(63) + b"\n" + b"\ne\nx" + x(60), (off + 65, 1)),
            ("same pair @%d" % off, b"e", pre + x(66) + b"\neee\n" + x(57), (off + 67, 3)),
            ("earlier word @%d" % off, b"error", pre + x(130) + b"\n" + x(34) + b"error\n" + x(50), (off + 131, 39)),
            ("earlier block @%d" % off, b"error", pre + x(130) + b"\n" + x(295) + b"error\n" + x(50), (off + 131, 300)),
        ]
    cases += [
        ("before the chunk, not owned", b"error", b"x" * (C - 100) + b"\n" + b"x" * 144 + b"error\n" + b"x" * 300,
         (C - 99, 149)),
        ("split start, owned", b"error", b"x" * 200 + b"error\n" + b"x" * 100, (0, 205)),
        ("split start, owned, in the first word", b"e", b"e\n" + b"x" * 100, (0, 1)),
    ]
    return cases


@pytest.mark.parametrize("chunk", CHUNKS)
def test_line_start_encoding(sheng_ctx, chunk):
    for name, pattern, data, rec in line_start_cases(_chunk_bytes(chunk)):
        want = _scan_check(sheng_ctx, pattern, data, chunk)
        assert _records(want) == {rec}, (name, _records(want))
