"""GPU parity for over-budget patterns whose NFA program has more than 1024
rune-set positions (more than 32 position words): verify_nfa_wave_kernel gives
each candidate line to one wave, word j of the position set in lane j & 63,
slot j >> 6 (1, 2 or 4 slots). Compared bit-exactly with the oracle
(grep.go:17-29 restated) through the C ABI, at the sizes where the word-to-lane
layout changes, with closure contexts and multi-byte runes, with every line a
candidate, and on the route narrower programs keep."""
import random

import pytest

from nfa_wide_cases import (CJK, E_ACUTE, LETTER_PATTERN, N_RULES, RULES_POSITIONS, WORD_PATTERN, WORD_POSITIONS,
                            ab_lines, ab_pattern, rule, rule_set)
from test_gpu_parity import _check
from test_gpu_partial import _ab_lines

pytestmark = pytest.mark.gpu


def _load(ctx, pattern, budget, npos=None):
    import dgrep

    cp = ctx.load(dgrep.CompiledPattern(pattern, state_budget=budget))
    assert cp.partial, cp.flags
    if npos is not None:
        assert cp.nfa_positions == npos
    return cp


# nw = 33 (the first wide program), 64 | 65 (slot 1 begins with one word),
# 128 | 129 (slots 2 and 3 begin), 256 (every slot full)
@pytest.mark.parametrize("npos", [1025, 2048, 2049, 4096, 4097, 8192])
def test_slot_and_word_edges(gpu_ctx, npos):
    cp = _load(gpu_ctx, ab_pattern(npos), 64, npos)
    hit, miss = ab_lines(npos)
    rnd = random.Random(npos)
    data = b"\n".join([_ab_lines(rnd, 3000), hit, miss, b"x" + hit, b"\xff" + hit, b"", miss + b"c" + hit[:-1], hit,
                       b"b" * 7 + hit])  # the last line has no '\n'
    n = _check(gpu_ctx, cp, data, threads=16)
    assert gpu_ctx.scan_stats()["stepper"] == "filter"
    assert n == 5, n


@pytest.mark.parametrize("pattern,npos", [(WORD_PATTERN, WORD_POSITIONS), (LETTER_PATTERN, 1042)],
                         ids=["word-boundary", "letters"])
def test_contexts_and_multibyte_runes(gpu_ctx, pattern, npos):
    cp = _load(gpu_ctx, pattern, 64, npos)
    t = 1060
    rnd = random.Random(npos)
    lines = [
        # \bx[ab]*a[ab]{1060}: \b holds at the line start and after ' ', not after 'z'
        b"xa" + b"b" * t, b"xa" + b"b" * (t - 1), b"zxa" + b"b" * t, b"z xb" + b"ab" * (t // 2 + 3),
        b"\xffxa" + b"b" * t, b"_xa" + b"b" * t, E_ACUTE + b"xa" + b"b" * t,
        # x\pL{1040}y: two- and three-byte letters, truncated sequences, invalid bytes
        b"x" + E_ACUTE * 1040 + b"y", b"x" + CJK * 1040 + b"y", b"x" + E_ACUTE * 1039 + b"y",
        b"x" + CJK * 1041 + b"y", b"x" + E_ACUTE * 500 + b"\xe2\x82" + E_ACUTE * 539 + b"y",
        b"x" + CJK * 1040 + b"y\xe2\x82", b"x" + CJK * 1039 + b"\xe2\x82", b"x" + b"\xff" * 1040 + b"y",
        b"qx" + b"k" * 520 + E_ACUTE * 260 + CJK * 260 + b"yq", b"",
    ]
    rnd.shuffle(lines)
    data = _ab_lines(rnd, 2000) + b"\n" + b"\n".join(lines)
    n = _check(gpu_ctx, cp, data, threads=16)
    assert gpu_ctx.scan_stats()["stepper"] == "filter"
    assert n >= 4, n


def test_every_line_a_candidate(gpu_ctx):
    """State budget 3: the filter keeps no state, so the wave decides every
    line (empty split, no trailing '\\n', invalid UTF-8, lines across chunk and
    tile edges)."""
    import dgrep

    cp = _load(gpu_ctx, ab_pattern(1025), 3, 1025)
    hit, miss = ab_lines(1025)
    rnd = random.Random(1025)
    alpha = [b"a", b"e", b"r", b"o", b"x", b"k", b" ", b"_", b"1", b"-", b"\n", b"\n", b"\xe2\x82\xac", b"\xff",
             b"WARN", b"ERROR", b"error", b"2024-01", b"key ", b"\xe2\x82"]
    for size in (0, 1, 777, 70000):
        data = b"".join(rnd.choice(alpha) for _ in range(size // 3 + 1))[:size]
        _check(gpu_ctx, cp, data)
    data = bytearray(dgrep.synth_corpus_host(3 << 20, 9, 0))
    for at in (5000, 65000, 262100, 1 << 20, (3 << 20) - 1100):  # matching lines, two of them across an edge below
        data[at:at + len(hit) + 2] = b"\n" + hit + b"\n"
    data[2 << 20:(2 << 20) + len(miss) + 2] = b"\n" + miss + b"\n"
    for edge in (4095, 4096, 65535, 65536, 262143, 262144):
        data[edge] = 0x0A
    n = _check(gpu_ctx, cp, bytes(data), threads=16)
    assert n >= 3, n


def test_a_long_candidate(gpu_ctx):
    """Lines over the tile loop's own wave threshold (16 KiB) take the same
    route as short ones."""
    cp = _load(gpu_ctx, ab_pattern(1025), 64, 1025)
    rnd = random.Random(40000)
    never = (b"ab" * 250 + b"c") * 80  # 40,080 bytes, no run of 1024 [ab]
    data = b"\n".join([_ab_lines(rnd, 500), b"ab" * 20000, never, b"ba" * 300, never[:-1] + b"b" * 1100, b"ab" * 5])
    assert _check(gpu_ctx, cp, data, threads=16) == 2


def test_rule_set_at_the_default_budget(gpu_ctx):
    """120 `kwNNNa.*tailNNNb` rules over a log corpus: 50 planted matches and 50
    near misses (rule i's prefix, rule j's tail)."""
    import dgrep

    cp = _load(gpu_ctx, rule_set(), 0, RULES_POSITIONS)
    assert cp.nstates == 65535
    rnd = random.Random(120)
    lines = dgrep.synth_corpus_host(4 << 20, 11, 0).split(b"\n")
    for k in range(100):
        i = rnd.randrange(N_RULES)
        j = i if k < 50 else (i + 1 + rnd.randrange(N_RULES - 1)) % N_RULES
        at = rnd.randrange(len(lines))
        lines[at] = lines[at][:rnd.randrange(30)] + rule(i, j) + lines[at][-rnd.randrange(1, 30):]
    n = _check(gpu_ctx, cp, b"\n".join(lines), threads=16)
    assert gpu_ctx.scan_stats()["stepper"] == "filter"
    assert 45 <= n <= 50, n  # two plants may fall on one line


@pytest.mark.parametrize("pattern,npos", [(b"[ab]*a[ab]{300}", 302), (ab_pattern(1024), 1024)], ids=["302", "1024"])
def test_lane_per_line_route_unchanged(gpu_ctx, pattern, npos):
    """nw <= 32: verify_nfa_kernel<32>, as before the wave kernel."""
    cp = _load(gpu_ctx, pattern, 64, npos)
    hit, miss = ab_lines(npos)
    rnd = random.Random(npos)
    data = b"\n".join([_ab_lines(rnd, 3000), hit, miss, b"x" + hit, b"\xff" + hit, b"", hit])
    assert _check(gpu_ctx, cp, data, threads=16) == 4
