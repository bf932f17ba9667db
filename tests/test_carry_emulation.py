"""The bounded stream's state machine, before a GPU is involved: the
pure-Python model of carry_cases.bounded() -- the fold rule, the walk of the
carried line's last bytes, the splice, the finish -- run over a compiled
pattern's own tables, gives exactly the oracle's Map of the concatenated
pieces, for every cut, and never holds a window or more as the tail."""
import numpy as np
import pytest

import carry_cases as CC
import oracle_lib as O
import window_cases as WC

_want = {}


def _oracle(pattern, data):
    k = (bytes(pattern), data)
    if k not in _want:
        _want[k] = O.grep_map(pattern, data)
    return _want[k]


def _check(pattern, dfa, rx, name, window, data, cuts):
    pieces = WC.pieces_of(data, cuts)
    calls, info = CC.bounded(pieces, window, dfa, rx.match)
    assert len(calls) == len(pieces) + 1
    got, want = CC.flat(calls), _oracle(pattern, data)
    assert len(got) == len(want[0]), (name, len(got), len(want[0]))
    for k in range(3):
        np.testing.assert_array_equal(np.array([r[k] for r in got], np.uint64), want[k], err_msg=name)
    return got, info


@pytest.mark.parametrize("pattern", CC.PATTERNS, ids=lambda p: p.decode("utf-8") or "empty")
def test_model_equals_oracle_map(pattern):
    import dgrep

    dfa, rx = CC.Dfa(dgrep.CompiledPattern(pattern)), O.Regexp(pattern)
    seen, folds = set(), 0
    for case in WC.CASES:
        got, info = _check(pattern, dfa, rx, case.name, case.window, case.data, case.cuts)
        seen.add(len(got) > 0)
        folds += info["folds"]
        if info["folds"] == 0:  # nothing outgrew the window: the calls are those of the plain windowed model
            assert CC.bounded(WC.pieces_of(case.data, case.cuts), case.window, dfa, rx.match)[0] == \
                WC.windowed(WC.pieces_of(case.data, case.cuts), case.window, rx.match)[0], case.name
    for case in CC.LONG:
        got, info = _check(pattern, dfa, rx, case.name, case.window, case.data, case.cuts)
        assert info["folds"] >= 1 and info["max_carry"] >= case.longest, (case.name, info)
        folds += info["folds"]
        seen.add(len(got) > 0)
    for W in WC.WINDOWS:
        for seed in range(3):
            data, _ = CC.memory_line(W, seed, nwin=5)
            got, _ = _check(pattern, dfa, rx, "memory/%d/w%d" % (seed, W), W, data,
                            WC.random_cuts("memory", len(data), 3))
            seen.add(len(got) > 0)
        got, _ = _check(pattern, dfa, rx, "greek/w%d" % W, W, CC.greek_line(W), [])
        seen.add(len(got) > 0)
    assert folds > 0 and True in seen


def test_long_line_verdicts_follow_the_line():
    """the long cases decide what they were built to decide"""
    import dgrep

    dfa, rx = CC.Dfa(dgrep.CompiledPattern(CC.SHENG8)), O.Regexp(CC.SHENG8)
    lens = {}
    for case in CC.LONG:
        if case.pattern != CC.SHENG8:
            continue
        got, _ = _check(CC.SHENG8, dfa, rx, case.name, case.window, case.data, case.cuts)
        lens[case.name] = [r[2] for r in got]
    for W in WC.WINDOWS:
        assert 7 * W // 2 in lens["hit_first/whole/w%d" % W] and 7 * W // 2 in lens["hit_last/random/w%d" % W]
        assert 13 * W // 2 in lens["hit_middle/whole/w%d" % W]
        assert max(lens["miss_middle/whole/w%d" % W]) < W
        b2b = lens["back_to_back/random/w%d" % W]
        assert 5 * W // 2 + 5 in b2b and 9 * W // 4 + 5 in b2b and 13 * W // 4 not in b2b
        assert lens["ends_exact/whole/w%d" % W] == [2 * W]


def test_even_k_and_greek_decide_by_the_whole_line():
    import dgrep

    for W in WC.WINDOWS:
        dfa, rx = CC.Dfa(dgrep.CompiledPattern(CC.EVEN_K)), O.Regexp(CC.EVEN_K)
        for seed in range(4):
            data, nk = CC.memory_line(W, seed, nwin=5)
            got, info = _check(CC.EVEN_K, dfa, rx, "even", W, data, [])
            assert info["folds"] >= 4
            assert (max(r[2] for r in got) > 5 * W) == (nk % 2 == 0), (seed, nk)
        dfa, rx = CC.Dfa(dgrep.CompiledPattern(CC.GREEK)), O.Regexp(CC.GREEK)
        got, info = _check(CC.GREEK, dfa, rx, "greek", W, CC.greek_line(W), [])
        assert info["folds"] >= 6 and [r[0] for r in got] == [2, 5]


def test_invariant_holds_for_every_feed_pattern():
    """one-byte feeds of a newline-free stream: the tail never reaches a window (bounded() asserts it)"""
    import dgrep

    dfa, rx = CC.Dfa(dgrep.CompiledPattern(b"error")), O.Regexp(b"error")
    data = b"abc " * 2100 + b"error"
    for W in WC.WINDOWS:
        calls, info = CC.bounded([data[i:i + 1] for i in range(len(data))], W, dfa, rx.match)
        assert CC.flat(calls) == [(1, 0, len(data))] and info["folds"] == len(data) // W
