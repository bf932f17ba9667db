"""The windowed scan's algebra, before a GPU is involved: for every case of
window_cases.CASES the pure-Python model (the cut at a window's last '\\n', the
running byte and line bases, the carried tail), run with the oracle's
regexp.Match as the per-line predicate, gives exactly the oracle's Map of the
concatenated pieces -- for every cut."""
import numpy as np
import pytest

import oracle_lib as O
import window_cases as WC

PATTERNS = [b"error", b"^$", b"", b"("]


def _flat(calls):
    return [r for call in calls for r in call]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_model_equals_oracle_map(pattern):
    rx = O.Regexp(pattern)
    seen = set()
    for case in WC.CASES:
        pieces = WC.pieces_of(case.data, case.cuts)
        calls, _ = WC.windowed(pieces, case.window, rx.match)
        assert len(calls) == len(pieces) + 1
        want = O.grep_map(pattern, case.data)
        got = _flat(calls)
        assert len(got) == len(want[0]), case.name
        for k in range(3):
            np.testing.assert_array_equal(np.array([r[k] for r in got], np.uint64), want[k], err_msg=case.name)
        seen.add(len(got) > 0)
    assert seen == ({False} if pattern == b"(" else {False, True} if pattern != b"" else {True})


def test_long_line_is_carried_whole():
    rx = O.Regexp(b"^[a-j ]*error[a-j ]*$")
    for W in WC.WINDOWS:
        for at_start in (True, False):
            data, n = WC.long_line(W, at_start)
            assert n == 7 * W // 2
            calls, (windows, max_carry) = WC.windowed([data], W, rx.match)
            want = O.grep_map(rx.pattern, data)
            got = _flat(calls)
            assert [r[1] for r in got] == want[1].tolist() and [r[2] for r in got] == want[2].tolist()
            assert n in want[2].tolist()  # the long line itself matches
            assert max_carry >= 2 * W     # it outgrew a window: the buffers had to grow


def test_cases_cover_the_shapes():
    names = {c.name.split("/")[0] for c in WC.CASES}
    assert {"nl_last", "nl_first", "line_is_window", "all_newlines", "no_newline", "ends_in_newline", "empty",
            "cut_in_match"} <= names
    assert any(len(c.cuts) == 299 for c in WC.CASES)                      # 300 one-byte feeds
    assert any(len(set(c.cuts)) < len(c.cuts) for c in WC.CASES)          # feeds of length 0
    assert max(len(c.data) for c in WC.CASES) <= 300 * 1000
