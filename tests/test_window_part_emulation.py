"""The windowed partition writer's contract on the CPU (window_part_cases.py):
the model's rows, joined per partition, equal the writer's output on the whole
split for every cut and window; the cases reach every situation the GPU file
(test_gpu_window_part.py) relies on; and the local width rule, restated in
Python, agrees with the oracle's json.Encoder."""
import itertools
import random

import pytest

import oracle_lib as O
import window_cases as WC
import window_part_cases as PC

FILENAME = b"pg-\"quoted\".txt"


@pytest.mark.parametrize("pattern", [b"error", b"^$", b""])
@pytest.mark.parametrize("nreduce", [1, 10])
def test_rows_joined_equal_the_whole_split(pattern, nreduce):
    match = O.Regexp(pattern).match
    whole = {}
    for case in PC.CASES:
        if id(case.data) not in whole:
            whole[id(case.data)] = PC.whole_partitions(case.data, match, FILENAME, nreduce)
        calls = PC.windowed_partitions(WC.pieces_of(case.data, case.cuts), case.window, match, FILENAME, nreduce)
        assert len(calls) == len(case.cuts) + 2, case.name  # one per feed, and the finish
        assert all(len(row) == nreduce for rows in calls for row in rows), case.name
        assert PC.joined(calls, nreduce) == whole[id(case.data)], case.name
        # rows are the windows that completed a matching line: window_cases.windowed() saw the same records
        recs, _ = WC.windowed(WC.pieces_of(case.data, case.cuts), case.window, match)
        for rows, r in zip(calls, recs):
            assert sum(cell.count(b"\n") for row in rows for cell in row) == len(r), case.name


def test_the_cases_reach_what_the_gpu_file_needs():
    match = O.Regexp(b"error").match
    seen = set()
    for case in PC.CASES:
        calls = PC.windowed_partitions(WC.pieces_of(case.data, case.cuts), case.window, match, FILENAME, 10)
        recs, (windows, _) = WC.windowed(WC.pieces_of(case.data, case.cuts), case.window, match)
        rows = [row for rows in calls for row in rows]
        if any(b"" in row for row in rows):
            seen.add("a row with empty cells")
        if len(rows) < windows:
            seen.add("a window with no matching line, and so no row")
        seen.add("a finish that adds a row" if calls[-1] else "a finish that adds none")
        for lo, hi in ((9, 10), (99, 100), (999, 1000)):
            a, b = b"(line number #%d)" % lo, b"(line number #%d)" % hi
            for w, row in enumerate(rows):
                if w >= 1 and any(a in c for c in row) and any(b in c for c in row):
                    seen.add("%d -> %d inside a later window" % (lo, hi))
    assert seen == {"a row with empty cells", "a window with no matching line, and so no row",
                    "a finish that adds a row", "a finish that adds none", "9 -> 10 inside a later window",
                    "99 -> 100 inside a later window", "999 -> 1000 inside a later window"}, seen


def _check_widths(s):
    assert sum(PC.escape_width(s, i) for i in range(len(s))) == PC.go_escaped_len(s), s.hex()


def test_width_rule_all_strings_of_1_and_2_bytes():
    for a in range(256):
        _check_widths(bytes([a]))
        for b in range(256):
            _check_widths(bytes([a, b]))


@pytest.mark.parametrize("n", [3, 4])
def test_width_rule_edge_alphabet(n):
    for t in itertools.product(PC.EDGE_BYTES, repeat=n):
        _check_widths(bytes(t))


def test_width_rule_random_strings():
    rnd = random.Random(20261020)
    for _ in range(2000):
        n = rnd.randrange(65)
        _check_widths(bytes(rnd.choice(PC.EDGE_BYTES) if rnd.random() < 0.5 else rnd.randrange(256)
                            for _ in range(n)))
