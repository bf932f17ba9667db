"""The random-pattern cases (tests/random_pattern_cases.py) on the CPU: the
quotas are full, corpus B holds the tile edges and the long lines it is about,
the long lines get both verdicts, the split cuts fall where they should, and
the compiled DFA and the forced-partial NFA program -- interpreted in Python --
agree with the oracle. A failure of tests/test_gpu_random_patterns.py then
points at a loader image or a kernel, not at the compiler, the oracle or an
input."""
import numpy as np
import pytest

import dfa_runner
import dgrep
import nfa_runner
import oracle_lib as O
import random_pattern_cases as R
import stepper_cells as SC


def _mixed(case):
    hit, miss = R.long_verdicts(case.pattern)
    return hit >= 3 and miss >= 3


def test_quotas_are_full_and_the_patterns_distinct():
    sel = R.selected()
    assert R.selection_draws() < R.DRAW_CAP
    assert len({c.pattern for c in sel}) == len(sel) == R.QUOTA * len(R.BUCKETS)
    assert len({c.name for c in sel}) == len(sel)
    for name, lo, hi in R.BUCKETS:
        mine = [c for c in sel if c.bucket == name]
        assert len(mine) == R.QUOTA, name
        assert all(lo <= c.nstates <= hi for c in mine), name
    for c in sel:
        cp = R.compiled(c.pattern)
        assert (cp.nstates, cp.nclasses) == (c.nstates, c.nclasses)
        assert not cp.flags & (dgrep.DFA_MATCH_ALL | dgrep.DFA_MATCH_NONE | dgrep.DFA_GO_SYNTAX_ERROR | dgrep.DFA_PARTIAL)
        assert O.compile_status(c.pattern) == O.ORC_OK
        n = len(R.want(c.pattern, "A")[0])
        assert 0 < n < R.corpus_a().count(b"\n") + 1, c
    assert {c.name for c in R.regressions()} == set(R.REGRESSIONS)
    print("selected %d patterns in %d draws; states %s; classes up to %d" % (
        len(sel), R.selection_draws(), sorted(c.nstates for c in sel)[::8], max(c.nclasses for c in sel)))


def test_selection_varies_the_structure():
    """What the hand-written patterns vary little: an empty line that matches
    (start's '\\n' leads to start_m), accepting states that do not absorb, and
    class maps of 60 classes and more. Some of each, no more is claimed."""
    empty_matches = moving_accept = wide = 0
    for c in R.selected():
        cp = R.compiled(c.pattern)
        bc, tr = cp.tables()
        cn = int(bc[10])
        assert set(tr[:, cn].tolist()) <= {cp.start, cp.start_m}, c  # the blob's contract
        empty_matches += int(tr[cp.start, cn]) == cp.start_m
        # accepting: '\n' leads to start_m; absorbing: every other class loops
        acc = [s for s in range(cp.nstates) if tr[s, cn] == cp.start_m]
        moving_accept += any(any(tr[s, k] != s for k in range(cp.nclasses) if k != cn) for s in acc)
        wide += c.nclasses >= 60
        assert cp.start != cp.start_m, c
    print("of %d: %d match the empty line, %d have a non-absorbing accepting state, %d have 60 classes or more" % (
        len(R.selected()), empty_matches, moving_accept, wide))
    assert empty_matches and moving_accept and wide


def test_corpus_a_shape():
    a = R.corpus_a()
    assert 48 << 10 <= len(a) < 50 << 10 and not a.endswith(b"\n")
    for tok in (b"\r", b"\xe2\x82\n", b"\xff", b"error", b"\n\n"):
        assert tok in a, tok
    assert R.corpus_a() is a


@pytest.mark.parametrize("stepper", R.STEPPERS, ids=lambda s: s.name)
def test_corpus_b_holds_tile_edges_and_straddling_long_lines(stepper):
    data, longs = R.corpus_b()
    tile = SC.tile_bytes(SC.geometry(stepper))
    assert tile == R.tiles()[stepper.name]
    assert len(data) < R.B_MAX and not data.endswith(b"\n")
    assert (len(data) - 1) // tile >= 2, (stepper.name, len(data), tile)  # two tile edges inside B
    across = R.straddled(tile)
    assert len({sl for v in across.values() for sl in v}) >= 2, across
    assert sum(1 for v in across.values() if v) >= 2, across


def test_corpus_b_long_lines():
    data, longs = R.corpus_b()
    assert len(longs) == 4 * len(R.LONG_TOKENS)
    lines = set(R._lines_of(data))
    for s, l in longs:
        assert (s, l) in lines and l >= 6000, (s, l)
    # every token at every placement; every length near 6, 20 and 70 KiB
    for tok in R.LONG_TOKENS:
        mine = [data[s:s + l] for s, l in longs if data[s:s + l].count(tok) * len(tok) >= l - 40]
        assert len(mine) >= 4, tok
    for n in R.LONG_LENGTHS:
        assert sum(1 for _, l in longs if n - 2 <= l <= n + 40) >= 8, n
    # the short lines between them are not long enough to be parked anywhere
    assert max(l for sl in lines - set(longs) for l in [sl[1]]) < 200


def test_long_lines_get_both_verdicts():
    sel = R.selected()
    mixed = [c for c in sel if _mixed(c)]
    per = {name: sum(1 for c in mixed if c.bucket == name) for name, _, _ in R.BUCKETS}
    print("patterns with 3 or more matching and 3 or more non-matching long lines: %d of %d, per bucket %r" % (
        len(mixed), len(sel), per))
    assert 2 * len(mixed) >= len(sel)
    assert min(per.values()) >= 5, per


def test_split_cuts():
    a = R.corpus_a()
    parts = R.splits_of(a)
    assert b"".join(parts[:-1]) == a and len(parts[-1]) == 1
    assert parts.count(b"") == 1 and len(parts) == 12
    cuts = R.split_cuts(a)
    assert len(cuts) == 9
    in_line = [c for c in cuts if a[c - 1] != 0x0A and a[c] != 0x0A]
    # inside a multi-byte sequence: a lead byte before, a continuation byte after
    in_rune = [c for c in cuts if a[c - 1] >= 0xC2 and a[c] & 0xC0 == 0x80]
    assert in_line and in_rune, cuts


def _eq(got, want, msg):
    assert len(got[0]) == len(want[0]), (msg, len(got[0]), len(want[0]))
    for g, w in zip(got, want):
        np.testing.assert_array_equal(np.asarray(g, np.uint64), w, err_msg=repr(msg))


@pytest.mark.parametrize("bucket", [b[0] for b in R.BUCKETS])
def test_interpreted_dfa_and_nfa_program_agree_with_the_oracle(bucket):
    data = R.slice_a()
    reached = total = 0
    for c in (c for c in R.selected() if c.bucket == bucket):
        want = R.want(c.pattern, "A4K")
        _eq(dfa_runner.run_blob(R.compiled(c.pattern), data), want, (c.pattern, "run_blob"))
        cp = R.compiled(c.pattern, R.PARTIAL_BUDGET)
        assert cp.partial, c
        _eq(nfa_runner.run_partial(cp, data), want, (c.pattern, "run_partial"))
        assert R.compiled(c.pattern, 12).partial, c
        cand, direct = R.partial_counts(cp, data)
        # the vectorised count is the interpreter's: the lines it hands to the program
        bc, tr = cp.tables()
        slow = 0
        for line in data.split(b"\n"):
            s = cp.start
            for b in line:
                s = int(tr[s, bc[b]])
                if s == cp.nstates - 1:
                    slow += 1
                    break
        assert cand == slow, c
        reached += cand
        total += data.count(b"\n") + 1
    print("%s: at state budget %d the NFA program decides %d of %d lines" % (bucket, R.PARTIAL_BUDGET, reached, total))
    assert reached > 0
