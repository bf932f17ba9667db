"""CPU model of how the filter stepper's parked lines are decided on the whole
DFA (long_dfa_seg1_kernel / long_dfa_fix_kernel in csrc/kernels/scan_dfa.hip,
the seeds of long_seeds in csrc/runtime/pattern_image.h and the segment cut of
resolve_long_filter in csrc/runtime/dgrep_runtime.hip).

A parked line is cut into 16 KiB segments. Each segment but the first is run
from up to 4 GUESSED entry states: 8 seed states (start, then states spread
over the LDS-resident breadth-first ids) step the first 64 bytes of the 256
bytes before the segment together, the distinct non-absorbing survivors (at
most 4, in seed order) step the rest. The fix kernel then walks the line's
segments from the true state: a segment whose guesses hold that state is
taken whole, any other is re-run serially -- the branch that keeps the result
exact for every DFA, and that a keyword automaton never reaches. The model
restates the seeds, the guesses and the walk, and counts the segments walked
and those re-run (dgrep_scan_stats long_segments, long_guess_misses); the GPU
test (tests/test_gpu_long_guess.py) requires the kernels' counts to be equal.

Here: the model's verdicts against the oracle, and the fixtures' purpose --
the cases meant to reach the re-run do, the others never do."""
import functools

import numpy as np
import pytest

import dgrep
import long_guess_cases as C
import oracle_lib as O
from test_xrec_emulation import BUDGET, bfs_table, build_ximg

SEEDS, GUESSES = 8, 4
LOOKBACK, SEED_BYTES = 256, 64
HOT_BYTES = 120 * 1024  # rows of the seg kernel's LDS copy when there is no whole-DFA image
NONE = -1


class Dfa:
    """The whole DFA as the runtime loads it: breadth-first ids (start 0,
    start_m 1), the absorbing states, the image's resident rows, the seeds."""

    def __init__(self, pattern):
        cp = dgrep.CompiledPattern(pattern)
        assert not cp.partial
        bc, T = cp.tables()
        S, K = cp.nstates, cp.nclasses
        F = bfs_table(cp)
        # bfs_table's order again, for the blob id -> breadth-first id map
        order, bid = [], np.full(S, -1, np.int64)
        for x in [cp.start, cp.start_m]:
            if bid[x] < 0:
                bid[x] = len(order)
                order.append(x)
        q = 0
        while len(order) < S and q < len(order):
            for y in T[order[q]].tolist():
                if bid[y] < 0:
                    bid[y] = len(order)
                    order.append(y)
            q += 1
        for x in range(S):
            if bid[x] < 0:
                bid[x] = len(order)
                order.append(x)
        assert np.array_equal(bid[T.astype(np.int64)[np.array(order)]], F)
        self.nstates, self.nclasses = S, K
        self.cls = bytes(bc.tolist())  # bytes.translate table: byte -> class
        self.rows = F.tolist()
        self.start, self.start_m = int(bid[cp.start]), int(bid[cp.start_m])
        assert (self.start, self.start_m) == (0, 1) or cp.start == cp.start_m
        # MATCHED / DEAD: the first state (blob order) that every byte but '\n'
        # keeps, and '\n' sends to start_m / start
        cn = int(bc[10])
        others = np.delete(np.arange(K), cn)
        absorbing = np.flatnonzero((T[:, others] == np.arange(S)[:, None]).all(1))
        self.matched = self.dead = NONE
        for x in absorbing.tolist():
            if T[x, cn] == cp.start_m and self.matched == NONE:
                self.matched = int(bid[x])
            if T[x, cn] == cp.start and self.dead == NONE:
                self.dead = int(bid[x])
        self.nl = cn
        # the rows the seg kernel keeps in LDS: the whole-DFA image's (u16 ids), else the first 120 KiB
        self.u32 = S > 65535
        esz = 4 if self.u32 else 2
        self.x_hot = 0
        if not self.u32 and K < 0xFF and 2 * K > 8 and BUDGET >= 8 * S + 64 * 2 * K + 8:
            img = build_ximg(F)
            self.x_hot = img[0] if img else 0
        H = min(S, max(64, self.x_hot or HOT_BYTES // (esz * K)))
        self.seeds = [self.start] * SEEDS
        for i in range(1, SEEDS):
            if H <= 2:
                break
            x = i * (H - 1) // SEEDS
            for _ in range(S):
                if x not in (self.matched, self.dead, self.start):
                    break
                x = (x + 1) % S
            self.seeds[i] = x

    def run(self, s, classes):
        rows = self.rows
        for c in classes:
            s = rows[s][c]
        return s

    def absorbed(self, s):
        return s == self.matched or s == self.dead

    def guesses(self, classes, begin, seeds_run=SEEDS):
        """Entry guesses of the segment that starts at `begin` of the line."""
        if begin == 0:
            return [self.start]
        fa = begin - min(LOOKBACK, begin)
        mid = min(begin, fa + SEED_BYTES)
        sd = [self.run(s, classes[fa:mid]) for s in self.seeds[:seeds_run]]
        gs = []
        for s in sd:
            if not self.absorbed(s) and len(gs) < GUESSES and s not in gs:
                gs.append(s)
        if not gs:
            gs = [sd[0]]
        return [self.run(s, classes[mid:begin]) for s in gs]

    def walk(self, line, seeds_run=SEEDS):
        """(segments entered, segments re-run, verdict) of one parked line."""
        classes = line.translate(self.cls)
        s, segments, misses = self.start, 0, 0
        for begin in range(0, len(line), C.SEG):
            if self.absorbed(s):
                break
            segments += 1
            misses += s not in self.guesses(classes, begin, seeds_run)
            s = self.run(s, classes[begin:begin + C.SEG])
        return segments, misses, s == self.matched or self.rows[s][self.nl] == self.start_m


@functools.lru_cache(maxsize=None)
def model(name, seeds_run=SEEDS):
    """(segments, misses, verdicts, Dfa) of the named case's long lines."""
    case = C.CASES[C.CASE_IDS.index(name)]
    d = Dfa(C.pattern_of(case))
    segments = misses = 0
    verdicts = []
    for line in C.long_lines(case):
        g, m, v = d.walk(line, seeds_run)
        segments += g
        misses += m
        verdicts.append(v)
    return segments, misses, verdicts, d


@pytest.mark.parametrize("name", C.CASE_IDS)
def test_model_verdicts_and_miss_counts(name):
    case = C.CASES[C.CASE_IDS.index(name)]
    lines = C.long_lines(case)
    assert sum(map(len, lines)) < 2 << 20 and all(len(x) >= 9216 for x in lines)
    segments, misses, verdicts, d = model(name)
    assert d.nstates > 256 and d.u32 == name.startswith("u32"), d.nstates
    # (a) the model decides every line as the oracle does
    data, spans = C.split_of(lines)
    _, ost, ole = O.grep_map(C.pattern_of(case), data, threads=8)
    matching = dict(zip(ost.tolist(), ole.tolist()))
    want = [matching.get(a) == n for a, n in spans]
    assert verdicts == want
    assert True in want and False in want
    print("%s: states %d x_hot %d seeds %s segments %d misses %d" % (name, d.nstates, d.x_hot, d.seeds, segments,
                                                                     misses))
    assert segments >= len(lines) and misses <= segments
    # (b), (c): what the case is for (a requirement on the lines, not on the kernels)
    if case.expect == "some":
        assert misses > 0
    if case.expect == "zero":
        assert misses == 0


def test_single_seed_misses_where_eight_do_not():
    """Start alone as the seed (the round-5 kernel): a k-parity's segments are
    entered in the other class about half the time."""
    assert model("kw100_mod2")[1] == 0
    assert model("kw100_mod2", 1)[1] > 0


def test_walk_stops_at_the_absorbing_state():
    """A keyword in a line's first segment: one segment walked, whatever follows."""
    _, _, _, d = model("kw100")
    assert d.matched != NONE
    kw = dgrep.synth_keywords(4, 1)[0]
    line = b"x" * 100 + kw.upper() + b" y" * 40000
    assert d.walk(line) == (1, 0, True)
    assert d.walk(b"x y " * 20000) == (5, 0, False)
