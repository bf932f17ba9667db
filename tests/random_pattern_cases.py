"""Random patterns for the GPU: a deterministic selection of
test_compiler._rand_pattern draws, bucketed by DFA size, and two corpora that
every scan entry point and every stepper the loader can be made to pick run
over. Data and generators only: tests/test_random_pattern_cases.py checks them
on the CPU (quotas, corpus B's geometry, mixed verdicts on the long lines, the
interpreted DFA and NFA program against the oracle) and
tests/test_gpu_random_patterns.py runs them on the GPU, so that a failure
there points at a loader image or a kernel.

The hand-written patterns of the other GPU tests fix a DFA's size; these vary
its structure: where '\\n' leads, which states absorb, start != start_m,
multi-byte classes, \\b / $ / \\z contexts.

Everything expensive is memoised at module level; the oracle's records are
computed once per (pattern, input) and never changed.
"""
import collections
import random

import dgrep
import oracle_lib as O
import stepper_cells as SC
from test_compiler import ALPHA, _rand_pattern

# ---- the selection --------------------------------------------------------------
SEED = 2026       # random.Random(SEED) feeds _rand_pattern
DRAW_CAP = 5000   # selected() fails if the quotas are not full after this many draws
QUOTA = 20        # distinct patterns per bucket
BUCKETS = (("le8", 1, 8), ("9-32", 9, 32), ("33-256", 33, 256), ("gt256", 257, 1 << 30))
PARTIAL_BUDGET = 3  # the forced state budget of the `partial` mode

Case = collections.namedtuple("Case", "name pattern nstates nclasses bucket")

# patterns that once failed on the GPU, by name: every mode also runs them
REGRESSIONS = []

_memo = {}


def bucket_of(nstates):
    return next(name for name, lo, hi in BUCKETS if lo <= nstates <= hi)


def compiled(pattern, budget=0):
    """the product's CompiledPattern, once per (pattern, budget)"""
    k = ("cp", bytes(pattern), budget)
    if k not in _memo:
        _memo[k] = dgrep.CompiledPattern(pattern, state_budget=budget)
    return _memo[k]


def _lines_of(data):
    """[(start, len)] of the lines of `data` (strings.Split semantics)"""
    out, pos = [], 0
    for line in data.split(b"\n"):
        out.append((pos, len(line)))
        pos += len(line) + 1
    return out


def selected():
    """The cases, and the number of draws they took (selection_draws()). A
    draw is kept if the oracle compiles it, the product compiles it to a DFA
    that is neither MATCH_ALL, MATCH_NONE nor a Go syntax error, its bytes are
    new, its bucket is not full and the oracle finds both a matching and a
    non-matching line in corpus A."""
    if "selected" in _memo:
        return _memo["selected"]
    rnd = random.Random(SEED)
    a = corpus_a()
    nlines = len(_lines_of(a))
    by = {name: [] for name, _, _ in BUCKETS}
    seen = set()
    draws = 0
    while any(len(v) < QUOTA for v in by.values()):
        if draws >= DRAW_CAP:
            raise AssertionError("random_pattern_cases.selected: quotas not full after %d draws: %r" % (
                draws, {k: len(v) for k, v in by.items()}))
        draws += 1
        pat = _rand_pattern(rnd).encode()
        if pat in seen or O.compile_status(pat) != O.ORC_OK:
            continue
        try:
            cp = compiled(pat)
        except dgrep.UnsupportedPattern:
            continue
        if cp.partial or cp.flags & (dgrep.DFA_MATCH_ALL | dgrep.DFA_MATCH_NONE | dgrep.DFA_GO_SYNTAX_ERROR):
            continue
        b = bucket_of(cp.nstates)
        if len(by[b]) >= QUOTA:
            continue
        n = len(want(pat, "A")[0])
        if n == 0 or n == nlines:
            continue
        seen.add(pat)
        by[b].append(Case("%s-%02d" % (b, len(by[b])), pat, cp.nstates, cp.nclasses, b))
    _memo["draws"] = draws
    _memo["selected"] = [c for name, _, _ in BUCKETS for c in by[name]]
    return _memo["selected"]


def selection_draws():
    selected()
    return _memo["draws"]


def regressions():
    by = {c.name: c for c in selected()}
    return [by[name] for name in REGRESSIONS]


# ---- corpus A: short lines -------------------------------------------------------
A_BYTES = 48 << 10


def _short_lines(rnd, nbytes):
    """lines of 0..24 ALPHA tokens ('\\n' is one of them), at least nbytes, ending with a '\\n'"""
    out = bytearray()
    while len(out) < nbytes:
        for _ in range(rnd.randint(0, 24)):
            out += rnd.choice(ALPHA)
        out += b"\n"
    return out


def corpus_a():
    """About 48 KiB of lines of 0..24 ALPHA tokens ('\\r', invalid and
    truncated UTF-8, `error`); the last line has no trailing '\\n'."""
    if "A" not in _memo:
        rnd = random.Random(SEED + 1)
        d = _short_lines(rnd, A_BYTES)
        d += b"".join(rnd.choice([t for t in ALPHA if t != b"\n"]) for _ in range(7))
        _memo["A"] = bytes(d)
    return _memo["A"]


def slice_a():
    """the first 4 KiB of corpus A, for the Python interpreters"""
    return corpus_a()[:4096]


# ---- corpus B: short lines with long lines spread through them ------------------
LONG_TOKENS = (b"1", b" ", b".", b"\xff", "é".encode(), b"b", b"_", b"\xe2\x82")
LONG_LENGTHS = (6 << 10, 20 << 10, 70 << 10)
B_MAX = 2 << 20

Stepper = collections.namedtuple("Stepper", "name expected")
# one entry per tile geometry the loader's choice can give
STEPPERS = (Stepper("sheng", {"stepper": "sheng"}), Stepper("pair", {"stepper": "pair"}),
            Stepper("filter", {"stepper": "filter"}), Stepper("table-2", {"stepper": "table", "streams": 2}),
            Stepper("table-1", {"stepper": "table", "streams": 1}))


def tiles():
    """{stepper: tile bytes at its compiled chunk}"""
    return {s.name: SC.tile_bytes(SC.geometry(s)) for s in STEPPERS}


def _piece(rnd):
    """a short random piece of a line: 1..6 ALPHA tokens, none a '\\n'"""
    return b"".join(rnd.choice([t for t in ALPHA if t != b"\n"]) for _ in range(rnd.randint(1, 6)))


def _long_lines(rnd):
    """For each token and a length cycling through LONG_LENGTHS: the bare
    repeated token, and the token with a short random piece at its start, in
    its middle and at its end."""
    out, k = [], 0
    for tok in LONG_TOKENS:
        for where in ("bare", "start", "middle", "end"):
            n = LONG_LENGTHS[k % len(LONG_LENGTHS)] // len(tok)
            k += 1
            p = b"" if where == "bare" else _piece(rnd)
            at = {"bare": 0, "start": 0, "middle": n // 2, "end": n}[where]
            out.append(tok * at + p + tok * (n - at))
    rnd.shuffle(out)
    return out


def corpus_b():
    """(data, [(start, len)] of its long lines). The short lines of corpus A
    with 32 long lines spread through them, placed so that the first two tile
    edges of every stepper each fall inside a long line; at least two tiles
    and 777 bytes of the largest tile; below 2 MiB."""
    if "B" in _memo:
        return _memo["B"]
    rnd = random.Random(SEED + 2)
    edges = sorted({k * t for t in tiles().values() for k in (1, 2)})
    size = 2 * max(tiles().values()) + 777
    out, longs = bytearray(), []
    for line in _long_lines(rnd):
        gap = rnd.randint(2 << 10, 12 << 10)
        ahead = [e for e in edges if e > len(out)]
        if ahead and ahead[0] <= len(out) + gap + 200:
            # the next edge would fall among short lines: the long line starts before it
            gap = max(0, ahead[0] - len(line) // 2 - len(out))
        out += _short_lines(rnd, gap) if gap else b""
        longs.append((len(out), len(line)))
        out += line + b"\n"
    out += _short_lines(rnd, max(size - len(out), 3 << 10))
    out += _piece(rnd)  # the last line has no trailing '\n'
    assert len(out) < B_MAX, len(out)
    _memo["B"] = (bytes(out), longs)
    return _memo["B"]


def straddled(tile):
    """{tile edge: the long lines of corpus B that start before it and end after it}"""
    data, longs = corpus_b()
    return {e: [(s, l) for s, l in longs if s < e < s + l] for e in range(tile, len(data), tile)}


# ---- splits of corpus A -----------------------------------------------------------
def splits_of(data):
    """`data` cut at 9 fixed pseudo-random byte offsets (not aligned to lines:
    some fall inside a line, some inside a multi-byte sequence), plus one empty
    split and one of a single byte."""
    rnd = random.Random(SEED + 3)
    cuts = sorted(rnd.sample(range(1, len(data)), 9))
    # one cut is moved into the nearest multi-byte UTF-8 sequence after it
    k = next(i for i in range(cuts[4], len(data)) if data[i] & 0xC0 == 0x80 and data[i - 1] >= 0xC2)
    cuts[4] = k
    cuts = sorted(set(cuts))
    parts = [data[a:b] for a, b in zip([0] + cuts, cuts + [len(data)])]
    return parts[:3] + [b""] + parts[3:] + [data[cuts[0]:cuts[0] + 1]]


def split_cuts(data):
    """the byte offsets of `data` at which splits_of cuts it"""
    cuts, at = [], 0
    for p in splits_of(data)[:-1]:
        at += len(p)
        if 0 < at < len(data) and (not cuts or cuts[-1] != at):
            cuts.append(at)
    return cuts


# ---- the oracle's records ------------------------------------------------------------
def data_of(which):
    """"A", "B", "A4K" (slice_a) or ("split", i) (splits_of(corpus A)[i])"""
    if which == "A":
        return corpus_a()
    if which == "B":
        return corpus_b()[0]
    if which == "A4K":
        return slice_a()
    kind, i = which
    assert kind == "split"
    return splits_of(corpus_a())[i]


def want(pattern, which):
    """The oracle's (line_no, start, len) of `pattern` over data_of(which):
    one oracle pass per (pattern, which), shared by every mode."""
    k = ("want", bytes(pattern), which)
    if k not in _memo:
        rec = O.grep_map(pattern, data_of(which), threads=16 if which == "B" else 0)
        for r in rec:
            r.setflags(write=False)
        _memo[k] = rec
    return _memo[k]


def long_verdicts(pattern):
    """(matching, non-matching) long lines of corpus B, by the oracle's records"""
    _, longs = corpus_b()
    rec = want(pattern, "B")
    got = set(zip(rec[1].tolist(), rec[2].tolist()))
    hit = sum(1 for sl in longs if sl in got)
    return hit, len(longs) - hit


# ---- what the loader does with a case ----------------------------------------------
def pair_fits(cp):
    """Whether build_pair_image holds this DFA (stepper_cells.pair_image on its
    shadow-state count). The size rule grows with the state count, so a DFA
    that does not fit without shadow states does not fit with them: the
    emulation's image is only built where it can matter."""
    lim = SC.limits()
    if SC.pair_image(cp.nstates, cp.nclasses, lim) is None:
        return None
    return SC.pair_image(SC.pair_shadow_states(cp), cp.nclasses, lim)


def auto_choice(cp):
    """stepper_cells.choose for the default stepper selection"""
    lim = SC.limits()
    Sp = SC.pair_shadow_states(cp) if pair_fits(cp) else cp.nstates + cp.nclasses
    return SC.choose(cp.nstates, cp.nclasses, Sp, "auto", lim)


def parks(stepper, nstates, partial=False):
    """Whether the runtime parks long lines: Sheng, pair and table with the
    long-line table (DFAs of at most 256 states), the filter on a whole DFA
    (stepper_cells.NO_PARKING: the pair stepper above 256 states reads on)."""
    if stepper == "filter":
        return not partial
    return nstates <= 256


def partial_counts(cp, data):
    """(lines that reach CAND, lines that stay in the kept states and match)
    of a partial blob over `data`: the first are decided by the NFA program.
    All lines step in lockstep, one numpy gather per byte column."""
    import numpy as np

    assert cp.partial
    bc, tr = cp.tables()
    cand, nl = cp.nstates - 1, int(bc[10])
    lines = data.split(b"\n")
    width = max(len(x) for x in lines)
    cls = np.full((len(lines), width), -1, np.int64)
    for i, x in enumerate(lines):
        cls[i, :len(x)] = bc[np.frombuffer(x, np.uint8)]
    tr = tr.astype(np.int64)
    s = np.full(len(lines), cp.start, np.int64)
    for j in range(width):
        c = cls[:, j]
        live = (c >= 0) & (s != cand)
        s[live] = tr[s[live], c[live]]
    reached = s == cand
    direct = ~reached & (tr[s, nl] == cp.start_m)
    return int(reached.sum()), int(direct.sum())
