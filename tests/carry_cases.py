"""Data and a pure-Python model for the bounded windowed scan
(DGREP_STREAM_BOUNDED / dgrep_scan_bounded): no GPU, no library beyond the
pattern compiler.

bounded() restates the stream's state machine over a compiled pattern's own
tables (CompiledPattern.tables()): a full window without a '\\n' is folded into
the DFA state and forgotten; when the line's '\\n' arrives its last bytes are
walked from the carried state and the verdict's record takes the place of what
the window's scan made of those bytes alone; a finish while carrying walks the
tail. The regions an ordinary scan takes use a per-line predicate (the
oracle's), as window_cases.windowed() does.

walk_model() restates the walk itself (csrc/kernels/carry_plan.h and the two
kernels of carry.hip): the chunk plan, the lookback's guesses and the chunks
whose true entry state none of them is -- what dgrep_stream_carry_stats counts.
"""
import collections
import random
import zlib

import numpy as np

import window_cases as WC

SHENG8 = b"^[a-j ]*error[a-j ]*$"
EVEN_K = b"^[^k]*(k[^k]*k[^k]*)*$"                 # an even number of k: the DFA never forgets
GREEK = "^[α-ω]+$".encode("utf-8")       # a two-byte UTF-8 class
PATTERNS = [b"error", b"^$", b"", b"k$", b"^error", b"\\bk\\b", EVEN_K, GREEK]


CARRY_GUESSES = 4        # kCarryGuesses
CARRY_LOOKBACK = 256     # kCarryLookback
CARRY_MIN_CHUNK = 256    # kCarryMinChunk
CARRY_ROWS_LDS = 32 << 10  # kCarryRowsLds


def carry_plan(m, max_lanes):
    """carry_plan.h: (chunk, nchunks), the smallest chunk of 256 << k that needs at most max_lanes lanes"""
    max_lanes = max_lanes or 1
    chunk = CARRY_MIN_CHUNK
    while chunk < (1 << 62) and -(-m // chunk) > max_lanes:
        chunk <<= 1
    return chunk, -(-m // chunk)


def carry_lanes(m, num_cus, rows_in_lds):
    """carry_plan.h: the power of two at or above sqrt(m), four times that for rows read through the caches,
    within [64, 1024 per CU]"""
    r = 1
    while r < (1 << 31) and r * r < m:
        r <<= 1
    if not rows_in_lds:
        r <<= 2
    most = (num_cus or 1) * 1024
    return 64 if r < 64 else most if r > most else r


def rows_in_lds(nstates, nclasses):
    """win_walk's choice: the rows, u16 while the ids fit, go to LDS up to 32 KiB"""
    return nstates * nclasses * (4 if nstates > 65535 else 2) <= CARRY_ROWS_LDS


def carry_absorbing(trans, nstates, nclasses, nl_class):
    """carry_plan.h: absorbing[x] = 1 iff every class but nl_class loops at x"""
    return [int(all(trans[x * nclasses + k] == x for k in range(nclasses) if k != nl_class)) for x in range(nstates)]


def carry_seeds(absorbing, nstates, start):
    """carry_plan.h: `start`, then states spread over the ids, never an absorbing one nor one taken before"""
    seed = [start] * CARRY_GUESSES
    for i in range(1, CARRY_GUESSES):
        if nstates <= 1:
            break
        x = (i * nstates // CARRY_GUESSES) % nstates
        for _ in range(nstates):
            if not absorbing[x] and x not in seed[:i]:
                seed[i] = x
                break
            x = (x + 1) % nstates
    return seed


def walk_model(dfa, data, entry, from_start, num_cus, trace=None):
    """carry_walk over `data` (no '\\n'): (exit_state, chunk, nchunks, misses). Chunk c > 0 guesses what the four
    seeds reach over data[c * chunk - 256 : c * chunk), chunk 0 knows its entry; a chunk misses when its true entry
    state is neither absorbing nor among its guesses (counters[1] of carry_fix_kernel). `trace`, a dict, also
    gets the missing chunks' indexes and the first chunk in which the state is absorbing."""
    assert b"\n" not in data
    if from_start:
        entry = dfa.start
    m = len(data)
    chunk, nchunks = carry_plan(m, carry_lanes(m, num_cus, dfa.rows_in_lds))
    miss_chunks, absorbed_at = [], None
    if trace is not None:
        trace.update(miss_chunks=miss_chunks, absorbed_at=None)
    if nchunks == 0:
        return entry, chunk, 0, 0
    cls = dfa.cls_np[np.frombuffer(data, np.uint8)]
    guesses = []
    if nchunks > 1:  # every lookback at once: [nchunks - 1, 4] states over [nchunks - 1, 256] classes
        at = np.arange(1, nchunks, dtype=np.int64)[:, None] * chunk - CARRY_LOOKBACK + np.arange(CARRY_LOOKBACK)
        look = cls[at]
        s = np.tile(np.array(dfa.seeds, np.int64), (nchunks - 1, 1))
        for j in range(CARRY_LOOKBACK):
            s = dfa.trans_np[s, look[:, j:j + 1]]
        guesses = s.tolist()
    t, K, steps = dfa.trans_scaled, dfa.K, cls.tobytes()
    st = entry * K
    for c in range(nchunks):
        x = st // K
        if dfa.absorbing[x]:  # nothing but a '\n' moves it
            if absorbed_at is None:
                absorbed_at = c - 1 if c else -1  # -1: the entry state already was
            continue
        if c and x not in guesses[c - 1]:
            miss_chunks.append(c)
        for k in steps[c * chunk:(c + 1) * chunk]:
            st = t[st + k]
    if absorbed_at is None and dfa.absorbing[st // K]:
        absorbed_at = nchunks - 1
    if trace is not None:
        trace["absorbed_at"] = absorbed_at
    return st // K, chunk, nchunks, len(miss_chunks)


class Dfa:
    """the blob's DFA (include/dgrep_blob.h): walk() over newline-free bytes,
    verdict() = the line ending in that state matches"""

    def __init__(self, cp):
        import dgrep

        bc, tr = cp.tables()
        self.cls = bc.tolist()
        self.K = cp.nclasses
        self.trans = tr.reshape(-1).tolist()
        self.start, self.start_m = cp.start, cp.start_m
        self.nl = self.cls[0x0A]
        self.none = bool(cp.flags & dgrep.DFA_MATCH_NONE)
        assert not cp.partial
        # what the walk's model needs (carry_ensure in the runtime)
        self.nstates = cp.nstates
        self.cls_np, self.trans_np = bc.copy(), tr.astype(np.int64)
        self.rows_in_lds = rows_in_lds(cp.nstates, cp.nclasses)
        self.absorbing = carry_absorbing(self.trans, cp.nstates, cp.nclasses, self.nl)
        self.seeds = carry_seeds(self.absorbing, cp.nstates, cp.start)
        self.trans_scaled = [x * self.K for x in self.trans]  # ids times the row length: one index per step

    def walk(self, state, data):
        assert b"\n" not in data
        t, K, cls = self.trans, self.K, self.cls
        for b in data:
            state = t[state * K + cls[b]]
        return state

    def verdict(self, state):
        return not self.none and self.trans[state * self.K + self.nl] == self.start_m


def bounded(pieces, window, dfa, match, num_cus=256, detail=None):
    """The records each call returns: one list per feed, then the finish's.
    Also returns {"folds", "folded_bytes", "max_carry", "walks"}; walks has one
    (kind, m, from_, chunk, nchunks, misses) per walk the stream makes, kind
    `fold`, `head` or `finish`, from_ the length of the tail in front of a head,
    the rest walk_model()'s for a device of num_cus CUs. `detail`, a list, gets
    one dict per walk: its entry state, its bytes, the whole buffer they lie in
    and walk_model's trace.
    Asserts the invariant: fewer than `window` bytes wait as the tail after
    every window."""
    calls, tail = [], b""
    byte_base = line_base = 0
    carrying, state, line_start = False, None, 0
    folds = folded = max_carry = 0
    walks = []

    def walk(kind, data, from_=0, fill=None):
        """the exit of `data` from the carried state, as win_walk: noted in walks"""
        trace = {}
        x, chunk, nchunks, misses = walk_model(dfa, data, state, not carrying, num_cus, trace)
        walks.append((kind, len(data), from_, chunk, nchunks, misses))
        if detail is not None:
            detail.append(dict(trace, kind=kind, entry=state if carrying else dfa.start, data=data, exit=x,
                               fill=data if fill is None else fill))
        return x

    for feed in pieces:
        got = []
        for o in range(0, len(feed), window):
            fill = tail + feed[o:o + window]
            F = len(fill)
            assert F < 2 * window
            cut = fill.rfind(b"\n")
            if cut < 0 and F >= window:  # fold: the bytes go into the state
                state = walk("fold", fill)
                if not carrying:
                    line_start = byte_base
                carrying = True
                byte_base += F
                tail = b""
                folds += 1
                folded += F
                max_carry = max(max_carry, byte_base - line_start)
            elif cut < 0:  # as without the flag: the bytes wait as the tail
                tail = fill
                max_carry = max(max_carry, byte_base + F - line_start if carrying else F)
            else:
                recs = WC.split_records(fill[:cut], match, line_base, byte_base)
                if carrying:
                    f = fill.index(b"\n")
                    assert b"\n" not in tail and f >= len(tail)
                    if recs and recs[0][1] == byte_base:  # the scan's verdict on the head alone: wrong, dropped
                        recs = recs[1:]
                    if dfa.verdict(walk("head", fill[:f], len(tail), fill)):
                        recs = [(line_base + 1, line_start, byte_base + f - line_start)] + recs
                    max_carry = max(max_carry, byte_base + f - line_start)
                    carrying = False
                elif tail:
                    max_carry = max(max_carry, fill.index(b"\n"))
                got += recs
                byte_base += cut + 1
                line_base += fill[:cut + 1].count(b"\n")
                tail = fill[cut + 1:]
                max_carry = max(max_carry, len(tail))
            assert len(tail) < window, (len(tail), window)
        calls.append(got)
    if carrying:
        n = byte_base + len(tail) - line_start
        max_carry = max(max_carry, n)
        calls.append([(line_base + 1, line_start, n)] if dfa.verdict(walk("finish", tail)) else [])
    else:
        calls.append(WC.split_records(tail, match, line_base, byte_base))
    return calls, {"folds": folds, "folded_bytes": folded, "max_carry": max_carry, "walks": walks}


def flat(calls):
    return [r for call in calls for r in call]


def body(n, at=0):
    """n bytes of [a-j ], the same for every call"""
    return (b"abcdefghij " * ((at + n) // 11 + 2))[at:at + n]


def k_line(n, seed, nk):
    """n bytes of [a-j ] with nk 'k' at seeded random places"""
    rnd = random.Random(zlib.crc32(b"carry cases k_line") + seed)
    d = bytearray(body(n))
    for p in rnd.sample(range(n), nk):
        d[p] = ord("k")
    return bytes(d)


# name, window, split, the piece cuts to feed it by, the pattern it is made
# for, the length of its longest line
Long = collections.namedtuple("Long", "name window data cuts pattern longest")


def _long_splits(W):
    """(name, split, pattern): lines longer than a window, and where their '\\n' falls against the windows"""
    out = []
    for at_start in (True, False):
        data, _ = WC.long_line(W, at_start)
        out.append(("hit_first" if at_start else "hit_last", data, SHENG8))
    n = 13 * W // 2  # the hit only in a middle window
    out.append(("hit_middle", WC.lines(700, 31) + body(3 * W + 100) + b"error" + body(n - 3 * W - 105) + b"\n" +
                WC.lines(400, 32) + b"no hit here", SHENG8))
    out.append(("miss_middle", WC.lines(700, 31) + body(3 * W + 100) + b"errxr" + body(n - 3 * W - 105) + b"\n" +
                WC.lines(400, 32) + b"j error", SHENG8))
    out.append(("no_newline_20", b"abc " * (20 * W // 4) + b"error", b"error"))       # finish while carrying
    out.append(("no_newline_20_miss", b"abc " * (20 * W // 4) + b"erro", b"error"))
    out.append(("nl_first", b"error" + body(3 * W - 5) + b"\n" + WC.lines(W + 9, 33) + b"tail error", SHENG8))
    out.append(("nl_last", body(3 * W - 6) + b"error\n" + WC.lines(W // 2, 34) + b"error", SHENG8))
    out.append(("back_to_back", WC.lines(90, 35) + body(5 * W // 2) + b"error\n" + body(13 * W // 4) + b"\n" +
                b"error" + body(9 * W // 4) + b"\n" + WC.lines(200, 36), SHENG8))
    out.append(("ends_exact", body(2 * W - 5) + b"error", SHENG8))  # the stream ends with the fold: finish walks nothing
    assert out[6][1][3 * W] == 0x0A and out[7][1][3 * W - 1] == 0x0A and len(out[9][1]) == 2 * W
    return out


def _long_cases():
    out = []
    for W in WC.WINDOWS:
        for name, data, pattern in _long_splits(W):
            longest = max(map(len, data.split(b"\n")))
            assert longest >= 2 * W
            for fname, cuts in (("whole", []), ("random", WC.random_cuts("carry " + name, len(data), 5))):
                out.append(Long("%s/%s/w%d" % (name, fname, W), W, data, cuts, pattern, longest))
        # a long line fed in 1-byte pieces around its end
        data, n = WC.long_line(W, False)
        end = data.index(b"\n", 1000 - 1 + n - 5)
        assert data[end - 5:end] == b"error"
        out.append(Long("hit_last/bytes/w%d" % W, W, data, list(range(end - 12, end + 12)), SHENG8, n))
    return out


LONG = _long_cases()


def memory_line(W, seed, nwin=12):
    """a split whose first line is nwin windows of [a-j ] with seeded random 'k': (split, the line's k count)"""
    n = nwin * W + W // 3
    nk = 40 + seed % 7
    return WC.lines(300, 37) + k_line(n, seed, nk) + b"\n" + WC.lines(300, 38) + b"k", nk


def greek_line(W):
    """a line of 3.5 windows of two-byte runes starting at an odd offset, so every fold cuts one mid-rune"""
    runes = "αβγδω".encode("utf-8")
    line = runes * (7 * W // 2 // len(runes))
    data = b"ab\n" + line + b"\n" + line[:-1] + b"\nx" + line + b"\n" + "ω".encode("utf-8")
    assert (W - 3) % 2 == 1
    return data


# ---- windows past one cut tile and one batch of the fix kernel ---------------------
# Up to 64 KiB a walk is at most 256 chunks of 256 bytes and the cut pass one
# workgroup per 16 KiB tile; these windows reach the plans, batches and partials
# beyond (tests/test_carry_emulation.py lists what the cases must show).
SCALE_WINDOWS = (65536, 131072, 1048576)
KEYWORDS = b"alpha|bravo|charlie"
C3 = b"^[0-9]{4}-[0-9]{2}.*(WARN|ERROR) [a-z_]+"
U16_GLOBAL = b"a[ab]{12}$"  # 8193 states: u16 entries, rows of 65,544 bytes read through the caches
U32 = b"a[ab]{16}$"         # 131,073 states: u32 entries


def mod_k(p):
    """the number of k is divisible by p: a DFA that keeps the count for the whole line"""
    return b"^(([^k]*k){%d})*[^k]*$" % p


SCALE_PATTERNS = collections.OrderedDict([("sheng", SHENG8), ("error", b"error"), ("keywords", KEYWORDS), ("c3", C3),
                                          ("mod7", mod_k(7)), ("mod3", mod_k(3)), ("u16_global", U16_GLOBAL),
                                          ("u32", U32)])
SCALE_1M = ("sheng", "mod7", "keywords")  # the patterns that also run at the 1 MiB window

Scale = collections.namedtuple("Scale", "name window data cuts pattern")


def planted(n, at, word):
    """body(n) with `word` at offset `at`"""
    d = bytearray(body(n))
    assert 0 <= at and at + len(word) <= n
    d[at:at + len(word)] = word
    return bytes(d)


def k_every(n, seed, p, divisible):
    """n bytes of [a-j ] with a k every 2 to 4 KiB at seeded places; their number is divisible by p, or one short"""
    rnd = random.Random(zlib.crc32(b"carry cases k_every") + seed)
    at, pos = [], rnd.randrange(2048, 4097)
    while pos < n:
        at.append(pos)
        pos += rnd.randrange(2048, 4097)
    keep = len(at) - len(at) % p - (0 if divisible else 1)
    assert keep > p
    d = bytearray(body(n))
    for q in at[len(at) - keep:]:
        d[q] = ord("k")
    return bytes(d)


def ab_line(n, seed, k, hit):
    """n seeded random bytes of [ab]; the byte k + 1 from the end decides a[ab]{k}$"""
    rnd = random.Random(zlib.crc32(b"carry cases ab_line") + seed)
    d = bytearray(rnd.choices(b"ab", k=n))
    d[n - k - 1] = ord("a" if hit else "b")
    return bytes(d)


def _after(W, seed):
    """short lines behind the long one: a '\\n' in every later 16 KiB tile of the window"""
    return WC.lines(W + 333 if W < (1 << 20) else W // 4, seed) + b"tail error"


# Where the long line lies against the windows; each gives (line length, how to
# build the split from the line, the feed cuts). With one whole feed the pieces
# are taken at multiples of W, and after a fold the tail is empty, so a byte at
# split offset q then lies at buffer offset q mod W.
def _at0(W, line):
    """the line starts the split: every fold has F = W"""
    return line + b"\n" + _after(W, 52)


def _prefixed(W, line):
    """short lines up to offset W - 1, then the line: its first fold has F = W + 1"""
    return WC.lines(W - 1, 51) + line + b"\n" + _after(W, 53)


def _unended(W, line):
    """the split ends inside the line: a finish while carrying"""
    return line


def _layouts(W):
    return {
        # name: (line length, build, cuts)
        "nl_16383": (3 * W + 16383, _at0, []),                 # the '\n' is the last byte of cut tile 0
        "nl_16384": (3 * W + 16385, _prefixed, []),            # ... the first byte of tile 1; a head of 64 whole chunks
        "nl_last_tile": (5 * W - 300, _at0, []),               # ... in the window's last tile, more behind it
        "long_head": (4 * W - 99, _prefixed, []),              # a head of W - 100 bytes behind a fold of W + 1
        "from_tile1": (3 * W + 49925, _at0, [3 * W, 3 * W + 20000]),  # the tail ends in tile 1, the '\n' lies in tile 3
        "finish": (3 * W + 20003, _unended, []),               # a finish walk of 79 chunks
        "two_windows": (4 * W + 777, _at0, [W - 1, 2 * W - 1]),  # a tail of W - 1 bytes, then a fold of 2 W - 1
        "short_head": (3 * W + 20000, _at0, []),
    }


def _scale_case(W, pname, name, layout, make):
    """make(n) -> the long line of n bytes"""
    n, build, cuts = _layouts(W)[layout]
    line = make(n)
    assert len(line) == n and b"\n" not in line
    return Scale("%s/%s/w%d" % (pname, name, W), W, build(W, line), cuts, SCALE_PATTERNS[pname])


def _word_pair(W, pname, layout, at, hit, miss, name=None, lead=b""):
    """two splits that differ in one byte of the long line, with opposite verdicts for it"""
    assert len(hit) == len(miss) and sum(a != b for a, b in zip(hit, miss)) == 1
    out = []
    for tag, word in (("hit", hit), ("miss", miss)):
        out.append(_scale_case(W, pname, "%s/%s" % (name or layout, tag), layout,
                               lambda n: lead + planted(n - len(lead), at(n) - len(lead), word)))
    return out


_scale_memo = {}


def scale_cases(W, pname):
    """the splits of one pattern at one window of SCALE_WINDOWS (built once)"""
    if (W, pname) not in _scale_memo:
        _scale_memo[W, pname] = _scale_build(W, pname)
    return _scale_memo[W, pname]


def _scale_build(W, pname):
    out = []
    big = W >= (1 << 20)
    if big:
        # about 3.3 windows: one line at offset 0, one behind a prefix of W - 1 bytes
        lay = {"at0": (3 * W + 314573, _at0, []), "prefixed": (3 * W + 1 + 300000, _prefixed, [])}

        def case(name, layout, make):
            n, build, cuts = lay[layout]
            line = make(n)
            assert len(line) == n and b"\n" not in line
            return Scale("%s/%s/w%d" % (pname, name, W), W, build(W, line), cuts, SCALE_PATTERNS[pname])

        assert pname in SCALE_1M
        if pname == "mod7":
            return [case("at0/div", "at0", lambda n: k_every(n, 1, 7, True)),
                    case("prefixed/rem", "prefixed", lambda n: k_every(n, 2, 7, False))]
        hit, miss = (b"error", b"errxr") if pname == "sheng" else (b"bravo", b"bravx")
        # a word in chunk 683 of the second fold; a word in chunk 576 of the head (sheng) or in the first chunk of all
        for layout, at in (("at0", lambda n: W + 700000), ("prefixed", (lambda n: n - 5000) if pname == "sheng" else
                                                             (lambda n: 40))):
            for tag, word in (("hit", hit), ("miss", miss)):
                out.append(case("%s/%s" % (layout, tag), layout, lambda n: planted(n, at(n), word)))
        return out
    if pname in ("sheng", "error"):
        E, X = b"error", b"errxr"
        out += _word_pair(W, pname, "nl_16383", lambda n: W + 3 * W // 4, E, X)       # chunk 384 of a 128 KiB fold
        out += _word_pair(W, pname, "nl_last_tile", lambda n: n - 200, E, X)          # the head's last chunk
        if pname == "error":  # the accepting state absorbs: the rest is the Sheng pattern's business
            return out + _word_pair(W, pname, "two_windows", lambda n: 2 * W - 301, E, X)
        out += _word_pair(W, pname, "nl_16384", lambda n: n - 3000, E, X)             # in the head
        out += _word_pair(W, pname, "from_tile1", lambda n: 3 * W + 30000, E, X)      # behind the tail, in the head
        out += _word_pair(W, pname, "finish", lambda n: n - 5, E, X)                  # the split's last bytes
        out += _word_pair(W, pname, "two_windows", lambda n: 2 * W - 301, E, X)       # the 2 W - 1 fold's last chunks
    elif pname == "keywords":
        B, X = b"bravo", b"bravx"
        # absorbing from the first chunk on; in chunk 384 of a 128 KiB fold; only in the head; `br` folded and `avo`
        # the head's first bytes
        out += _word_pair(W, pname, "nl_last_tile", lambda n: 40, B, X, "early")
        out += _word_pair(W, pname, "long_head", lambda n: W + 1 + 3 * W // 4, B, X, "deep")
        out += _word_pair(W, pname, "nl_last_tile", lambda n: n - 3000, B, X, "head")
        out += _word_pair(W, pname, "short_head", lambda n: 3 * W - 2, B, X, "straddle")
        out += _word_pair(W, pname, "two_windows", lambda n: 2 * W - 301, B, X)
        out += _word_pair(W, pname, "finish", lambda n: 3 * W + 100, B, X)
    elif pname == "c3":
        out.append(_scale_case(W, pname, "no_digit", "nl_16383", body))  # rejects at the line's first byte
        E, X = b" ERROR io_wait", b" ERRxR io_wait"
        out += _word_pair(W, pname, "long_head", lambda n: W + 1 + 3 * W // 4, E, X, "date_deep", b"2024-01 ")
        # the head alone starts with no digit: the chain from `start` stops at once, the carried one runs on
        out += _word_pair(W, pname, "nl_last_tile", lambda n: n - 3000, E, X, "date_head", b"2024-01 ")
    elif pname in ("mod7", "mod3"):
        p = 7 if pname == "mod7" else 3
        for i, (layout, div) in enumerate((("nl_last_tile", True), ("nl_16384", False), ("two_windows", False),
                                           ("finish", True), ("from_tile1", True))):
            out.append(_scale_case(W, pname, "%s/%s" % (layout, "div" if div else "rem"), layout,
                                   lambda n: k_every(n, 10 * p + i, p, div)))
    else:
        k = 12 if pname == "u16_global" else 16
        for i, (layout, hit) in enumerate((("long_head", True), ("long_head", False), ("nl_16383", True),
                                           ("two_windows", False))):
            out.append(_scale_case(W, pname, "%s/%s" % (layout, "hit" if hit else "miss"), layout,
                                   lambda n: ab_line(n, 5 if layout == "long_head" else i, k, hit)))
    return out
