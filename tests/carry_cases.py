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
"""
import random
import zlib

import window_cases as WC

SHENG8 = b"^[a-j ]*error[a-j ]*$"
EVEN_K = b"^[^k]*(k[^k]*k[^k]*)*$"                 # an even number of k: the DFA never forgets
GREEK = "^[α-ω]+$".encode("utf-8")       # a two-byte UTF-8 class
PATTERNS = [b"error", b"^$", b"", b"k$", b"^error", b"\\bk\\b", EVEN_K, GREEK]


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

    def walk(self, state, data):
        assert b"\n" not in data
        t, K, cls = self.trans, self.K, self.cls
        for b in data:
            state = t[state * K + cls[b]]
        return state

    def verdict(self, state):
        return not self.none and self.trans[state * self.K + self.nl] == self.start_m


def bounded(pieces, window, dfa, match):
    """The records each call returns: one list per feed, then the finish's.
    Also returns {"folds", "folded_bytes", "max_carry"}. Asserts the invariant:
    fewer than `window` bytes wait as the tail after every window."""
    calls, tail = [], b""
    byte_base = line_base = 0
    carrying, state, line_start = False, None, 0
    folds = folded = max_carry = 0
    for feed in pieces:
        got = []
        for o in range(0, len(feed), window):
            fill = tail + feed[o:o + window]
            F = len(fill)
            assert F < 2 * window
            cut = fill.rfind(b"\n")
            if cut < 0 and F >= window:  # fold: the bytes go into the state
                state = dfa.walk(state if carrying else dfa.start, fill)
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
                    if dfa.verdict(dfa.walk(state, fill[:f])):
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
        calls.append([(line_base + 1, line_start, n)] if dfa.verdict(dfa.walk(state, tail)) else [])
    else:
        calls.append(WC.split_records(tail, match, line_base, byte_base))
    return calls, {"folds": folds, "folded_bytes": folded, "max_carry": max_carry}


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
Long = __import__("collections").namedtuple("Long", "name window data cuts pattern longest")


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
