"""Data and a pure-Python model for the windowed scan (dgrep_scan_windowed /
dgrep_stream_*): no GPU, no library.

windowed() restates the algebra of csrc/kernels/window.h over a per-line
predicate: a window's bytes up to its last '\\n' are the lines it completed,
the rest is carried, and the records are rebased by the running byte and line
counts. CASES lists the splits, each with the piece cuts to feed it by.
"""
import collections
import random
import zlib

WINDOWS = (4096, 8192)


def split_records(data, match, line_base=0, byte_base=0):
    """grep.go:17-29 over `data`: (line_no, start, len) of every matching line
    of strings.Split(data, "\\n"), moved by the two bases."""
    out, pos = [], 0
    for i, line in enumerate(data.split(b"\n")):
        if match(line):
            out.append((line_base + i + 1, byte_base + pos, len(line)))
        pos += len(line) + 1
    return out


def windowed(pieces, window, match):
    """The records each call returns: one list per feed, then the finish's.
    Also returns (windows that completed a line, longest carried tail)."""
    calls, tail = [], b""
    byte_base = line_base = 0
    scanned = max_carry = 0
    for feed in pieces:
        got = []
        for o in range(0, len(feed), window):
            fill = tail + feed[o:o + window]
            cut = fill.rfind(b"\n")
            if cut < 0:  # no line completed: all of it is carried
                tail = fill
                max_carry = max(max_carry, len(tail))
                continue
            got += split_records(fill[:cut], match, line_base, byte_base)
            byte_base += cut + 1
            line_base += fill[:cut + 1].count(b"\n")
            tail = fill[cut + 1:]
            max_carry = max(max_carry, len(tail))
            scanned += 1
        calls.append(got)
    calls.append(split_records(tail, match, line_base, byte_base))  # the stream's last line
    return calls, (scanned + 1, max_carry)


def pieces_of(data, cuts):
    """data cut at the ascending offsets `cuts` (a repeated offset is a feed of length 0)."""
    out, at = [], 0
    for c in list(cuts) + [len(data)]:
        assert at <= c <= len(data), (at, c)
        out.append(data[at:c])
        at = c
    assert b"".join(out) == data
    return out


def random_cuts(name, n, k):
    rnd = random.Random(zlib.crc32(b"window cases " + name.encode()))
    return sorted(rnd.randrange(n + 1) for _ in range(k)) if n else [0] * k


_WORDS = (b"an error here", b"ok", b"", b"warning: disk", b"x" * 57, b"error", b"2024-01-02 ERROR io_wait",
          b"aaa bbb error ccc", b"nothing to see", b"e r r o r")


def lines(n, seed, longest=120):
    """exactly n bytes of short lines (some empty, some with `error`), the last byte a '\\n'"""
    rnd = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        w = rnd.choice(_WORDS)
        out += (w + b"." * rnd.randrange(max(longest - len(w), 1)))[:longest] + b"\n"
    del out[n:]
    if n:
        out[n - 1] = 0x0A
    return bytes(out)


Case = collections.namedtuple("Case", "name window data cuts")


def _feeds(name, data):
    """the feed patterns every split gets: whole, random cuts, and feeds of length 0 between others"""
    n = len(data)
    r = random_cuts(name, n, 5)
    return [("whole", []), ("random", r), ("zeros", [0, 0] + [c for c in r[:2] for _ in (0, 1)] + [n, n])]


def _splits(W):
    """(name, split): where the '\\n' falls against a window of W bytes"""
    body = lines(W - 1, 1)
    out = [
        ("nl_last", lines(W, 2) + lines(W // 2, 3) + b"error"),              # a '\n' as a window's last byte
        ("nl_first", body + b"e\n" + lines(W + 7, 4) + b"tail"),            # ... as the next window's first byte
        ("line_is_window", b"error" + b"j" * (W - 5) + b"\n" + lines(300, 5)),  # a line exactly one window long
        ("line_is_window2", lines(100, 6) + b"a" * (W - 5) + b"error\nlast error"),
        ("all_newlines", b"\n" * (2 * W) + b"error\n\n"),                  # a window made entirely of '\n'
        ("no_newline", b"an error without an end"),                         # a split with no '\n' at all
        ("no_newline_long", b"abc " * (5 * W // 8) + b"error"),              # ... longer than two windows
        ("ends_in_newline", lines(3 * W + 11, 7)),                           # an empty last line
        ("only_newline", b"\n"),
        ("empty", b""),                                                      # the empty split
        ("cut_in_match", lines(W - 3, 8) + b"error in the cut\n" + lines(W - 2, 9) + b"er" + b"ror\nx"),
        ("short_300", lines(300, 10, 40)),
    ]
    assert out[0][1][W - 1] == 0x0A and out[1][1][W] == 0x0A and out[1][1][W - 1] != 0x0A
    assert out[2][1].index(b"\n") == W and out[10][1][W - 3:W + 2] == b"error"
    return out


def _cases():
    out = []
    for W in WINDOWS:
        for name, data in _splits(W):
            for fname, cuts in _feeds(name, data):
                out.append(Case("%s/%s/w%d" % (name, fname, W), W, data, cuts))
        s300 = dict(_splits(W))["short_300"]
        out.append(Case("short_300/bytes/w%d" % W, W, s300, list(range(1, 300))))  # 300 one-byte feeds
    return out


CASES = _cases()


def long_line(W, hit_at_start):
    """a line of 3.5 windows of [a-j ] with its `error` at its very start or its very end, between short lines"""
    n = 7 * W // 2
    body = (b"abcdefghij " * (n // 11 + 1))[:n - 5]
    line = b"error" + body if hit_at_start else body + b"error"
    return lines(1000, 11) + line + b"\n" + lines(500, 12) + b"j error j", len(line)
