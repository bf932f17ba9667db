"""Data and references for the partition writers' byte rules (encode.hip,
encode_batch.hip, encode_window.hip and the job routes that reuse them): no GPU,
no library but the oracle. tests/test_writer_edge_cases.py checks what is
claimed here on the CPU; tests/test_gpu_writer_edges.py runs it on the GPU.

The alphabet is window_part_cases.EDGE_BYTES: the bounds of every second-byte
range of UTF-8 (after E0, ED, F0, F4), the invalid leads C0, F5, FF, the
continuation bytes on both sides of each bound, and 00 22 41 7F for the ASCII
widths 6, 2, 1, 1.

  short_values()   every string of 0..4 bytes over the alphabet
  de_bruijn()      every 4-gram over it exactly once, in 279,844 bytes
  long_split()     the de Bruijn value behind 0..15 bytes of padding
  record_cases()   every 3- and 4-gram as a record INSIDE a buffer: the bytes
                   behind a value are then not a '\\n' but each of the 23 bytes
  random_values()  2,000 seeded values around the lengths where a path changes
  lone_values()    every byte but '\\n' as a value's only byte outside plain
                   ASCII (the alphabet has no & < > \\ and one control byte)

Every expected byte comes from oracle_lib.json_kv, format_key and ihash.
go_json_witness() is an independent restatement of json_kv's escaping from
Python's strict UTF-8 decoder: it pins the oracle, it is not the reference.
"""
import codecs
import collections

import numpy as np

import oracle_lib as O
import window_part_cases as PC
from test_gpu_encode_records import LINE_NUMBERS
from window_part_cases import EDGE_BYTES

EDGE = EDGE_BYTES
LONG_VALUE = 256  # dgrep.LONG_VALUE_DEFAULT, the smallest dgrep_set_long_value accepts
TRUNCATED_LAST = b"the last line ends in \xf0\x9f\x98"

# a value that ever fails on a writer is named here and stays: (name, value bytes)
REGRESSIONS = []


# ---- the witness ------------------------------------------------------------------
_SHORT = {0x22: b'\\"', 0x5C: b"\\\\", 0x0A: b"\\n", 0x0D: b"\\r", 0x09: b"\\t"}
_char = {}


def _go_char(ch):
    """one decoded character as Go's encoding/json writes it (HTML escaping on)"""
    out = _char.get(ch)
    if out is None:
        c = ord(ch)
        if c in _SHORT:
            out = _SHORT[c]
        elif c < 0x20 or ch in "<>&" or c in (0x2028, 0x2029):
            out = b"\\u%04x" % c
        else:
            out = ch.encode("utf-8")  # 0x7f and a literal U+FFFD included: raw
        _char[ch] = out
    return out


def go_json_witness(value: bytes) -> bytes:
    """The body of the JSON string Go's json.Encoder writes for `value` (no
    quotes), from Python's strict UTF-8 decoder: where it refuses a byte, that
    ONE byte (e.start) becomes \\ufffd and decoding resumes behind it, as
    utf8.DecodeRune returns (RuneError, 1). Character by character: no replace()
    over finished text, which would take an escaped backslash followed by `b`
    for Python's \\b."""
    view, n, pos, out = memoryview(value), len(value), 0, []
    while pos < n:
        try:
            text, used = codecs.utf_8_decode(view[pos:], "strict", True)
            bad = False
        except UnicodeDecodeError as e:
            text, used = codecs.utf_8_decode(view[pos:pos + e.start], "strict", True)
            assert used == e.start
            bad = True
        out.extend(map(_go_char, text))
        pos += used
        if bad:
            out.append(b"\\ufffd")
            pos += 1
    return b"".join(out)


def witness_kv(key: bytes, value: bytes) -> bytes:
    return b'{"Key":"' + go_json_witness(key) + b'","Value":"' + go_json_witness(value) + b'"}\n'


# ---- the oracle, cached ---------------------------------------------------------------
_HEAD, _TAIL = b'{"Key":"","Value":"', b'"}\n'
_body = {}


def body(value: bytes) -> bytes:
    """the escaped form of one value: oracle_lib.json_kv's, computed once per distinct value"""
    out = _body.get(value)
    if out is None:
        line = O.json_kv(b"", value)
        assert line.startswith(_HEAD) and line.endswith(_TAIL)
        out = _body[value] = line[len(_HEAD):len(line) - len(_TAIL)]
    return out


def key_line_head(filename: bytes, line_no: int):
    """(ihash of the key, the line up to the value's first byte): json_kv's line is head + body + '"}\\n'"""
    key = O.format_key(filename, line_no)
    line = O.json_kv(key, b"")
    assert line.endswith(b'"' + _TAIL)
    return O.ihash(key), line[:len(line) - len(_TAIL)]


def needs_escape(v: bytes) -> bool:
    return any(b < 0x20 or b >= 0x80 or b in b'"\\<>&' for b in v)


def chunked(values, long_value=LONG_VALUE):
    """how many of the values the windowed writer's chunked path takes: long enough, and something to escape"""
    return sum(1 for v in values if len(v) >= long_value and needs_escape(v))


def lines_of(values):
    """the values as the lines of one split; the last has no '\\n'"""
    assert all(b"\n" not in v for v in values)
    return b"\n".join(values)


_parts = {}


def partitions(name, data, filename, nreduce):
    """dgrep_map_partitions of a named split under a pattern that matches every
    line (window_part_cases.whole_partitions): computed once, shared, never changed"""
    k = (name, bytes(filename), nreduce)
    if k not in _parts:
        _parts[k] = PC.whole_partitions(data, lambda line: True, filename, nreduce)
    return _parts[k]


def job_outputs(data, filename, nreduce):
    """(every mr-out-<r>, the lines read per partition) of a job over ONE file
    whose every line matches: the reduce keeps the first value of every key, and
    one file's keys are distinct, so mr-out-<r> is the partition's lines after
    the JSON round trip (oracle_lib.json_roundtrip_kv), "%v %v\\n" each, in
    input order. job_window_cases.expected_job gives the same bytes through
    go_json.reduce_reference, at ten times the cost on values of 280 KB."""
    outs, lines = [bytearray() for _ in range(nreduce)], [0] * nreduce
    for k, value in enumerate(data.split(b"\n")):
        key = O.format_key(filename, k + 1)
        p = O.ihash(key) % nreduce
        k2, v2 = O.json_roundtrip_kv(key, value)
        outs[p] += k2 + b" " + v2 + b"\n"
        lines[p] += 1
    return [bytes(o) for o in outs], lines


def cut_files(data, count, stem):
    """`data` cut after `count - 1` of its '\\n' into files whose lines, in
    order, are the split's: the '\\n' at a cut is dropped (it would add an empty
    last line). A cut is the first '\\n' behind k * n / count that leaves the
    next file's first byte at no multiple of 4 in the split."""
    files, at = [], 0
    for k in range(1, count):
        cut = data.index(b"\n", k * len(data) // count)
        while (cut + 1) % 4 == 0:
            cut = data.index(b"\n", cut + 1)
        files.append((b"%s-%d.log" % (stem, k - 1), data[at:cut]))
        at = cut + 1
    files.append((b"%s-%d.log" % (stem, count - 1), data[at:]))
    assert b"\n".join(d for _, d in files) == data
    return files


# ---- short values ----------------------------------------------------------------------
_cache = {}


def _once(fn):
    def wrapped():
        if fn.__name__ not in _cache:
            _cache[fn.__name__] = fn()
        return _cache[fn.__name__]
    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


@_once
def short_values():
    """every string of 0..4 bytes over EDGE: 1 + 23 + 23^2 + 23^3 + 23^4 = 292,561 values"""
    out, level = [b""], [b""]
    for _ in range(4):
        level = [v + bytes([b]) for v in level for b in EDGE]
        out += level
    return out


@_once
def short_split():
    """short_values() as the lines of one split, then a last line without '\\n'
    that ends inside a sequence. Under pattern b"" every line matches."""
    return lines_of(short_values() + [TRUNCATED_LAST])


# ---- the de Bruijn value ----------------------------------------------------------------
@_once
def de_bruijn():
    """B(23, 4) over EDGE (the standard recursive construction: the Lyndon words
    whose length divides 4, in order) plus its first 3 bytes, so that the
    cyclic 4-grams are all there: 23^4 + 3 = 279,844 bytes."""
    k, n = len(EDGE), 4
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
            return
        a[t] = a[t - p]
        db(t + 1, p)
        for j in range(a[t - p] + 1, k):
            a[t] = j
            db(t + 1, t)

    db(1, 1)
    s = bytes(EDGE[i] for i in seq)
    return s + s[:3]


def padded(p):
    return b"a" * p + de_bruijn()


def _short_plain(k):
    return b"plain line %d " % k + b"." * (3 * k % 11)


@_once
def long_split():
    """16 lines, line p = 'a' * p + de_bruijn(), between short plain lines. A
    lane of the chunked path takes one aligned 16-byte block: over the 16
    paddings every 4-gram lies at every phase of a block, wherever the window
    buffer puts the line. No step's lanes share a width sum (the widths 0, 1,
    2, 3, 4 and 6 all occur)."""
    out = []
    for p in range(16):
        out += [_short_plain(p), padded(p)]
    return lines_of(out + [_short_plain(16)])


# ---- the record form -----------------------------------------------------------------------
RECORD_SHORT_STARTS = 16384


@_once
def record_cases():
    """(buffer, records): the buffer is de_bruijn(); the records (line_no, st,
    le) are le in {3, 4} at every st in [0, 279841) and le in {0, 1, 2} at
    every st in [0, 16384), the line numbers LINE_NUMBERS cyclically. A value's
    last byte is followed IN THE BUFFER by every one of the 23 bytes, so a
    writer that counted `i + need <= L` past the value's end would complete a
    cut-off sequence; in a split a value is always followed by '\\n'."""
    buf = de_bruijn()
    n4 = len(buf) - 3
    st = np.concatenate([np.arange(n4), np.arange(n4)] + [np.arange(RECORD_SHORT_STARTS)] * 3).astype(np.uint64)
    le = np.concatenate([np.full(n4, 3), np.full(n4, 4)] +
                        [np.full(RECORD_SHORT_STARTS, k) for k in (0, 1, 2)]).astype(np.uint64)
    # interleave the lengths, so that neighbouring lanes hold values of different lengths
    order = np.random.RandomState(7).permutation(len(st))
    st, le = st[order], le[order]
    # every other one, round and round (their count is odd): neighbours differ in their digit counts
    assert len(LINE_NUMBERS) % 2 == 1
    ln = np.array(LINE_NUMBERS, dtype=np.uint64)[2 * np.arange(len(st)) % len(LINE_NUMBERS)]
    recs = np.stack([ln, st, le], axis=1)
    assert int((st + le).max()) == len(buf)
    return buf, recs


def record_expected(buf, recs, names, split_of=None):
    """nreduce = 1: the lines of every split's records in record order, split by
    split -- (bytes, [cell offsets])"""
    cells = [[] for _ in names]
    heads = {}
    for k, (ln, st, le) in enumerate(recs.tolist()):
        s = 0 if split_of is None else split_of[k]
        h = heads.get((s, ln))
        if h is None:
            h = heads[(s, ln)] = key_line_head(names[s], ln)[1]
        cells[s].append(h + body(buf[st:st + le]) + _TAIL)
    cells = [b"".join(c) for c in cells]
    off = [0]
    for c in cells:
        off.append(off[-1] + len(c))
    return b"".join(cells), off


# ---- random values ---------------------------------------------------------------------------
BANDS = ((0, 40, 0.70), (250, 260, 0.14), (4090, 4100, 0.10), (16370, 16400, 0.06))  # lo, hi (inclusive), share
_OTHER = np.array([b for b in range(256) if b != 0x0A], dtype=np.uint8)


def random_values(seed=2026):
    """2,000 values: the length from one of BANDS (below every threshold; around
    the long-value floor of 256; around one 4 KiB step of the chunked path;
    around one dgrep.LONG_CHUNK), every byte with probability 1/2 from EDGE,
    otherwise any byte but '\\n'. About 3 MB."""
    key = ("random_values", seed)
    if key not in _cache:
        rs = np.random.RandomState(seed)
        edge = np.frombuffer(EDGE, dtype=np.uint8)
        out = []
        for _ in range(2000):
            u = rs.random_sample()
            for lo, hi, share in BANDS:
                if u < share:
                    break
                u -= share
            n = int(rs.randint(lo, hi + 1))
            pick = rs.randint(0, 2, n).astype(bool)
            v = np.where(pick, edge[rs.randint(0, len(edge), n)], _OTHER[rs.randint(0, len(_OTHER), n)])
            out.append(v.astype(np.uint8).tobytes())
        _cache[key] = out
    return _cache[key]


@_once
def lone_values():
    """Every byte b but '\\n' alone among plain ASCII, so that b alone decides
    the value's path: at every position of a dword in a short value; in a long
    value that b alone makes an escaped one; and in a long value that a final
    '"' escapes anyway, where b is the only special byte of its 16-byte block."""
    out = []
    for b in range(256):
        if b == 0x0A:
            continue
        one = bytes([b])
        out += [b"abcdefg"[:k] + one + b"xyz" for k in range(4)]
        out.append(b"a" * (100 + b % 16) + one + b"a" * 180)
        out.append(b"a" * (100 + b % 16) + one + b"a" * 180 + b'"')
    return out


@_once
def random_split():
    """random_values(), the REGRESSIONS and lone_values() as the lines of one split"""
    return lines_of(random_values() + [v for _, v in REGRESSIONS] + lone_values())


def values_of(split):
    return split.split(b"\n")


# ---- what the inputs reach (the tally) ----------------------------------------------------------
@_once
def _de_bruijn_widths():
    """(every byte's output width by window_part_cases.escape_width, the index of the nearest byte before it
    that is no continuation byte)"""
    s = de_bruijn()
    w = np.array([PC.escape_width(s, i) for i in range(len(s))], dtype=np.int64)
    lead, last = np.zeros(len(s), dtype=np.int64), 0
    for i, b in enumerate(s):
        lead[i] = last
        if not 0x80 <= b <= 0xBF:
            last = i
    return w, lead


def long_classes(shift):
    """What the 16 long lines of long_split() put before the chunked path's lanes
    when the split's byte 0 lies `shift` bytes behind a 16-byte boundary of the
    buffer: a Counter of
      width0 .. width6   bytes of that output width
      halo_left          a continuation byte in a block's first 3 bytes swallowed by a lead in the block before
      halo_right         a valid sequence whose lead is in a block's last 3 bytes and that ends in the next block
      first_partial / first_whole   the value starts inside / at the start of its first block
      last_partial / ends_on_edge   the value ends inside / at the end of its last block
      sums               the fewest distinct width sums among the 256 lanes of a line's first 4 KiB step
    """
    w, lead = _de_bruijn_widths()
    sb = np.frombuffer(de_bruijn(), dtype=np.uint8)
    tally = collections.Counter()
    at, fewest = 0, 256
    for line in long_split().split(b"\n"):
        start, at = at, at + len(line) + 1
        if len(line) < LONG_VALUE:
            continue
        p = len(line) - len(sb)
        addr = shift + start  # the value's first byte in the buffer
        tally["first_whole" if addr % 16 == 0 else "first_partial"] += 1
        tally["ends_on_edge" if (addr + len(line)) % 16 == 0 else "last_partial"] += 1
        tally["width1"] += p
        for wd, cnt in enumerate(np.bincount(w, minlength=7).tolist()):
            tally["width%d" % wd] += cnt
        a = addr + p + np.arange(len(sb))
        tally["halo_left"] += int(((w == 0) & (a % 16 < 3) & ((addr + p + lead) // 16 < a // 16)).sum())
        tally["halo_right"] += int(((w >= 2) & (w <= 4) & (sb >= 0xC2) & (a // 16 < (a + w - 1) // 16)).sum())
        first = addr & ~15
        lane = np.concatenate([(addr + np.arange(p) - first) // 16, (a - first) // 16])
        wl = np.concatenate([np.ones(p, dtype=np.int64), w])
        sel = lane < 256
        fewest = min(fewest, len(set(np.bincount(lane[sel], weights=wl[sel], minlength=256).astype(np.int64).tolist())))
    tally["sums"] = fewest
    return tally


def edge_classes(split, shift):
    """Where the chunked values of a split start and end against the 16-byte
    blocks when the split's byte 0 lies `shift` bytes behind a block boundary:
    a Counter of first_whole / first_partial / ends_on_edge / last_partial."""
    tally, at = collections.Counter(), 0
    for line in split.split(b"\n"):
        start, at = shift + at, at + len(line) + 1
        if len(line) >= LONG_VALUE and needs_escape(line):
            tally["first_whole" if start % 16 == 0 else "first_partial"] += 1
            tally["ends_on_edge" if (start + len(line)) % 16 == 0 else "last_partial"] += 1
    return tally


LONG_CLASSES = ("width0", "width1", "width2", "width3", "width4", "width6", "halo_left", "halo_right")
EDGE_CLASSES = ("first_partial", "first_whole", "last_partial", "ends_on_edge")


def paths(values):
    """(plain, escaped by one lane, chunked at the long-value floor) counts of a split's values"""
    esc = [v for v in values if needs_escape(v)]
    long_ = sum(1 for v in esc if len(v) >= LONG_VALUE)
    return len(values) - len(esc), len(esc) - long_, long_
