"""The stepper cells: one pattern per scan-kernel instantiation dgrep_load_dfa
can pick, at the DFA sizes where its choice changes, and hand-built inputs for
the shapes each instantiation can get wrong. Data and generators only:
tests/test_stepper_cells.py checks them on the CPU (state counts, the loader's
rule restated, the planted shapes on the oracle's records) and
tests/test_gpu_stepper_cells.py runs them on the GPU.

A cell's `hit` makes a line match when it ends the line; its `miss` byte never
advances a match, so filler of `miss` bytes and '\\n' holds no matching line.
The generators are pure Python and deterministic (the filler's line lengths
come from a zlib.crc32 seed); each returns Cases: the split and what was
planted in it (check_planted asserts that on the oracle's records).
"""
import collections
import os
import random
import re
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "distributed-grep_amd", "csrc")
SCAN_COMMON_H = os.path.join(_CSRC, "kernels", "scan_common.h")
SCAN_DFA_HIP = os.path.join(_CSRC, "kernels", "scan_dfa.hip")
RUNTIME_HIP = os.path.join(_CSRC, "runtime", "dgrep_runtime.hip")

KW26 = ("alpha|bravo|charlie|delta|echo|foxtrot|golf|hotel|india|juliet|kilo|lima|mike|november|oscar|papa|quebec|"
        "romeo|sierra|tango|uniform|victor|whiskey|xray|yankee|zulu")
KW13 = "|".join(KW26.split("|")[:13])
KW14 = "|".join(KW26.split("|")[:14])
NUM = ("one|two|three|four|five|six|seven|eight|nine|ten|eleven|twelve|thirteen|fourteen|fifteen|sixteen|seventeen|"
       "eighteen|nineteen|twenty")
MON = "january|february|march|april|june|july|august|september|october|december"
_DIGITS = b"3141592653589793238462643383279502884197169399375105820974944592307816"

# name, pattern, force ("auto" / "table"), nstates, nclasses, expected (the
# instantiation: see choose()), hit, miss, xrun (x{n}$ cells: n)
Cell = collections.namedtuple("Cell", "name pattern force S K expected hit miss xrun")


def _table(rows, streams):
    return {"stepper": "table", "rows": rows, "streams": streams}


def _pair(entry, image, lds):
    return {"stepper": "pair", "entry": entry, "image": image, "lds": lds}


def _cell(name, pattern, force, S, K, expected, hit, miss=b"#", xrun=0):
    assert b"\n" not in hit and len(miss) == 1 and miss != b"\n"
    return Cell(name, pattern.encode(), force, S, K, expected, hit, miss, xrun)


def _kwd(n):
    return "(%s|%s|%s)[0-9]{%d}$" % (KW26, NUM, MON, n)


CELLS = [
    _cell("sheng-8", "^[a-j ]*error[a-j ]*$", "auto", 8, 6, {"stepper": "sheng"}, b"error", b"a"),
    _cell("pair-9", "warning", "auto", 9, 8, _pair("u32", 5088, 8192), b"warning"),
    _cell("pair-u16", "timeout while waiting for lock", "auto", 32, 19, _pair("u16", 27968, 40960),
          b"timeout while waiting for lock"),
    _cell("pair-u16-edge", "the quick brown fox jumps", "auto", 27, 22, _pair("u16", 31520, 40960),
          b"the quick brown fox jumps"),
    _cell("table-auto-32", "the quick brown fox jumps over", "auto", 32, 23, _table(32, 2),
          b"the quick brown fox jumps over"),
    _cell("table-auto-64", "pack my box with five dozen jugs", "auto", 34, 26, _table(64, 2),
          b"pack my box with five dozen jugs"),
    _cell("table-auto-64b", "(%s)[0-9]" % KW13, "auto", 61, 24, _table(64, 2), b"foxtrot7"),
    _cell("table-auto-128", "(%s)[0-9]" % KW14, "auto", 68, 24, _table(128, 1), b"november4"),
    _cell("table-auto-256", "(%s)[0-9]$" % KW26, "auto", 130, 29, _table(256, 1), b"uniform7"),
    _cell("table-auto-256i", "(?i)(%s)[0-9]{2}$" % KW26, "auto", 142, 34, _table(256, 1), b"UniForm42"),
    _cell("table-auto-255", _kwd(63), "auto", 255, 29, _table(256, 1), b"twenty" + _DIGITS[:63]),
    _cell("table-auto-256s", _kwd(64), "auto", 256, 29, _table(256, 1), b"december" + _DIGITS[:64]),
    _cell("filter-257", _kwd(65), "auto", 257, 29, {"stepper": "filter"}, b"one" + _DIGITS[:65]),
] + [
    _cell("table-%d" % S, "x{%d}$" % n, "table", S, 3, _table(rows, 2 if S <= 64 else 1), b"x" * n, b"y", n)
    for n, S, rows in ((14, 16, 16), (15, 17, 32), (30, 32, 32), (31, 33, 64), (62, 64, 64), (63, 65, 128),
                       (126, 128, 128), (127, 129, 256), (254, 256, 256))
] + [
    _cell("pair-257", "a[ab]{7}$", "auto", 257, 4, _pair("u16", 13456, 16384), b"abababab", b"c"),
    _cell("pair-302", "x{300}$", "auto", 302, 3, _pair("u32", 14816, 16384), b"x" * 300, b"y", 300),
    _cell("pair-1002", "x{1000}$", "auto", 1002, 3, _pair("u16", 28160, 40960), b"x" * 1000, b"y", 1000),
]
# forced onto the table stepper with one state too many: refused at load
REFUSED = _cell("table-refuse", "x{255}$", "table", 257, 3, {"stepper": None, "refused": True}, b"x" * 255, b"y", 255)
# the pair cells whose DFA the long-line table cannot hold: their lanes read a long line on
NO_PARKING = ("pair-257", "pair-302", "pair-1002")


# ---- the loader's rule, restated from the sources' constants ---------------
def source_constant(path, name):
    """The integer a source file gives `name`, as `#define name N` or
    `constexpr <type> name = N;`."""
    with open(path, encoding="utf-8") as f:
        text = f.read()
    m = (re.search(r"^#define %s (\d+)\b" % re.escape(name), text, re.M) or
         re.search(r"^constexpr \w+ %s = (\d+);" % re.escape(name), text, re.M))
    assert m, "%s: no integer constant %s" % (os.path.basename(path), name)
    return int(m.group(1))


def limits():
    """Every size the choice depends on, read by name."""
    with open(SCAN_DFA_HIP, encoding="utf-8") as f:
        scan = f.read()
    lim = {name: source_constant(SCAN_COMMON_H, name)
           for name in ("kPairT2", "kPairW32MaxImage", "kPairMaxT2", "kPairMaxImage")}
    lim["kRow"] = source_constant(SCAN_DFA_HIP, "kRow")
    lim["sheng_max"] = source_constant(RUNTIME_HIP, "DGREP_SHENG_MAX_STATES")
    # part_table's row steps (the last one takes the rest) and streams_of's limit
    steps = [int(x) for x in re.findall(r"run<StepTable, (\d+) \* kRow>", scan)]
    assert steps == sorted(set(steps)) and len(steps) == 5, steps
    lim["table_rows"] = steps
    m = re.search(r"kStepTable \? \(TBL <= (\d+) \* int\(kRow\) \? Tune<Step>::S : 1\)", scan)
    assert m, "streams_of: the table stepper's stream rule"
    lim["stream_rows"] = int(m.group(1))
    lim["table_streams"] = int(re.search(r"B = DGREP_TABLE_BLOCK, S = (\d+)", scan).group(1))
    # part_pair's LDS image steps
    m = re.search(r"table_bytes <= (\d+)\) return op\.template run<StepPair, \1>", scan)
    lim["pair32_small"] = int(m.group(1))
    m = re.search(r"table_bytes <= (\d+)\) return op\.template run<StepPair16, \1>", scan)
    lim["pair16_small"] = int(m.group(1))
    return lim


def pair_shadow_states(cp):
    """build_pair_image's S' = S + the distinct successors of start_m, if any
    '\\n' transition enters start_m (test_pair_emulation.build_pair's Sp)."""
    import test_pair_emulation

    return test_pair_emulation.build_pair(cp)["Sp"]


def pair_image(Sp, K, lim):
    """build_pair_image's size rule: (entry, image bytes), or None if the DFA
    does not fit."""
    def row_of(esz):
        return ((esz * K * K + 3) & ~3) | 4

    def end_of(r):
        t1 = (lim["kPairT2"] + r * Sp + 15) & ~15
        return (t1 + 2 * Sp * K + 15) & ~15

    esz = 4 if end_of(row_of(4)) <= lim["kPairW32MaxImage"] else 2
    row = row_of(esz)
    if row * Sp > lim["kPairMaxT2"] or end_of(row) > lim["kPairMaxImage"] or esz * (K - 1) > 255:
        return None
    return ("u32" if esz == 4 else "u16", end_of(row))


def choose(S, K, Sp, force, lim):
    """dgrep_load_dfa's choice for a whole (not partial) DFA, in its order:
    pair if wanted and fitting, filter above 256 states, Sheng, table."""
    def table():
        nbytes = (S * lim["kRow"] + 15) & ~15
        rows = next((r for r in lim["table_rows"][:-1] if nbytes <= r * lim["kRow"]), lim["table_rows"][-1])
        return _table(rows, lim["table_streams"] if rows <= lim["stream_rows"] else 1)

    if force == "table":
        return table() if S <= 256 else {"stepper": None, "refused": True}
    assert force == "auto"
    if S > lim["sheng_max"]:
        img = pair_image(Sp, K, lim)
        if img:
            entry, nbytes = img
            if entry == "u32":
                lds = lim["pair32_small"] if nbytes <= lim["pair32_small"] else lim["kPairW32MaxImage"]
            else:
                lds = lim["pair16_small"] if nbytes <= lim["pair16_small"] else lim["kPairMaxImage"]
            return _pair(entry, nbytes, lds)
    if S > 256:
        return {"stepper": "filter"}
    if S <= lim["sheng_max"]:
        return {"stepper": "sheng"}
    return table()


# ---- geometry ---------------------------------------------------------------
# C: lane chunk, S: chunks per lane (streams), B: the stepper's load block,
# cap: records a lane holds (LDS slots + spill area), force_chunk: the chunk to
# set with dgrep_set_lane_chunk (0: the default)
Geo = collections.namedtuple("Geo", "C S B cap force_chunk")


def tile_bytes(geo):
    return 64 * geo.S * geo.C


_PREFIX = {"sheng": "DGREP_SHENG", "pair": "DGREP_PAIR", "table": "DGREP_TABLE", "filter": "DGREP_FILTER"}


def geometry(cell, C=None, cap=None):
    """The cell's geometry; C and cap as the GPU reported them
    (scan_stats lane_chunk / lane_slots), else the sources' defaults."""
    stepper = cell.expected["stepper"]
    pre = _PREFIX[stepper]
    if C is None:
        C = source_constant(SCAN_DFA_HIP, pre + "_CHUNK")
    if cap is None:
        cap = source_constant(SCAN_DFA_HIP, pre + "_SLOTS")
        if stepper != "table":
            cap += source_constant(RUNTIME_HIP, "DGREP_SPILL_RECORDS")
    return Geo(C, cell.expected.get("streams", 1), source_constant(SCAN_DFA_HIP, pre + "_BLOCK"), cap, 0)


def _lines_per_chunk(cell, C):
    return C // (len(cell.hit) + 1) - 1  # whole `hit + '\n'` lines inside any chunk, at least


DENSE_FORCED_CHUNK = 16384


def dense_geometry(cell, geo):
    """The dense generator's geometry: where a short hit cannot overflow a
    lane's slots and spill area at the default chunk of an adaptive stepper
    (the u16 pair cells' 26 and 31 B lines: 176 and 147 per 4.5 KiB against 256
    records), the chunk is forced to 16 KiB."""
    if (len(cell.hit) <= 40 and cell.expected["stepper"] != "table" and
            _lines_per_chunk(cell, geo.C) <= geo.cap + 1):
        return geo._replace(C=DENSE_FORCED_CHUNK, force_chunk=DENSE_FORCED_CHUNK)
    return geo


# ---- inputs -----------------------------------------------------------------
Case = collections.namedtuple("Case", "name data planted")

_FILLER = {}


def filler(n, cell):
    """n bytes of non-matching lines of 0..120 `miss` bytes; always the same
    bytes for a cell, starting at a line start."""
    buf = _FILLER.get(cell.miss)
    if buf is None or len(buf) < n:
        rnd = random.Random(zlib.crc32(b"stepper cells filler " + cell.miss))
        out = bytearray()
        while len(out) < max(n, 1 << 20) + 200:
            out += cell.miss * rnd.randint(0, 120) + b"\n"
        buf = _FILLER[cell.miss] = bytes(out)
    return bytearray(buf[:n])


def pad(n, cell):
    """filler that ends with a '\\n' (what follows starts a line)."""
    d = filler(n, cell)
    if n:
        d[n - 1] = 0x0A
    return d


def plant(d, nl, hit):
    """`hit` + '\\n' with the '\\n' at byte nl: the line ending there matches."""
    assert nl >= len(hit) and nl < len(d), (nl, len(hit), len(d))
    d[nl - len(hit):nl] = hit
    d[nl] = 0x0A


def _shift(planted, off):
    out = {}
    for k, v in planted.items():
        if k in ("ends", "not_ends", "absent_starts"):
            out[k] = [x + off for x in v]
        elif k == "records":
            out[k] = [(s + off, l) for s, l in v]
        else:
            out[k] = v
    return out


def _merge(a, b):
    out = dict(a)
    for k, v in b.items():
        out[k] = out[k] + v if k in out and isinstance(v, list) else v
    return out


def lay(name, shape, planted, cell, geo):
    """The shape three times: alone in a split shorter than a tile (the
    part-tile path), and in a split whose first tile is whole, at offsets
    below 64 C (stream 0) and, with two streams, at 64 C or more (stream 1).
    The offsets are multiples of C, so residues of the block stay."""
    C, tile = geo.C, tile_bytes(geo)
    assert len(shape) < tile and len(shape) <= 58 * C, (name, len(shape))
    cases = [Case(name + "/part", bytes(shape), dict(planted, full_tile=False))]
    d = filler(tile + 777, cell)
    both = {}
    for k in range(geo.S):
        off = 64 * C * k + (3 + 2 * k) * C
        d[off - 1] = 0x0A
        d[off:off + len(shape)] = shape
        both = _merge(both, _shift(planted, off))
    cases.append(Case(name + "/full", bytes(d), dict(both, full_tile=True, both_streams=geo.S == 2)))
    return cases


def gen_placement(cell, geo):
    """A matching line's '\\n' at every residue of the stepper's block (so at
    every offset of a 16-byte window too); at most 4 per 2 KiB, so that no
    lane's slots overflow and the scan kernel itself writes the records."""
    B, L = geo.B, len(cell.hit)
    stride = max(512, -(-(L + 2) // B) * B)
    d = filler(stride * (B + 1) + B, cell)
    ends = []
    for i in range(B):
        q = stride * (i + 1) + i
        plant(d, q, cell.hit)
        ends.append(q)
    return lay("placement", d, {"ends": ends, "residues": B}, cell, geo)


def gen_adjacent(cell, geo):
    """Two to four '\\n' in one 4-byte word, from byte i to byte j for every
    i < j: once closing a matching line (then empty lines follow), once with a
    matching line starting right after the run."""
    L = len(cell.hit)
    slot = max(512, -(-(L + 40) // 16) * 16)
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    d = filler(slot * (2 * len(pairs) + 1), cell)
    ends, not_ends, records = [], [], []
    for k, (i, j) in enumerate(pairs):
        p = slot * (2 * k + 1) - 8  # a matching line, then j - i empty ones
        assert p % 4 == 0
        plant(d, p + i, cell.hit)
        d[p + i:p + j + 1] = b"\n" * (j - i + 1)
        ends.append(p + i)
        not_ends += list(range(p + i + 1, p + j + 1))
        p = slot * (2 * k + 1) + 16  # the run, then a line that is the hit alone
        d[p + i:p + j + 1] = b"\n" * (j - i + 1)
        plant(d, p + j + 1 + L, cell.hit)
        records.append((p + j + 1, L))
        not_ends += list(range(p + i, p + j + 1))
    return lay("adjacent", d, {"ends": ends, "not_ends": not_ends, "records": records}, cell, geo)


def _edges(geo):
    C = geo.C
    return [C, 64 * C] + ([128 * C] if geo.S == 2 else [])


def _quad(d, E, cell, ends):
    """a matching line closed at E - 2, then '\\n' at E - 1, E and E + 1"""
    plant(d, E - 2, cell.hit)
    for q in (E - 1, E, E + 1):
        if q < len(d):
            d[q] = 0x0A
    ends.append(E - 2)


def gen_edges(cell, geo):
    """'\\n' at E - 2 .. E + 1 for E = C, 64 C (and 128 C with two streams) in
    splits of tile - 1, tile and tile + 1 bytes; in a split of 2 tiles + 777:
    a matching line across each of those edges, a matching line starting
    exactly at a chunk end (2 C and 66 C), and the '\\n' groups in the second
    tile."""
    C, tile, L = geo.C, tile_bytes(geo), len(cell.hit)
    a = filler(tile + 64, cell)
    ends = []
    for E in _edges(geo):
        _quad(a, E, cell, ends)
    cases = []
    for n in (tile - 1, tile, tile + 1):
        cases.append(Case("edges/quad@%+d" % (n - tile), bytes(a[:n]),
                          {"ends": [e for e in ends if e < n], "full_tile": n >= tile}))
    b = filler(2 * tile + 777, cell)
    ends, records, straddle = [], [], []
    for E in _edges(geo):
        plant(b, E + max(1, L // 2), cell.hit)
        ends.append(E + max(1, L // 2))
        straddle.append(E)
        _quad(b, tile + E, cell, ends)
    for k in (2, 66):
        plant(b, k * C - 1, cell.hit)
        plant(b, k * C + L, cell.hit)
        ends.append(k * C - 1)
        records.append((k * C, L))
    cases.append(Case("edges/straddle", bytes(b), {"ends": ends, "records": records, "straddle": straddle,
                                                   "full_tile": True}))
    return cases


def gen_dense(cell, geo):
    """`hit + '\\n'` over a little more than three lane chunks: every line
    matches. overflow: a lane owns more of them than its slots and spill area
    hold (promised only where the line length makes it certain)."""
    line = cell.hit + b"\n"
    k = (3 * geo.C + 100) // len(line) + 1
    overflow = len(cell.hit) <= 40 and _lines_per_chunk(cell, geo.C) > geo.cap + 1
    return [Case("dense", line * k, {"count": k, "overflow": overflow, "full_tile": False})]


LONG_1 = lambda C: 3 * C + 4096 + 700
LONG_2 = lambda C: 5 * C + 37


def _long_seq(cell, C, at, records, absent):
    """Short matching lines between lines of LONG_1 and LONG_2 bytes of `miss`,
    with and without the hit at their end; for the x{n}$ cells a run of n + 17
    'x' whose middle lies on a chunk edge. Appends to records / absent."""
    hit, m = cell.hit, cell.miss
    short = m * 9 + hit
    lines = [(short, True)]
    for n in (LONG_1(C), LONG_2(C)):
        lines += [(m * (n - len(hit)) + hit, True), (short, True), (m * n, False), (short, True)]
    out = bytearray()
    for body, match in lines:
        if match:
            records.append((at + len(out), len(body)))
        else:
            absent.append(at + len(out))
        out += body + b"\n"
    if cell.xrun:
        run = cell.xrun + 17
        lead = (-(at + len(out) + run // 2)) % C  # the run's middle byte starts a chunk
        records.append((at + len(out), lead + run))
        out += m * lead + b"x" * run + b"\n"
    absent.append(at + len(out))
    out += m * 5 + b"\n"
    records.append((at + len(out), len(short)))
    out += short + b"\n"
    return out


def gen_long(cell, geo):
    """The long-line sequence at the split's start and again from 64 C + 1000
    (stream 1 of the first tile with two streams, else the second tile); the
    first tile is whole."""
    C, tile = geo.C, tile_bytes(geo)
    records, absent = [], []
    d = _long_seq(cell, C, 0, records, absent)
    second = 64 * C + 1000
    assert len(d) < second
    d += pad(second - len(d), cell)
    d += _long_seq(cell, C, second, records, absent)
    if len(d) < tile + 777:
        d += filler(tile + 777 - len(d), cell)
    return [Case("long", bytes(d), {"records": records, "absent_starts": absent,
                                    "long": min(LONG_1(C), LONG_2(C)),
                                    "full_tile": True})]


def gen_tail(cell, geo):
    """The split ends without '\\n' on a matching line, on a non-matching line,
    and directly after a '\\n'."""
    C, hit, m = geo.C, cell.hit, cell.miss
    a = pad(2 * C + 333, cell)
    b = pad(max(C - 5 - len(hit), 16), cell)
    c = pad(3 * C + 1 - len(hit) - 1, cell)
    return [
        Case("tail/match", bytes(a + m * 5 + hit), {"records": [(len(a), 5 + len(hit))], "full_tile": False}),
        Case("tail/miss", bytes(b + hit + b"\n" + m * 7),
             {"records": [(len(b), len(hit))], "absent_starts": [len(b) + len(hit) + 1], "full_tile": False}),
        Case("tail/newline", bytes(c + hit + b"\n"),
             {"records": [(len(c), len(hit))], "absent_starts": [len(c) + len(hit) + 1], "full_tile": False}),
    ]


GENERATORS = collections.OrderedDict([
    ("placement", gen_placement), ("adjacent", gen_adjacent), ("edges", gen_edges), ("dense", gen_dense),
    ("long", gen_long), ("tail", gen_tail),
])


def cases(cell, gen, geo):
    """(the generator's geometry, its cases)"""
    if gen == "dense":
        geo = dense_geometry(cell, geo)
    return geo, GENERATORS[gen](cell, geo)


def check_planted(case, geo, rec):
    """Asserts on the oracle's records (line_no, start, len) that the case
    holds what its generator planted."""
    C, tile, p = geo.C, tile_bytes(geo), case.planted
    starts, lens = rec[1].tolist(), rec[2].tolist()
    ends = set(s + l for s, l in zip(starts, lens))
    records = set(zip(starts, lens))
    assert p["full_tile"] == (len(case.data) >= tile), case.name
    assert set(p.get("ends", ())) <= ends, (case.name, sorted(set(p["ends"]) - ends)[:5])
    assert not set(p.get("not_ends", ())) & ends, case.name
    assert set(p.get("records", ())) <= records, (case.name, sorted(set(p["records"]) - records)[:5])
    assert not set(p.get("absent_starts", ())) & set(starts), case.name
    if "residues" in p:
        for span in ((0, tile), (0, 64 * C), (64 * C, 128 * C))[:3 if p.get("both_streams") else 1]:
            mine = [e for e in p["ends"] if span[0] <= e < span[1]]
            assert {e % 16 for e in mine} == set(range(16)), (case.name, span)
            assert {e % p["residues"] for e in mine} == set(range(p["residues"])), (case.name, span)
    if p.get("both_streams"):
        # events in both streams of a whole tile
        assert any(e < 64 * C for e in ends) and any(64 * C <= e < tile for e in ends), case.name
    for E in p.get("straddle", ()):
        assert any(s < E < s + l for s, l in records), (case.name, E)
    if "count" in p:
        assert len(starts) == p["count"], (case.name, len(starts))
    if "long" in p:
        assert sum(1 for l in lens if l >= p["long"]) >= 4, case.name
