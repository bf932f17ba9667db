"""Data and a pure-Python model for the windowed whole job (dgrep_job_* /
dgrep_grep_job_windowed): no GPU, no library but the oracle.

expected_job() is what the resident job must give: go_json.reduce_reference
over partitions built from the oracle's Map (encode_batch_cases), as
test_gpu_reduce_batch.py checks dgrep_grep_job. model_job() restates the plan
of csrc/runtime/job_plan.h: which files are packed, when a pack is flushed,
which files stream through windows (window_part_cases.windowed_partitions), and
what every flush and every window appends to the arena and to the segment
table. Its outputs are the reduce reference over the arena cut by seg_off with
segment g in partition g % nreduce.
"""
import collections
import random
import zlib

import encode_batch_cases as E
import go_json as G
import oracle_lib as O
import window_cases as WC
import window_part_cases as PC

WINDOWS = (4096, 8192)          # the GPU file's: the smallest window and twice it
CPU_WINDOWS = (4096, 8192, 65536)
ARENA_INITIAL = 4096            # job_plan.h kJobArenaInitial
LONG_NAME = b"d/" * 1100 + b"past-the-lds-head.txt"  # its escaped form is past the line writer's LDS copy

Case = collections.namedtuple("Case", "name pattern files nreduce")
Model = collections.namedtuple(
    "Model", "arena seg_off appends outputs lines_in packs files_packed files_windowed rows arena_cap growths")


def matcher(pattern):
    rx = O.Regexp(pattern)
    if rx.status != 0:  # Go rejects the pattern: grep.go drops the error and nothing matches
        return lambda line: False
    cache = {}

    def match(line):
        if line not in cache:
            cache[line] = rx.match(line)
        return cache[line]
    match.rx = rx  # keeps the handle alive
    return match


def expected_job(pattern, files, nreduce):
    """(outputs, lines_in) of dgrep_grep_job(files, nreduce)"""
    parts = [E.expected_partitions(pattern, f, d, nreduce) for f, d in files]
    outs, lines = [], []
    for r in range(nreduce):
        data = b"".join(p[r] for p in parts)
        ref = G.reduce_reference(data)
        assert ref.bad_line is None
        outs.append(ref.output)
        lines.append(data.count(b"\n"))
    return outs, lines


def _grow(cap, need, initial):
    """job_plan.h job_grow_cap"""
    if need <= cap:
        return cap
    return max(2 * cap if cap else initial, need)


def model_job(pattern, files, window, nreduce, routes, feeds):
    """routes[i]: "add" (dgrep_job_add) or "stream" (begin / feed / end);
    feeds[i]: the ascending cut offsets of a streamed file (ignored for "add")."""
    match = matcher(pattern)
    arena, seg, appends = bytearray(), [0], []
    pack, tally = [], collections.Counter()
    cap = {"arena": 0, "growths": 0}

    def append(cells, rows):
        total = sum(map(len, cells))
        need = (len(arena) + total + 15) & ~15
        grown = _grow(cap["arena"], need, ARENA_INITIAL)
        if cap["arena"] and grown != cap["arena"]:
            cap["growths"] += 1
        cap["arena"] = grown
        appends.append((len(arena), total, rows))
        for c in cells:
            arena.extend(c)
            seg.append(len(arena))
        tally["rows"] += rows

    def flush():
        if not pack:
            return
        tally["packs"] += 1
        raw, off = E.expected_cells(pattern, pack, nreduce)
        if raw:  # a pack without a matching line appends nothing
            off = [int(x) for x in off]
            append([raw[off[c]:off[c + 1]] for c in range(len(off) - 1)], len(pack))
        del pack[:]

    for (name, data), route, cuts in zip(files, routes, feeds):
        if route == "add" and len(data) <= window:
            tally["files_packed"] += 1
            if pack and sum(len(d) for _, d in pack) + len(pack) + len(data) > window:
                flush()  # the pack's bytes, its separators and one more would pass the window
            pack.append((name, data))
            continue
        tally["files_windowed"] += 1
        flush()  # task order: the pack's cells come before this file's
        pieces = [data] if route == "add" else WC.pieces_of(data, cuts)
        for rows in PC.windowed_partitions(pieces, window, match, name, nreduce):
            for row in rows:
                append(row, 1)
    flush()
    nseg = len(seg) - 1
    outs, lines = [], []
    for p in range(nreduce):
        data = b"".join(bytes(arena[seg[g]:seg[g + 1]]) for g in range(p, nseg, nreduce))
        ref = G.reduce_reference(data)
        assert ref.bad_line is None
        outs.append(ref.output)
        lines.append(data.count(b"\n"))
    return Model(bytes(arena), seg, appends, outs, lines, tally["packs"], tally["files_packed"],
                 tally["files_windowed"], tally["rows"], cap["arena"], cap["growths"])


# ---- routes and feed cuts ---------------------------------------------------------
def route_assignments(case):
    """Every add / stream assignment for up to 5 files; beyond that all-add,
    all-stream, both alternations and four seeded ones."""
    k = len(case.files)
    if k <= 5:
        return [tuple("stream" if (m >> i) & 1 else "add" for i in range(k)) for m in range(1 << k)]
    rnd = random.Random(zlib.crc32(b"job routes " + case.name.encode()))
    out = [("add",) * k, ("stream",) * k, tuple(("add", "stream")[i & 1] for i in range(k)),
           tuple(("stream", "add")[i & 1] for i in range(k))]
    out += [tuple(rnd.choice(("add", "stream")) for _ in range(k)) for _ in range(4)]
    return out


def mixed(case):
    """add and stream alternating, the first file added"""
    return tuple(("add", "stream")[i & 1] for i in range(len(case.files)))


def step_cuts(case, step):
    return [list(range(step, len(d), step)) for _, d in case.files]


def random_cuts(case):
    return [WC.random_cuts("job %s %d" % (case.name, i), len(d), 3) for i, (_, d) in enumerate(case.files)]


def whole(case):
    return [[] for _ in case.files]


# ---- the cases ---------------------------------------------------------------------
def _all_error(n, seed):
    """exactly n bytes of lines that all hold `error`, the last byte a '\\n'"""
    rnd = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += b"error %d " % len(out) + b"x" * rnd.randrange(50) + b"\n"
    del out[n:]
    out[n - 1] = 0x0A
    return bytes(out)


def _residue_names():
    """Filenames from 1 byte up, one matching line each: picked so that the
    arena offset before an append and the appended total each take every residue
    modulo 16 when every file is streamed (one row per file)."""
    def total(n):
        name = b"n" * n
        return len(O.json_kv(O.format_key(name, 1), b"error"))
    names, at, seen_at, seen_total = [], 0, set(), set()
    while len(seen_at) < 16 or len(seen_total) < 16:
        best = max(range(1, 40), key=lambda n: ((at % 16) not in seen_at) + (total(n) % 16 not in seen_total) * 2 +
                   (((at + total(n)) % 16) not in seen_at) - n / 1000.0)
        seen_at.add(at % 16)
        seen_total.add(total(best) % 16)
        names.append(b"n" * best)
        at += total(best)
        assert len(names) < 80
    return names


def cases(W):
    """the jobs for a window of W bytes: the route edge and the pack sizes follow W"""
    L = WC.lines
    esc = b'error "quoted" <&> \xe2\x80\xa8 ' + b'\xff"' * 200  # needs escaping, past the long-value floor of 256
    assert len(esc) >= 256
    # a line of 1.5 windows between short ones: the carried tail grows the window buffers
    long_line = L(1000, 11) + b"error" + (b"abcdefghij " * (W // 7))[:3 * W // 2 - 5] + b"\n" + L(500, 12) + b"j error j"
    half = W // 2
    out = [
        Case("edges", b"error", [(b"empty", b""), (b"no-newline", b"an error without an end"),
                                 (b"no-final-newline", L(700, 41) + b"the last error"), (b"only-newline", b"\n"),
                                 (b"plain", L(900, 42))], 10),
        Case("route_edge", b"error", [(b"w", L(W, 43)), (b"w-1", L(W - 1, 44)), (b"w+1", L(W + 1, 45))], 10),
        # a + 1 separator + b == W: full to the byte; then one more byte overflows it
        Case("pack_full", b"error", [(b"a", L(half, 46)), (b"b", L(W - half - 1, 47)), (b"c", L(300, 48))], 10),
        Case("pack_overflow", b"error", [(b"a", L(half, 46)), (b"b", L(W - half, 49)), (b"c", L(300, 48))], 10),
        Case("window_between_packs", b"error",
             [(b"s1", L(500, 50)), (b"s2", L(600, 51)), (b"big", L(2 * W + 77, 52) + b"tail error"),
              (b"s3", L(400, 53)), (b"s4", b"error at the end")], 10),
        # both files hold line 1 and line 2: the earlier file's values stay
        Case("same_name", b"error", [(b"twice.log", b"error A\nerror B\nok\n"), (b"other.log", L(300, 54)),
                                     (b"twice.log", b"error C\nok\nerror D\n")], 10),
        Case("long_line", b"error", [(b"head", L(200, 55)), (b"long", long_line), (b"tail", b"error\n")], 10),
        Case("long_value", b"error", [(b"small-escaped", L(300, 56) + esc + b"\n"),
                                      (b"windowed-escaped", L(W, 57) + esc + b"\n" + L(500, 58) + esc)], 10),
        Case("names", b"error", [(n, b"error\n") for n in _residue_names()] +
             [(LONG_NAME, b"ok\nerror\n"), (b'"' * 1030, b"error")], 10),
        Case("no_match", b"zzz_never", [(b"a", L(600, 59)), (b"b", L(W + 9, 60)), (b"c", b"")], 10),
        Case("syntax_error", b"(", [(b"a", b"(\n"), (b"b", L(W + 9, 60))], 10),
        Case("nreduce_1", b"error", [(b"a", L(800, 61)), (b"b", L(W + 300, 62)), (b"c", L(500, 63))], 1),
        # more segments than lines
        Case("nreduce_1000", b"error", [(b"a", b"error 1\nok\n"), (b"b", L(W + 100, 64)[:W + 100 - 300] + b"z" * 299 + b"\n"),
                                        (b"c", b"ok\nerror 2")], 1000),
        # first appends small, then one file whose windows grow the arena several times
        Case("growth", b"error", [(b"t1", b"error\n"), (b"t2", b"ok\nan error\n"), (b"big", _all_error(6 * W, 65))], 10),
    ]
    return out


def many_small():
    """64 files of 1 KiB for a 64 KiB window: 63 of them and their 62 separators fit one pack"""
    return Case("many_small", b"error", [(b"f%02d" % i, WC.lines(1024, 100 + i)) for i in range(64)], 10)


def residues(model):
    """(arena offsets before the appends, appended totals), modulo 16"""
    return {at % 16 for at, _, _ in model.appends}, {total % 16 for _, total, _ in model.appends}
