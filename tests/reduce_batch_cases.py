"""Inputs of the batch-reduce tests (dgrep_reduce_batch / _device): one buffer,
a segment table and nparts; segment g belongs to partition g % nparts. Shared by
tests/test_reduce_batch_emulation.py (CPU) and tests/test_gpu_reduce_batch.py.
The expected result is stated through go_json.reduce_reference alone, one
partition's concatenated input at a time."""
import random
from collections import namedtuple

import fnv64_collisions as F
import go_json as G
import reduce_cases as R

NL_BLOCK = 256 << 10  # the newline passes' block (reduce_common.h kSeg)

Case = namedtuple("Case", "name data seg_off nparts")
Expected = namedtuple("Expected", "outputs lines_in bad")  # bad: None or (partition, 1-based line)


def from_segments(name, segs, nparts) -> Case:
    assert len(segs) % nparts == 0 and len(segs) > 0
    off = [0]
    for s in segs:
        off.append(off[-1] + len(s))
    return Case(name, b"".join(segs), off, nparts)


def segments(case):
    return [case.data[a:b] for a, b in zip(case.seg_off, case.seg_off[1:])]


def partition_inputs(case):
    """what reduce task p reads: its segments in ascending g, concatenated"""
    segs = segments(case)
    return [b"".join(segs[p::case.nparts]) for p in range(case.nparts)]


def expected(case) -> Expected:
    """Per partition reduce_reference(its concatenated input). Malformed: the
    lowest partition that has a line outside the accepted form or a non-empty
    segment without a final '\\n' (even where the fused line would parse); its
    line = the lower of reduce_reference's bad line and the unfinished line's
    number, 1 + the '\\n' of the partition's input up to that segment's end."""
    segs = segments(case)
    outs, lines = [], []
    for p, data in enumerate(partition_inputs(case)):
        ref = G.reduce_reference(data)
        cand = [ref.bad_line] if ref.bad_line is not None else []
        seen = 0
        for s in segs[p::case.nparts]:
            seen += s.count(b"\n")
            if s and not s.endswith(b"\n"):
                cand.append(seen + 1)
                break
        if cand:
            return Expected(None, None, (p, min(cand)))
        outs.append(ref.output)
        lines.append(data.count(b"\n"))
    return Expected(outs, lines, None)


def plain_line(key: bytes, value: bytes) -> bytes:
    return R.kv_line(key, value)


def random_lines(rnd, count, keys=40):
    """Lines over a small key pool (so keys repeat within and across
    partitions): keys and values of every raw length 0..9, every fifth line
    respelled (reduce_cases.SPELLINGS), every seventh with an invalid byte
    sequence (reduce_cases.INVALID) in its value."""
    pool = [R.random_atoms(rnd, j % 10, j % 10, plain_bias=0.8) for j in range(keys)]
    out = []
    for i in range(count):
        ka = pool[rnd.randrange(keys)]
        va = R.random_atoms(rnd, i % 10, i % 10)
        k = R.respell(ka, rnd) if i % 5 == 0 else R.canonical(ka)
        v = R.respell(va, rnd) if i % 5 == 1 else R.canonical(va)
        if i % 7 == 3:
            v += R.INVALID[i % len(R.INVALID)]
        out.append(R.kv_line(k, v))
    return out


def dealt(name, seed, nparts, k, count, empty=()):
    """`count` random lines dealt at random over k * nparts segments (line order
    kept inside a segment); the segments listed in `empty` get none."""
    rnd = random.Random(seed)
    nseg = k * nparts
    open_segs = [g for g in range(nseg) if g not in set(empty)]
    segs = [[] for _ in range(nseg)]
    for line in random_lines(rnd, count):
        segs[rnd.choice(open_segs)].append(line)
    return from_segments(name, [b"".join(s) for s in segs], nparts)


def kept_runs():
    """Partitions with 63, 64 and 65 kept lines (each key twice, so half the
    lines go), then 30 partitions with 1 kept line, two of them from two lines:
    writer waves span partitions."""
    segs = []
    for p, kept in enumerate((63, 64, 65)):
        lines = [plain_line(b"p%d-%d" % (p, i), b"v" * (i % 10)) for i in range(kept)]
        segs.append(b"".join(lines + [plain_line(b"p%d-%d" % (p, i), b"second") for i in range(kept)]))
    for p in range(30):
        one = plain_line(b"k", b"x" * (p % 10))
        segs.append(one + (plain_line(b"k", b"again") if p % 15 == 0 else b""))
    return from_segments("kept-63-64-65-then-ones", segs, 33)


def phases():
    """keys and values of every length 0..9, one line per segment of one
    partition each: partition starts and line edges on every dword phase"""
    segs = []
    for kl in range(10):
        for vl in range(10):
            segs.append(plain_line((b"%d" % (kl * 10 + vl)).rjust(kl, b"k")[:kl], b"v" * vl))
    return from_segments("phases-0-9", segs, 50)  # 100 segments: k = 2


def block_edge(delta):
    """segment 0 ends exactly at the newline block's edge + delta; nparts 2"""
    lines, size = [], 0
    i = 0
    while size < NL_BLOCK + delta - 200:
        lines.append(plain_line(b"e%d" % (i % 5000), b"v" * (i % 10)))
        size += len(lines[-1])
        i += 1
    pad = NL_BLOCK + delta - size - len(plain_line(b"pad", b""))
    assert 0 <= pad < 200
    lines.append(plain_line(b"pad", b"p" * pad))
    seg0 = b"".join(lines)
    assert len(seg0) == NL_BLOCK + delta
    others = [plain_line(b"e%d" % j, b"other") for j in range(0, 300, 7)]
    seg2 = seg0[:seg0.find(b"\n", 1000) + 1]  # partition 0 again: every key a duplicate
    return from_segments("block-edge%+d" % delta, [seg0, b"".join(others), seg2, b"".join(others[:20])], 2)


def sparse_65535():
    segs = [b""] * 65535
    for p in (0, 1, 2, 40000, 65533, 65534):
        segs[p] = plain_line(b"same", b"%d" % p) + plain_line(b"same", b"dup") + plain_line(b"p%d" % p, b"")
    return from_segments("nparts-65535", segs, 65535)


def new_rules():
    rnd = random.Random(5)
    atoms = [b"/", b"a", "é".encode(), b"<", R.FFFD]
    a, b = R.canonical(atoms), R.respell(atoms, rnd)
    while b == a:
        b = R.respell(atoms, rnd)
    segs = [
        plain_line(b"both", b"p0") + R.kv_line(a, b"first"),  # (0, 0)
        plain_line(b"both", b"p1"),                            # (0, 1)
        plain_line(b"both", b"p0 again") + R.kv_line(b, b"second spelling") + plain_line(b"new", b"n"),  # (1, 0)
        R.kv_line(b, b"p1 spelled") + plain_line(b"both", b"p1 again"),                                  # (1, 1)
    ]
    return from_segments("new-rules", segs, 2)


def good_cases():
    one = plain_line(b"k", b"v")
    cases = [dealt("dealt-n%d-k%d" % (nparts, k), 100 * nparts + k, nparts, k, 600)
             for nparts in (1, 2, 3, 10, 64) for k in (1, 2, 3)]
    cases += [
        dealt("dealt-n3-k257", 7, 3, 257, 3000),
        dealt("dealt-n10-k257", 8, 10, 257, 1500),
        dealt("empty-first-last-runs", 9, 4, 3, 200, empty=(0, 1, 2, 5, 6, 7, 11)),
        from_segments("all-empty", [b""] * 6, 3),
        from_segments("all-empty-one", [b""], 1),
        from_segments("one-line", [one], 1),
        from_segments("one-line-among-empty", [b"", b"", one, b"", b"", b""], 3),
        sparse_65535(), kept_runs(), phases(), new_rules(),
        block_edge(-1), block_edge(0), block_edge(1),
    ]
    # different keys with one 64-bit hash, within and across partitions (fnv64_collisions.py)
    cases += [from_segments(name, segs, nparts) for name, segs, nparts in F.batch_segments()]
    return cases


def bad_cases():
    """(case, agrees): agrees = reduce_reference of the reported partition's
    input reports the same line (false only where the fused line parses)"""
    good = [plain_line(b"g%d" % i, b"v") for i in range(5)]
    clean = b"".join(good)
    head, tail = b'{"Key":"a","Val', b'ue":"b"}\n'
    return [
        (from_segments("bad-line-partition-2", [clean, clean, good[0] + b"not json\n" + good[1], clean, clean,
                                                 good[2]], 3), True),
        (from_segments("bad-in-two-partitions", [clean, good[0] + good[1] + b'{"Value":"b","Key":"a"}\n', clean,
                                                 b"{}\n" + clean, b"x\n", clean], 3), True),
        (from_segments("no-final-newline", [clean, clean + good[0][:-1]], 2), True),
        (from_segments("no-final-newline-then-more", [clean, clean[:-1], clean, clean], 2), True),
        (from_segments("split-line-pair-two-partitions", [clean + head, tail + clean], 2), True),
        (from_segments("split-line-pair-one-partition", [clean + head, tail + clean], 1), False),
        (from_segments("split-line-pair-same-partition-of-two", [clean + head, b"", tail, clean], 2), False),
        (from_segments("bytes-without-newline", [b"", b"abc"], 2), True),
        (from_segments("lower-partition-later-in-buffer", [clean, b"zzz", clean + b"bad\n", clean], 2), True),
    ]
