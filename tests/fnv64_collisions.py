"""Different keys with one 64-bit hash, and the reduce inputs made of them.

The reduce groups lines by the FNV-1a 64 of the decoded key and settles equal
hashes with an exact compare (reduce.hip dedupe_kernel, reduce_batch.hip
dedupe_batch_kernel): a length check, a compare of the escaped bytes, a compare
of the decoded keys. Only keys that differ AND share a hash reach that compare's
"different" verdicts. tests/golden/fnv64_collisions.json holds such keys (found
by tools/fnv64_collide.cpp); this module loads them and builds the inputs of
tests/test_gpu_reduce_collisions.py and the batch cases of reduce_batch_cases.
tests/test_fnv64_collisions.py (no GPU) verifies every family and every input.

Two keys that collide from a state still collide before any common suffix, and
pairs searched from one another's common hash chain into 4 and 8 keys.
No GPU, no library: go_json and reduce_cases only."""
import itertools
import json
import os
import random
from collections import namedtuple

import go_json as G
import reduce_cases as R
from reduce_cases import kv_line

FNV64_INIT = 1469598103934665603  # reduce_common.h json_string
FNV64_PRIME = 1099511628211
M64 = (1 << 64) - 1


def fnv64(b: bytes, h: int = FNV64_INIT) -> int:
    for x in b:
        h = ((h ^ x) * FNV64_PRIME) & M64
    return h


def ihash(key: bytes) -> int:
    """the reference's partition hash (worker.go ihash): FNV-1a 32 & 0x7fffffff"""
    h = 2166136261
    for x in key:
        h = ((h ^ x) * 16777619) & 0xFFFFFFFF
    return h & 0x7FFFFFFF


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fnv64_collisions.json")) as _f:
    FIXTURE = json.load(_f)
SEARCHES = {s["name"]: s for s in FIXTURE["searches"] + FIXTURE["recorded"]}


def _family(chain):
    """the product of the chained pairs behind the first one's prefix"""
    first = SEARCHES[chain[0]]
    keys = [first["prefix"].encode()]
    for name in chain:
        keys = [k + part.encode() for k in keys for part in SEARCHES[name]["keys"]]
    return keys


FAMILIES = {name: _family(chain) for name, chain in FIXTURE["families"].items()}
PAIR, FOUR, EIGHT = FAMILIES["pair"], FAMILIES["four"], FAMILIES["eight"]
MIXED, MIXED_FOUR, PREFIXED = FAMILIES["mixed"], FAMILIES["mixed-four"], FAMILIES["prefixed"]

Input = namedtuple("Input", "name data nkeys")  # nkeys: the distinct keys the construction intends


def u00(byte: int) -> bytes:
    return b"\\u%04x" % byte


def escaped_at(key: bytes, i: int) -> bytes:
    """key with byte i (negative: from the end) spelled \\u00XX"""
    i %= len(key)
    return key[:i] + u00(key[i]) + key[i + 1:]


def spellings(key: bytes):
    """the canonical spelling, then \\u00XX for the first, a middle and the last byte"""
    return [key, escaped_at(key, 0), escaped_at(key, len(key) // 2), escaped_at(key, -1)]


def extended(family, raw_len: int, fill: bytes = b"s"):
    """the family before a common suffix; the longest member gets raw_len bytes"""
    suffix = fill * (raw_len - max(map(len, family)))
    assert suffix
    return [k + suffix for k in family]


def _lines(name, spelled_keys, nkeys) -> Input:
    """one line per spelled key, the value naming the line"""
    return Input(name, b"".join(kv_line(k, b"v%d" % i) for i, k in enumerate(spelled_keys)), nkeys)


# ---- single reduce ---------------------------------------------------------------------
def stay_apart():
    """A B A B and B A B A for every two-key family of one length"""
    out = []
    for fam in ("pair", "prefixed"):
        a, b = FAMILIES[fam]
        out += [_lines("%s-abab" % fam, [a, b, a, b], 2), _lines("%s-baba" % fam, [b, a, b, a], 2)]
    return out


def different_lengths():
    """the mixed-length pairs: the duplicate's equal is not its neighbour"""
    out = []
    for fam in ("mixed", "recorded-mixed"):
        for tag, (x, y) in (("long-first", FAMILIES[fam]), ("short-first", FAMILIES[fam][::-1])):
            assert len(x) != len(y)
            for shape in ("xyxy", "xyyx", "xyyyx", "xxyx"):
                out.append(_lines("%s-%s-%s" % (fam, tag, shape), [{"x": x, "y": y}[c] for c in shape], 2))
    return out


def walk_past():
    """4 keys: every order of the first occurrences, the second occurrences in
    another order; A B C D A; 8 keys: seeded orders and A..H A"""
    out = []
    for fam in ("four", "mixed-four", "recorded-four"):
        keys = FAMILIES[fam]
        for n, perm in enumerate(itertools.permutations(range(4))):
            second = perm[n % 3 + 1:] + perm[:n % 3 + 1] if n % 2 else perm[::-1]
            assert second != perm
            out.append(_lines("%s-perm%d" % (fam, n), [keys[i] for i in perm + tuple(second)], 4))
        for last in range(4):
            out.append(_lines("%s-abcd-%d" % (fam, last), keys + [keys[last]], 4))
    rnd = random.Random(8)
    for n in range(6):
        first, second = rnd.sample(EIGHT, 8), rnd.sample(EIGHT, 8)
        out.append(_lines("eight-perm%d" % n, first + second, 8))
    out.append(_lines("eight-a-h-a", EIGHT + [EIGHT[0]], 8))
    return out


def respelled():
    """A and B in four spellings each. An escaped spelling meets the OTHER key
    first; A' against B' is decided "different" by the decoded compare, A'
    against A "same"; the canonical and the last-byte-escaped spelling of one
    key agree up to their last unit; equal escaped spellings (an escape at the
    same place in both) stop in the escaped compare."""
    out = []
    for fam in ("pair", "prefixed", "mixed"):
        for tag, (a, b) in (("ab", FAMILIES[fam]), ("ba", FAMILIES[fam][::-1])):
            sa, sb = spellings(a), spellings(b)
            order = [sa[0], sb[1], sa[1], sb[0], sb[2], sa[2], sa[3], sb[3], sa[0], sb[0], sa[1], sb[1], sb[3], sa[3]]
            out.append(_lines("%s-%s-spellings" % (fam, tag), order, 2))
            out.append(_lines("%s-%s-escaped-first" % (fam, tag), [sa[1], sb[1], sa[2], sb[2], sb[0], sa[0]], 2))
            out.append(_lines("%s-%s-last-unit" % (fam, tag), [sb[0], sa[0], sa[3], sb[3], sa[0]], 2))
    # a common suffix of reduce_cases atoms, respelled at random behind every member
    rnd = random.Random(64)
    atoms = [b"/", b"a", "é".encode(), b"<", R.FFFD, b" ", b'"', "\U0001F600".encode(), b"7"]
    for fam in ("four", "mixed-four"):
        lines = [k + R.canonical(atoms) for k in FAMILIES[fam]]
        for _ in range(5):
            lines += [k + R.respell(atoms, rnd) for k in rnd.sample(FAMILIES[fam], 4)]
        out.append(_lines("%s-respelled-suffix" % fam, lines, 4))
    return out


def long_keys():
    """every family before a common suffix, to 63, 64, 65 and 200 raw bytes (the
    prefixed pair as it is: it first differs past byte 64), members then members
    reversed; and members that carry a raw invalid byte in the common suffix"""
    out = []
    for fam, keys in FAMILIES.items():
        for raw_len in (63, 64, 65, 200):
            if max(map(len, keys)) >= raw_len:
                continue
            ext = extended(keys, raw_len)
            out.append(_lines("%s-to-%d" % (fam, raw_len), ext + ext[::-1], len(keys)))
    out.append(_lines("prefixed-as-it-is", PREFIXED + PREFIXED[::-1], 2))
    for fam in ("pair", "mixed", "prefixed"):
        a, b = FAMILIES[fam]
        tail = b"t" * 60
        # raw \xff, the escape and the raw rune all decode to U+FFFD: two keys
        spelled = [a + b"\xff" + tail, b + b"\xff" + tail, b + b"\\ufffd" + tail, a + R.FFFD + tail,
                   a + b"\xfe" + tail, b + b"\x80" + tail]
        out.append(_lines("%s-invalid-byte-in-suffix" % fam, spelled, 2))
    return out


def crowd():
    """the 4-way and the mixed 4-way family among 700 unrelated keys, about 2000
    lines: the runs sit inside a real sort, the kept lines span many waves"""
    rnd = random.Random(2000)
    lines = [kv_line(b"crowd-%d" % (i % 700), b"value %d" % i) for i in range(1900)]
    lines += [kv_line(b"crowd\\u002d%d" % i, b"respelled %d" % i) for i in range(0, 700, 7)]
    rnd.shuffle(lines)
    for fam in (FOUR, MIXED_FOUR):
        fam_lines = [kv_line(k, b"%s %d" % (k[:4], n)) for n in range(4) for k in rnd.sample(fam, 4)]
        at = sorted(rnd.sample(range(len(lines)), len(fam_lines)), reverse=True)
        for pos, line in zip(at, reversed(fam_lines)):  # from the back: the family's own order is kept
            lines.insert(pos, line)
    return [Input("crowd", b"".join(lines), 708)]


def single_inputs():
    out = stay_apart() + different_lengths() + walk_past() + respelled() + long_keys() + crowd()
    assert len({i.name for i in out}) == len(out)
    return out


# ---- batch reduce: (name, segments, nparts); segment g belongs to partition g % nparts ------
def batch_segments():
    a, b = PAIR
    m1, m2 = MIXED
    line = kv_line
    same_partition = [
        line(a, b"a seg0") + line(b"x", b"1") + line(m1, b"m1 seg0"),  # (0, 0)
        line(b"y", b"2") + line(a, b"a in p1"),                         # (0, 1)
        line(b, b"b seg2") + line(a, b"a again") + line(m2, b"m2 seg2") + line(b, b"b again") +
        line(escaped_at(a, 3), b"a respelled") + line(m1, b"m1 again"),  # (1, 0)
        line(b"x", b"3"),                                               # (1, 1)
    ]
    across = [
        line(a, b"a first") + line(a, b"a dup") + line(m1, b"m1"),  # (0, 0)
        line(b, b"b first") + line(b, b"b dup") + line(m2, b"m2"),  # (0, 1)
        line(m1, b"m1 dup") + line(a, b"a dup 2"),                   # (1, 0)
        line(escaped_at(b, -1), b"b dup 2") + line(m2, b"m2 dup"),   # (1, 1)
    ]
    out = [("collide-one-partition-two-segments", same_partition, 2), ("collide-across-partitions", across, 2)]
    for name, fam, seed in (("collide-four-over-3-partitions", FOUR, 43), ("collide-mixed-four-over-3-partitions",
                                                                            MIXED_FOUR, 44)):
        rnd = random.Random(seed)
        segs = [[] for _ in range(6)]
        for p in range(3):  # every key twice in every partition, in either of its two segments
            for n, k in enumerate(rnd.sample(fam, 4) + rnd.sample(fam, 4)):
                spelled = k if n < 5 else escaped_at(k, rnd.randrange(len(k)))
                segs[p + 3 * rnd.randrange(2)].append(line(spelled, b"p%d n%d" % (p, n)))
        for g in range(6):
            segs[g].insert(rnd.randrange(len(segs[g]) + 1), line(b"other-%d" % (g % 2), b"o"))
        out.append((name, [b"".join(s) for s in segs], 3))
    return out


# ---- whole job: files named by family members ---------------------------------------------
def job_key(name: bytes, line_no: int) -> bytes:
    """grep.go Map: the key of line line_no of file name"""
    return name + b" (line number #%d)" % line_no


def shared_lines(names, nreduce, upto):
    """the line numbers 1..upto at which the keys of all the names fall into one partition"""
    return [n for n in range(1, upto + 1) if len({ihash(job_key(f, n)) % nreduce for f in names}) == 1]


def job_files(names, nreduce, nlines=240, big=None, big_bytes=0):
    """(files, shared): one file per name, then each name again (other values:
    duplicate keys), every file matching `error` on the same lines: every third
    line and every line of shared_lines. The file named `big` is padded with
    non-matching bytes past big_bytes."""
    shared = shared_lines(names, nreduce, nlines)
    hit = set(shared) | set(range(1, nlines + 1, 3))
    files = []
    for rep, order in enumerate((names, names[::-1])):
        for f in order:
            body = b"".join(b"error %d.%d\n" % (rep, n) if n in hit else b"-\n" for n in range(1, nlines + 1))
            if f == big and rep == 0:
                pad = b"quiet " * 9 + b"\n"  # lines after nlines, without a match
                body += pad * ((big_bytes - len(body)) // len(pad) + 1)
            files.append((f, body))
    return files, shared
