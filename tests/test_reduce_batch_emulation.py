"""The batch reduce's pipeline (csrc/kernels/reduce_batch.hip), restated in
numpy and checked against go_json.reduce_reference on every case of
reduce_batch_cases -- the algorithm pinned where there is no GPU:

* newline positions over the whole buffer;
* line -> segment: the last segment that starts at or before the line's '\\n'
  (an upper bound in seg_off, which skips empty segments), partition = segment
  % nparts; a line starts after the previous '\\n' or at its segment's start;
* placement: a stable sort of the line ids by partition; the partitions' first
  lines by lower bound;
* malformed input: the lowest (partition, line) over the lines that do not
  parse and over the segments without a final '\\n' (the line after the
  partition's lines that end before the segment's end);
* grouping: a sort by (FNV-1a 64 of the decoded key, line); inside an
  equal-hash run a line walks back over the earlier lines and is dropped at
  the first one of the SAME partition with the same decoded key, decided as the
  kernels decide it: decoded length, then the escaped bytes, then the decoded
  keys (the collide-* cases are different keys with one hash, which take the
  walk past unequal entries and every "different" verdict);
* an exclusive sum of the kept lengths in placed order, part_off read from it.

The line language itself (go_json.parse_kv_line here) is tested elsewhere."""
import numpy as np
import pytest

import go_json as G
import reduce_batch_cases as C

GOOD = C.good_cases()
BAD = C.bad_cases()


def fnv64(b: bytes) -> int:
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _escaped_equal(s: bytes, aj: int, ak: int) -> bool:
    """the dedupe kernels' first compare: the keys' escaped bytes, from the
    lines' starts up to the closing quote (the byte after a backslash is
    compared and skipped, so an escaped quote does not end it)"""
    t = 8
    while True:
        x = s[aj + t]
        if x != s[ak + t]:
            return False
        if x == 0x22:
            return True
        if x == 0x5C:
            t += 1
            if s[aj + t] != s[ak + t]:
                return False
        t += 1


def emulate(case) -> C.Expected:
    data, nparts = case.data, case.nparts
    seg_off = np.asarray(case.seg_off, np.int64)
    nseg = len(seg_off) - 1
    buf = np.frombuffer(data, np.uint8)
    nl = np.flatnonzero(buf == 10).astype(np.int64)
    L = len(nl)
    seg = np.searchsorted(seg_off[:nseg + 1], nl, side="right") - 1
    part = (seg % nparts).astype(np.int64)
    start = np.maximum(np.concatenate(([0], nl[:-1] + 1)) if L else nl, seg_off[seg])
    parsed = [G.parse_kv_line(data[a:e]) for a, e in zip(start.tolist(), nl.tolist())]
    flagged = np.array([p is None for p in parsed], bool)
    # placement
    order = np.argsort(part, kind="stable")
    part_sorted = part[order]
    line_start = np.searchsorted(part_sorted, np.arange(nparts + 1), side="left")
    lines_in = np.diff(line_start).tolist()
    # the first malformed line
    bad = []
    for q in np.flatnonzero(flagged[order]).tolist():
        p = int(part_sorted[q])
        bad.append((p << 34) | ((q - int(line_start[p])) << 1) | 1)
    ends = nl[order]
    for g in range(nseg):
        b, e = int(seg_off[g]), int(seg_off[g + 1])
        if e == b or data[e - 1] == 10:
            continue
        p = g % nparts
        lo, hi = int(line_start[p]), int(line_start[p + 1])
        q = lo + int(np.searchsorted(ends[lo:hi], e, side="left"))
        bad.append((p << 34) | ((q - lo) << 1))
    if bad:
        key = min(bad)
        return C.Expected(None, None, (key >> 34, ((key >> 1) & ((1 << 33) - 1)) + 1))
    # grouping
    h = np.array([fnv64(p[0]) for p in parsed], np.uint64)
    by_hash = np.lexsort((np.arange(L), h))
    keep = np.ones(L, bool)
    for q in range(L):
        j = by_hash[q]
        t = q
        while t > 0 and h[by_hash[t - 1]] == h[j]:
            t -= 1
            k = by_hash[t]
            if part[k] != part[j]:
                continue  # the same key in another partition is another key
            if len(parsed[k][0]) != len(parsed[j][0]):
                continue
            same = _escaped_equal(data, int(start[j]), int(start[k]))
            if not same:  # another spelling of the same key, or another key with this hash and length
                same = parsed[k][0] == parsed[j][0]
            if same:
                keep[j] = False
                break
    # placement of the kept lines
    out_len = np.array([len(p[0]) + len(p[1]) + 2 if kp else 0 for p, kp in zip(parsed, keep)], np.int64)
    plen = out_len[order]
    ppos = np.concatenate(([0], np.cumsum(plen)[:-1])) if L else plen
    total = int(plen.sum())
    part_off = [int(ppos[q]) if q < L else total for q in line_start.tolist()]
    out = bytearray(total)
    for q in range(L):
        if plen[q]:
            k, v = parsed[order[q]]
            out[ppos[q]:ppos[q] + plen[q]] = k + b" " + v + b"\n"
    assert part_off[0] == 0 and part_off[-1] == total
    return C.Expected([bytes(out[a:b]) for a, b in zip(part_off, part_off[1:])], lines_in, None)


@pytest.mark.parametrize("case", GOOD, ids=[c.name for c in GOOD])
def test_pipeline_matches_reference(case):
    want = C.expected(case)
    assert want.bad is None
    got = emulate(case)
    assert got.bad is None
    assert got.lines_in == want.lines_in
    assert got.outputs == want.outputs


@pytest.mark.parametrize("case,agrees", BAD, ids=[c.name for c, _ in BAD])
def test_first_malformed_line(case, agrees):
    want = C.expected(case)
    assert want.bad is not None
    p, line = want.bad
    ref = G.reduce_reference(C.partition_inputs(case)[p])
    # the lower partitions are clean; this one's reference agrees unless the fused line parses
    assert all(G.reduce_reference(x).bad_line is None for x in C.partition_inputs(case)[:p])
    assert (ref.bad_line == line) == agrees
    assert emulate(case).bad == want.bad


def test_cases_cover_what_they_claim():
    names = {c.name for c in GOOD}
    assert len(names) == len(GOOD)
    by = {c.name: c for c in GOOD}
    assert {c.nparts for c in GOOD} >= {1, 2, 3, 10, 64, 65535}
    assert {(len(c.seg_off) - 1) // c.nparts for c in GOOD} >= {1, 2, 3, 257}
    for d in (-1, 0, 1):
        assert by["block-edge%+d" % d].seg_off[1] == C.NL_BLOCK + d
    kept = [o.count(b"\n") for o in C.expected(by["kept-63-64-65-then-ones"]).outputs]
    assert kept[:3] == [63, 64, 65] and set(kept[3:]) == {1}
    rules = C.expected(by["new-rules"])
    assert rules.outputs[0].count(b"both p0\n") == 1 and rules.outputs[1].count(b"both p1\n") == 1
    assert b"first\n" in rules.outputs[0] and b"second spelling" not in rules.outputs[0]
    assert b"p1 spelled\n" in rules.outputs[1]
    sparse = C.expected(by["nparts-65535"])
    assert sum(1 for o in sparse.outputs if o) == 6
