"""tests/golden/fnv64_collisions.json and everything tests/fnv64_collisions.py
builds from it, verified without a GPU and without trust in the tool that found
the keys: every family's members differ, share one hash under the suite's
fnv64 (test_reduce_batch_emulation.py, the kernels' constants), need no JSON
escape; the derived keys still collide once decoded; and every built input has
exactly the distinct keys its construction intends (go_json.reduce_reference)."""
import random

import pytest

import fnv64_collisions as F
import go_json as G
import job_window_cases as J
import oracle_lib as O
import reduce_batch_cases as B
import reduce_cases as R
from test_reduce_batch_emulation import fnv64

FAMILY_NAMES = list(F.FAMILIES)
SINGLE = F.single_inputs()


def _decoded_keys(data: bytes):
    return [G.parse_kv_line(line)[0] for line in data.split(b"\n")[:-1]]


def test_the_fixture_covers_what_the_cases_need():
    assert fnv64(b"") == F.FNV64_INIT == int(F.FIXTURE["initial_state"], 16)
    assert {len(F.FAMILIES[n]) for n in ("pair", "four", "eight")} == {2, 4, 8}
    assert len(set(map(len, F.PAIR))) == 1 and len(set(map(len, F.EIGHT))) == 1
    assert len(set(map(len, F.MIXED))) == 2 and len(set(map(len, F.MIXED_FOUR))) == 2
    a, b = F.PREFIXED
    common = next(i for i in range(len(a)) if a[i] != b[i])
    assert common == 70 and len(a) == len(b)  # the first difference is past byte 64
    for s in F.FIXTURE["searches"]:  # what the summary of the search records
        assert s["threads"] <= 16 and s["seconds"] > 0 and 28 < s["log2_evaluations"] < 36


@pytest.mark.parametrize("name", list(F.SEARCHES))
def test_every_search_result_collides_from_its_state(name):
    s = F.SEARCHES[name]
    state = int(s["from_state"], 16)
    assert fnv64(s["prefix"].encode()) == state or (not s["prefix"] and state != F.FNV64_INIT)
    x, y = (k.encode() for k in s["keys"])
    assert x != y
    assert F.fnv64(x, state) == F.fnv64(y, state) == int(s["hash"], 16)


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_family_members_differ_and_collide(name):
    fam = F.FAMILIES[name]
    assert len(set(fam)) == len(fam) >= 2
    assert len({fnv64(k) for k in fam}) == 1
    assert all(F.fnv64(k) == fnv64(k) for k in fam)
    last = F.SEARCHES[F.FIXTURE["families"][name][-1]]
    assert fnv64(fam[0]) == int(last["hash"], 16)
    for k in fam:  # bytes a JSON string carries raw, and json.Encoder leaves alone
        assert all(0x20 <= c < 0x7F and c not in b'"\\<>&' for c in k), k
        assert G.unquote(k + b'"') == (k, len(k) + 1)
        assert G.parse_kv_line(R.kv_line(k, b"v")[:-1]) == (k, b"v")


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_derived_keys_still_collide_after_decoding(name):
    fam = F.FAMILIES[name]
    rnd = random.Random(len(name))
    for suffix in (b" (line number #1)", b" (line number #4294967295)", b"s" * 200, R.FFFD + b"t", b""):
        assert len({fnv64(k + suffix) for k in fam}) == 1
    for raw_len in (63, 64, 65, 200):
        if raw_len > max(map(len, fam)):
            ext = F.extended(fam, raw_len)
            assert max(map(len, ext)) == raw_len and len(set(ext)) == len(fam) and len({fnv64(k) for k in ext}) == 1
    # behind a common prefix they collide only from the prefix's state: NOT in general
    assert len({fnv64(b"p" + k) for k in fam}) == len(fam)
    for k in fam:
        sp = F.spellings(k)
        assert len(set(sp)) == 4 and sp[0] == k
        for s in sp:  # another spelling, the same decoded key, hence the same hash
            assert G.unquote(s + b'"') == (k, len(s) + 1)
        assert sp[3].startswith(k[:-1]) and sp[3] != k  # agrees with the canonical one up to its last unit
        atoms = [b"/", b"a", "é".encode(), b"<", R.FFFD, b'"', b"7"]
        raw = k + b"".join(atoms)
        for _ in range(4):
            s = k + R.respell(atoms, rnd)
            assert G.unquote(s + b'"')[0] == raw and fnv64(raw) == fnv64(fam[0] + b"".join(atoms))


@pytest.mark.parametrize("inp", SINGLE, ids=[i.name for i in SINGLE])
def test_single_inputs_hold_the_keys_they_intend(inp):
    ref = G.reduce_reference(inp.data)
    assert ref.bad_line is None
    assert len(ref.kv) == inp.nkeys
    assert ref.output.count(b"\n") == inp.nkeys < inp.data.count(b"\n")  # a duplicate in every input
    keys = _decoded_keys(inp.data)
    if inp.name != "crowd":  # one equal-hash run: every line meets every earlier one
        assert len({fnv64(k) for k in keys}) == 1
    else:
        runs = {}
        for k in keys:
            runs.setdefault(fnv64(k), set()).add(k)
        assert sorted(len(v) for v in runs.values())[-2:] == [4, 4] and len(inp.data.split(b"\n")) > 2000
        assert ref.output.count(b"\n") > 10 * 64  # kept lines over many writer waves


def test_single_inputs_cover_the_verdicts():
    by = {i.name: i for i in SINGLE}
    # the length check: neighbours in the run with different decoded lengths, the equal further back
    keys = _decoded_keys(by["mixed-long-first-xyxy"].data)
    assert len(keys[2]) != len(keys[1]) and keys[2] == keys[0]
    # three unequal entries between a line and its equal
    keys = _decoded_keys(by["four-abcd-0"].data)
    assert keys[4] == keys[0] and len({keys[1], keys[2], keys[3], keys[0]}) == 4
    # an escaped spelling whose nearest earlier line is the other key, at equal decoded length
    lines = by["pair-ab-spellings"].data.split(b"\n")[:-1]
    keys = _decoded_keys(by["pair-ab-spellings"].data)
    assert b"\\u00" in lines[2] and b"\\u00" in lines[1] and keys[2] != keys[1] and len(keys[2]) == len(keys[1])
    assert keys[2] == keys[0] and lines[2] != lines[0]
    # first difference past byte 64, with and without a suffix; every length on both sides of 64
    assert {n for i in SINGLE for n in (63, 64, 65, 200) if i.name.endswith("-to-%d" % n)} == {63, 64, 65, 200}
    keys = _decoded_keys(by["prefixed-as-it-is"].data)
    assert keys[0][:70] == keys[1][:70] and keys[0][70] != keys[1][70]
    # the coerced byte: the line is not plain, the decoded keys are two
    assert b"\xff" in by["pair-invalid-byte-in-suffix"].data
    assert len(set(_decoded_keys(by["pair-invalid-byte-in-suffix"].data))) == 2


def test_batch_cases_are_in_the_shared_list_and_mix_partitions():
    good = {c.name: c for c in B.good_cases()}
    for name, segs, nparts in F.batch_segments():
        case = good[name]
        assert B.segments(case) == segs and case.nparts == nparts
        want = B.expected(case)
        assert want.bad is None
    one = [set(_decoded_keys(x)) for x in B.partition_inputs(good["collide-one-partition-two-segments"])]
    assert set(F.PAIR) <= one[0] and F.PAIR[0] in one[1] and F.PAIR[1] not in one[1]
    segs = B.segments(good["collide-one-partition-two-segments"])
    assert F.PAIR[0] in _decoded_keys(segs[0]) and F.PAIR[1] in _decoded_keys(segs[2])
    a, b = F.PAIR
    p0, p1 = (set(_decoded_keys(x)) for x in B.partition_inputs(good["collide-across-partitions"]))
    assert a in p0 and b not in p0 and b in p1 and a not in p1
    for name, fam in (("collide-four-over-3-partitions", F.FOUR), ("collide-mixed-four-over-3-partitions",
                                                                   F.MIXED_FOUR)):
        want = B.expected(good[name])
        for p, data in enumerate(B.partition_inputs(good[name])):
            keys = _decoded_keys(data)
            assert all(keys.count(k) == 2 for k in fam), (name, p)  # duplicates in every partition
            assert want.outputs[p].count(b"\n") == 4 + len({k for k in keys if k.startswith(b"other")})


@pytest.mark.parametrize("fam,nreduce", [("pair", 1), ("pair", 2), ("pair", 3), ("four", 1), ("four", 2), ("four", 3),
                                         ("mixed-four", 3)])
def test_job_files_put_colliding_keys_into_one_partition(fam, nreduce):
    names = F.FAMILIES[fam]
    files, shared = F.job_files(names, nreduce, big=names[1], big_bytes=J.WINDOWS[0])
    assert len(shared) >= 3, shared
    for n in shared:
        keys = [F.job_key(f, n) for f in names]
        assert len({fnv64(k) for k in keys}) == 1 and len(set(keys)) == len(names)
        assert len({F.ihash(k) % nreduce for k in keys}) == 1
        assert all(F.ihash(k) == O.ihash(k) for k in keys) and keys[0] == O.format_key(names[0], n)
    assert [f for f, _ in files] == names + names[::-1]
    sizes = {f: len(d) for f, d in files[:len(names)]}
    assert sizes[names[1]] > J.WINDOWS[0] and all(v <= J.WINDOWS[0] for f, v in sizes.items() if f != names[1])
    assert all(len(d) <= J.WINDOWS[0] for _, d in files[len(names):])
    for _, d in files:
        lines = d.split(b"\n")
        assert all(b"error" in lines[n - 1] for n in shared)
