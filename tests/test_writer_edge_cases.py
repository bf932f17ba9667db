"""tests/writer_edge_cases.py on the CPU: the generators hold what they claim;
the oracle's escaping of invalid UTF-8 (each bad byte becomes \\ufffd) agrees
with an independent witness built on Python's strict decoder; and the product's
host-compiled escapers -- json_body<true> and escape_width_at + escape_put, in
tests/escape_c's stand-alone program under ASan + UBSan -- agree with the
oracle on every value the GPU file sends through the device-compiled ones. A
mismatch in tests/test_gpu_writer_edges.py is then a device-side fault.
Nothing is loaded into Python."""
import collections
import os
import struct
import subprocess

import numpy as np

import oracle_lib as O
import window_part_cases as PC
import writer_edge_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "escape_c")


# ---- the generators ----------------------------------------------------------------
def test_short_values_and_split():
    assert C.EDGE is PC.EDGE_BYTES and len(set(C.EDGE)) == 23 and 0x0A not in C.EDGE
    values = C.short_values()
    assert len(values) == 292561 == sum(23 ** k for k in range(5)) and len(set(values)) == len(values)
    assert collections.Counter(map(len, values)) == {k: 23 ** k for k in range(5)}
    assert all(set(v) <= set(C.EDGE) for v in values)
    data = C.short_split()
    assert data.count(b"\n") == len(values) and not data.endswith(b"\n") and data.endswith(b"\xf0\x9f\x98")
    assert data.split(b"\n")[:-1] == values
    assert 1400000 < len(data) < 1500000
    files = C.cut_files(data, 7, b"short")
    assert len(files) == 7 and len({f for f, _ in files}) == 7
    at = 0
    for _, d in files:  # no file starts at an aligned offset of the split
        assert at == 0 or at % 4 != 0, at
        at += len(d) + 1


def test_de_bruijn_holds_every_4_gram_once():
    s = C.de_bruijn()
    assert len(s) == 23 ** 4 + 3 == 279844 and s[-3:] == s[:3] and set(s) == set(C.EDGE)
    grams = collections.Counter(s[i:i + 4] for i in range(len(s) - 3))
    assert len(grams) == 23 ** 4 and set(grams.values()) == {1}
    # the escaped form's length: the oracle's, the local width rule's and the witness's
    w, _ = C._de_bruijn_widths()
    assert len(C.body(s)) == int(w.sum()) == len(C.go_json_witness(s)) == 1347744
    assert set(w.tolist()) == {0, 1, 2, 3, 4, 6}


def test_long_split():
    data = C.long_split()
    long_lines = [v for v in data.split(b"\n") if len(v) >= C.LONG_VALUE]
    assert long_lines == [C.padded(p) for p in range(16)]
    assert C.chunked(data.split(b"\n")) == 16 and data.count(b"\n") == 32
    assert not any(C.needs_escape(v) for v in data.split(b"\n") if len(v) < C.LONG_VALUE)
    # every 4-gram at every phase of a 16-byte block, whatever the first line's phase
    s = C.de_bruijn()
    at = s.index(b"\xf0\x90\x80\x80")
    assert {(p + at) % 16 for p in range(16)} == set(range(16))


def test_long_split_reaches_every_class_at_every_buffer_phase():
    for shift in range(16):
        t = C.long_classes(shift)
        assert all(t[k] > 0 for k in C.LONG_CLASSES), (shift, t)
        # a scan that is only right for equal lane sums cannot pass: the lanes of a step differ
        assert t["sums"] >= 16, (shift, t)
        e = C.edge_classes(C.long_split(), shift) + C.edge_classes(C.random_split(), shift)
        assert all(e[k] > 0 for k in C.EDGE_CLASSES), (shift, e)


def test_record_cases():
    buf, recs = C.record_cases()
    assert buf == C.de_bruijn()
    n4 = len(buf) - 3
    assert len(recs) == 2 * n4 + 3 * 16384 == 608834
    ln, st, le = (recs[:, k] for k in range(3))
    for k in (3, 4):
        assert sorted(st[le == k].tolist()) == list(range(n4))
    for k in (0, 1, 2):
        assert sorted(st[le == k].tolist()) == list(range(16384))
    assert int((st + le).max()) <= len(buf)
    assert set(ln.tolist()) == set(C.LINE_NUMBERS)
    digits = np.array([len(str(v)) for v in ln[:1000].tolist()])
    assert (digits[1:] != digits[:-1]).mean() > 0.9  # neighbouring lanes: different digit counts
    # every 3-gram is a value followed in the buffer by each of the 23 bytes
    behind = collections.defaultdict(set)
    for s in st[le == 3].tolist():
        if s + 3 < len(buf):
            behind[buf[s:s + 3]].add(buf[s + 3])
    assert len(behind) == 23 ** 3 and all(b == set(C.EDGE) for b in behind.values())
    # ... among them the bytes that would complete a sequence the value's end cuts off
    assert 0x80 in behind[b"\xf0\x90\x80"] and 0xA8 in behind[b"A\xe2\x80"]


def test_random_values():
    values = C.random_values()
    assert len(values) == 2000 and values is C.random_values() and all(b"\n" not in v for v in values)
    for lo, hi, _ in C.BANDS:
        seen = {len(v) for v in values if lo <= len(v) <= hi}
        assert len(seen) >= (hi - lo + 1) * 3 // 4, (lo, hi, sorted(seen))
    assert all(any(lo <= len(v) <= hi for lo, hi, _ in C.BANDS) for v in values)
    assert {256, 4096, 16384} <= {len(v) for v in values} and max(map(len, values)) > 16384
    assert 2500000 < sum(map(len, values)) < 3500000
    every = b"".join(values)
    assert len(set(every)) == 255
    assert sum(every.count(bytes([b])) for b in C.EDGE) > len(every) // 2
    split = C.random_split().split(b"\n")
    assert split == values + [v for _, v in C.REGRESSIONS] + C.lone_values()
    plain, one_lane, chunked = C.paths(split)
    assert plain > 100 and one_lane > 1000 and chunked > 500, (plain, one_lane, chunked)


def test_lone_values():
    values = C.lone_values()
    assert len(values) == 255 * 6 and all(b"\n" not in v for v in values)
    special = lambda v: [x for x in v if C.needs_escape(bytes([x]))]
    alone = collections.Counter(special(v)[0] for v in values if len(special(v)) == 1)
    for b in range(256):
        if b != 0x0A and C.needs_escape(bytes([b])):
            assert alone[b] >= 5, b  # four short values and a long one that b alone escapes
    assert sum(1 for v in values if not special(v)) == 5 * (255 - len(alone))
    assert sum(1 for v in values if len(v) >= C.LONG_VALUE) == 255 * 2


def test_job_outputs_is_expected_job():
    import job_window_cases as JW

    data = C.lines_of([v for v in C.random_values() if len(v) < 300] + C.lone_values()[::3] + [C.padded(3)[:20000]])
    assert C.job_outputs(data, b'a "name".log', 10) == JW.expected_job(b"", [(b'a "name".log', data)], 10)


# ---- the witness against the oracle -----------------------------------------------------
def _agree(values):
    bad = [v for v in values if C.go_json_witness(v) != C.body(v)]
    assert not bad, (len(bad), bad[:3])


def test_witness_short_values():
    _agree(C.short_values())


def test_witness_every_two_byte_string():
    _agree([bytes([a, b]) for a in range(256) for b in range(256)])


def test_witness_random_and_lone_values_and_the_long_value():
    _agree(C.random_values() + C.lone_values() + [C.padded(p) for p in (0, 5)])


def test_witness_named_values():
    named = {
        b"\xef\xbf\xbd": b"\xef\xbf\xbd",                    # a literal U+FFFD: raw
        b"\xef\xbf\xbd\xff": b"\xef\xbf\xbd\\ufffd",
        b"\x08\x0c": b"\\u0008\\u000c",                      # no \b, \f short forms in Go
        b"\\b\\f\\u0041": b"\\\\b\\\\f\\\\u0041",            # a backslash followed by b, f, u
        b"\\\x08b": b"\\\\\\u0008b",
        b"\\ufffd": b"\\\\ufffd",
        b"<>&\x7f": b"\\u003c\\u003e\\u0026\x7f",
        b"\xe2\x80\xa8\xe2\x80\xa9\xe2\x80\xaa": b"\\u2028\\u2029\xe2\x80\xaa",
        b"\xed\x9f\xbf\xed\xa0\x80": b"\xed\x9f\xbf\\ufffd\\ufffd\\ufffd",
        b"\xf4\x8f\xbf\xbf\xf4\x90\x80\x80": b"\xf4\x8f\xbf\xbf\\ufffd\\ufffd\\ufffd\\ufffd",
        b"\xc0\x80\xc1\xbf\xc2\x80": b"\\ufffd\\ufffd\\ufffd\\ufffd\xc2\x80",
        b"a\xf0\x9f\x98": b"a\\ufffd\\ufffd\\ufffd",
        b"\t\r\"": b"\\t\\r\\\"",
    }
    for v, want in named.items():
        assert C.go_json_witness(v) == want == C.body(v), v
    key = b'k"\xff<'
    assert C.witness_kv(key, b"\\b") == O.json_kv(key, b"\\b")
    # json_kv's line is head + body + tail, which the record form's reference relies on
    for v in (b"", b"plain", b'"\xff\xe2\x80\xa8'):
        h, head = C.key_line_head(key, 2 ** 64 - 1)
        assert head + C.body(v) + b'"}\n' == O.json_kv(O.format_key(key, 2 ** 64 - 1), v)
        assert h == O.ihash(O.format_key(key, 2 ** 64 - 1))


# ---- the host-compiled escapers against the oracle ------------------------------------------
def _stream(values):
    """[(json_body<true>'s bytes, escape_width_at + escape_put's bytes)] from the stand-alone program"""
    subprocess.run(["make", "-s", "-C", DIR], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1")
    feed = b"".join(struct.pack("<I", len(v)) + v for v in values)
    p = subprocess.run([os.path.join(DIR, "escape_width_test"), "--stream"], input=feed, capture_output=True,
                       timeout=300, env=env)
    assert p.returncode == 0, (p.returncode, p.stderr.decode(errors="replace")[-3000:])
    assert b"AddressSanitizer" not in p.stderr and b"runtime error" not in p.stderr
    assert p.stderr.endswith(b"streamed %d values\n" % len(values)), p.stderr[-200:]
    out, at, raw = [], 0, p.stdout
    for _ in values:
        pair = []
        for _ in (0, 1):
            (n,) = struct.unpack_from("<I", raw, at)
            pair.append(raw[at + 4:at + 4 + n])
            at += 4 + n
        out.append(pair)
    assert at == len(raw)
    return out


def test_host_escapers_against_the_oracle():
    values = C.short_values() + [C.padded(p) for p in range(16)] + C.random_values() + C.lone_values()
    got = _stream(values)
    bad = [(v[:40], len(v)) for v, (seq, local) in zip(values, got) if not seq == local == C.body(v)]
    assert not bad, (len(bad), bad[:3])
