"""dgrep_reduce over everything it accepts, byte for byte against
tests/go_json.py (Go's json decoder restated): the compact two-field line with
ANY JSON string the decoder takes -- respelled keys on both sides of the old
64-byte compare switch, raw invalid UTF-8, the lines whose lengths look plain
and are not -- and DGREP_E_INVALID naming the line for everything else. The
first line of each distinct key is kept, in input order, so the expected output
is one byte string (values may hold '\\n' or ') ')."""
import os
import random
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import go_json as G  # noqa: E402
import reduce_cases as C  # noqa: E402
from reduce_cases import FFFD, kv_line  # noqa: E402

pytestmark = pytest.mark.gpu

K_SEG = 256 << 10  # reduce.hip kSeg: bytes per newline-pass block


def check(ctx, data: bytes, nkeys=None) -> bytes:
    """ctx.reduce(data) == the reference, byte for byte (nkeys: the number of
    distinct keys the test's own construction intends)."""
    ref = G.reduce_reference(data)
    assert ref.bad_line is None, ref.bad_line
    if nkeys is not None:
        assert len(ref.kv) == nkeys, (len(ref.kv), nkeys)
    got = ctx.reduce(data)
    if got != ref.output:
        n = min(len(got), len(ref.output))
        d = next((i for i in range(n) if got[i] != ref.output[i]), n)
        raise AssertionError("output differs at byte %d of %d (got %d bytes, %d lines; want %d lines): got %r want %r" % (
            d, len(ref.output), len(got), got.count(b"\n"), ref.output.count(b"\n"), got[max(0, d - 40):d + 40],
            ref.output[max(0, d - 40):d + 40]))
    return got


# ---- spellings across the 64-byte switch --------------------------------
E_ACUTE, GRIN = "é".encode(), "\U0001F600".encode()


def _spellings(tag: bytes, raw_len: int):
    """(raw key, [spelled keys]) of raw_len raw bytes: '<', é, an astral rune,
    '/', ASCII filler and a tag, the respelled ASCII byte being the LAST one so
    that the escaped forms first differ at every depth."""
    fill = b"k" * (raw_len - 8 - len(tag) - 1)
    assert len(fill) >= 1
    raw = b"<" + E_ACUTE + GRIN + b"/" + fill + tag + b"q"
    assert len(raw) == raw_len
    lt, ea, gr, sl, last = b"\\u003c", E_ACUTE, GRIN, b"/", b"q"
    mk = lambda lt=lt, ea=ea, gr=gr, sl=sl, last=last: lt + ea + gr + sl + fill + tag + last  # noqa: E731
    return raw, [mk(), mk(last=b"\\u0071"), mk(lt=b"\\u003C"), mk(ea=b"\\u00e9"), mk(gr=b"\\ud83d\\ude00"),
                 mk(sl=b"\\/"), mk(lt=b"<", ea=b"\\u00E9", gr=b"\\uD83D\\uDE00", sl=b"\\u002F", last=b"\\u0071")]


@pytest.mark.parametrize("raw_len", [63, 64, 65, 66, 200])
def test_spellings_merge_across_64_bytes(gpu_ctx, raw_len):
    keys = [_spellings(b"#%d" % i, raw_len) for i in range(5)]
    nsp = len(keys[0][1])
    lines, first = [], {}
    for s in range(nsp):
        for i, (raw, sp) in enumerate(keys):
            which = (s + i) % nsp  # every key starts with another spelling
            value = b"v%d-%d" % (i, which)
            first.setdefault(raw, value)
            lines.append(kv_line(sp[which], value))
        lines.append(kv_line(b"other-%d" % s, b"o"))
    data = b"".join(lines)
    got = check(gpu_ctx, data, nkeys=len(keys) + nsp)
    for raw, value in first.items():
        assert got.count(raw + b" ") == 1 and raw + b" " + value + b"\n" in got


def test_long_keys_that_stay_apart(gpu_ctx):
    """These keys differ and so do their hashes: they never meet in an
    equal-hash run, and the compare's "different" verdict is not asked for.
    Keys that differ and share their hash are in test_gpu_reduce_collisions.py."""
    x70 = b"x" * 70
    pairs = [
        (b"k" * 64 + b"a", b"k" * 64 + b"b"),  # the last raw byte
        (b"k" * 199 + b"a", b"k" * 199 + b"b"),
        (x70 + b"\\u003c", x70 + b"\\u003e"),  # inside an escape
        (b"\\u003c" + x70, b"\\u003e" + x70),
        (b"\\u0041" + x70, b"\\u0042" + x70),  # equal escaped length, other raw content
        (b"\\n" + x70, b"ab" + x70),  # equal escaped length, raw 71 and 72
        (b"\\u00e9" + x70, b"abcdef" + x70),
        (b"p" * 65, b"p" * 66),  # one a prefix of the other
        (b"p" * 66 + b"\\u0070", b"p" * 66 + b"\\u0070\\u0070"),  # = p*67 and p*68, respelled
        (E_ACUTE * 40, E_ACUTE * 39 + b"\\u00e8"),
        (b"z" * 64 + b"\\ufffd", b"z" * 64 + b"\\ufffe"),
    ]
    lines = []
    for rep in range(2):
        for n, (a, b) in enumerate(pairs):
            lines.append(kv_line(a, b"a%d-%d" % (n, rep)))
            lines.append(kv_line(b, b"b%d-%d" % (n, rep)))
    check(gpu_ctx, b"".join(lines), nkeys=2 * len(pairs))


# ---- raw invalid UTF-8 ---------------------------------------------------
def test_raw_invalid_utf8_in_key_and_value(gpu_ctx):
    lines = []
    for n, seq in enumerate(C.INVALID):
        lines.append(kv_line(b"k%d" % n + seq + b"z", b"v" + seq + b"w"))
        # as the last thing before the closing quote, in the key, the value, both
        lines.append(kv_line(b"e%d" % n + seq, b"plain"))
        lines.append(kv_line(b"f%d" % n, seq))
        lines.append(kv_line(seq, seq))
        # beyond 64 raw bytes, and a valid rune right after the bad bytes
        lines.append(kv_line(b"L%d" % n + b"y" * 70 + seq, seq + "€".encode() + seq))
    data = b"".join(lines)
    assert b'\xe2","Value"' in data and b'\xe2"}\n' in data
    # the bare sequences of equal length decode to the same run of U+FFFD
    nbare = len({len(seq) for seq in C.INVALID})
    check(gpu_ctx, data, nkeys=4 * len(C.INVALID) + nbare)


@pytest.mark.parametrize("tail_len", [5, 61, 62, 100])
def test_raw_invalid_utf8_keys_merge(gpu_ctx, tail_len):
    """a\\xff.., a\\xfe.., escaped a\\ufffd.. and raw a\\xef\\xbf\\xbd.. are one key
    (raw length 9, 65, 66, 104)."""
    tail = b"t" * tail_len
    heads = [b"a\xff", b"a\xfe", b"a\\ufffd", b"a" + FFFD, b"a\\uFFFD", b"a\x80", b"a\xc0", b"a\\udc00"]
    for rot in range(len(heads)):
        order = heads[rot:] + heads[:rot]
        lines = [kv_line(b"before", b"0")]
        for n, h in enumerate(order):
            lines.append(kv_line(h + tail, b"v%d" % n))
            lines.append(kv_line(b"between%d" % n, h))
        got = check(gpu_ctx, b"".join(lines), nkeys=2 + len(heads))
        assert b"a" + FFFD + tail + b" v0\n" in got


# ---- lines whose lengths look plain -------------------------------------
# Encoded minus raw length of one unit: short escape +1; \u00XX of an ASCII byte
# +5, of a 2-byte rune +4, of a 3-byte rune or a lone surrogate +3; an escaped
# pair +8; a coerced invalid byte 1 - 3 = -2. A line is a copy of its two byte
# ranges only if it has none of them, but encoded == 21 + klen + vlen whenever
# the surpluses cancel: 2 x (+1) with one bad byte, +4 with two, +5 +1 with
# three, ...
SURPLUS = [(b"\\n", 1), (b"\\/", 1), (b'\\"', 1), (b"\\u0041", 5), (b"\\u00e9", 4), (b"\\u20ac", 3), (b"\\ud800", 3),
           (b"\\ud83d\\ude00", 8)]
BAD_BYTES = [b"\xff", b"\x80", b"\xc3", b"\xe2", b"\xf0"]


def _coincidences():
    combos = []

    def grow(start, chosen, total):
        if total and total % 2 == 0:
            combos.append((list(chosen), total // 2))
        if len(chosen) == 4:
            return
        for i in range(start, len(SURPLUS)):
            if total + SURPLUS[i][1] <= 10:
                grow(i, chosen + [SURPLUS[i][0]], total + SURPLUS[i][1])

    grow(0, [], 0)
    return combos


def test_length_coincidence_is_not_plain(gpu_ctx):
    combos = _coincidences()
    assert ([b"\\n", b"\\n"], 1) in combos and ([b"\\u00e9"], 2) in combos and ([b"\\n", b"\\u0041"], 3) in combos
    lines = []
    for n, (escapes, nbad) in enumerate(combos):
        esc = b"-".join(escapes)
        bad = b"-".join(BAD_BYTES[(n + k) % len(BAD_BYTES)] for k in range(nbad))
        pad = b"p" * (n % 5)  # every dword phase of source and output
        for m, (k, v) in enumerate([(esc + b"+" + bad, b"plain"), (b"plain", bad + b"+" + esc), (esc, bad), (bad, esc),
                                    (b"y" * 66 + esc, bad + b"y" * 300)]):
            key, value = b"%d.%d" % (n, m) + pad + k, pad + v
            line = kv_line(key, value)
            kr, vr = G.unquote(key + b'"')[0], G.unquote(value + b'"')[0]
            assert len(line) - 1 == 21 + len(kr) + len(vr), line  # the coincidence itself
            lines.append(line)
            lines.append(kv_line(b"plain%d.%d" % (n, m), b"between" + pad))
    check(gpu_ctx, b"".join(lines), nkeys=len(lines))


# ---- random differential ----------------------------------------------------
def test_random_differential(gpu_ctx):
    rnd = random.Random(20240607)
    lens = [0, 1, 2, 62, 63, 64, 65, 66, 67, 130, 250, 400]
    keys = [C.random_atoms(rnd, n, n) for n in lens]
    keys += [C.random_atoms(rnd, 40, 90, plain_bias=rnd.choice((0.3, 0.7, 0.95))) for _ in range(150 - len(keys))]
    lines = []
    for _ in range(2000):
        katoms = rnd.choice(keys)
        kind = rnd.random()
        key = C.canonical(katoms) if kind < 0.3 else C.respell(katoms, rnd)
        vatoms = C.random_atoms(rnd, 0, rnd.choice((0, 8, 60, 300)), plain_bias=rnd.choice((0.5, 0.9, 1.0)))
        value = b"".join(rnd.choice(C.SPELLINGS[a]) for a in vatoms)
        lines.append(kv_line(key, value))
    data = b"".join(lines)
    ref = G.reduce_reference(data)
    assert 100 <= len(ref.kv) <= 150  # (a key the draw never picked, or two draws of one key)
    assert sum(len(v) > 1 for v in ref.kv.values()) > 90
    check(gpu_ctx, data)


# ---- rejects ---------------------------------------------------------------
GOOD = [kv_line(b"good-%d" % i, b"value %d" % i) for i in range(1000)]
VALID_LINES = [
    kv_line(b'a\\"b', b"c\\\\d"), kv_line(b"\\/x", b"\\b\\f"), kv_line(b"\\n\\r", b"\\t"), kv_line(b"\\u0041", b"\\u00e9"),
    kv_line(b"\\u003C", b"\\uABcd"), kv_line(b"\\ud83d\\ude00", b"\\uD83D\\uDE00"), kv_line(b"\\ud800", b"\\udc00x"),
    kv_line(E_ACUTE + GRIN, b"\xff\xe2"), kv_line(b"", b""), kv_line(b"log.txt (line number #7)", b"an error <here>"),
]


def _line_named(err) -> int:
    m = re.search(r"line (\d+)", str(err.value))
    assert m, str(err.value)
    return int(m.group(1))


def test_rejects_every_proper_prefix(gpu_ctx):
    import dgrep

    check(gpu_ctx, b"".join(VALID_LINES))  # the lines themselves are accepted
    before, after = b"".join(GOOD[:3]), b"".join(GOOD[3:5])
    for line in VALID_LINES:
        for cut in range(len(line) - 1):  # proper prefixes of the line without its '\n'
            data = before + line[:cut] + b"\n" + after
            assert G.reduce_reference(data).bad_line == 4, (line, cut)
            with pytest.raises(dgrep.DgrepError) as err:
                gpu_ctx.reduce(data)
            assert _line_named(err) == 4, (line, cut)


@pytest.mark.parametrize("bad", [b"not json\n", b'{"Key":"' + b"k" * 100 + b'","Value":"\\q"}\n'],
                         ids=["not-json", "long-key-bad-value"])
def test_rejects_name_the_first_bad_line(gpu_ctx, bad):
    import dgrep

    for where in (1, 64, 65, 256, 257, 1000):
        lines = list(GOOD)
        lines[where - 1] = bad
        with pytest.raises(dgrep.DgrepError) as err:
            gpu_ctx.reduce(b"".join(lines))
        assert _line_named(err) == where
    for lo, hi in ((3, 4), (64, 65), (1, 1000), (257, 700)):
        lines = list(GOOD)
        lines[lo - 1] = bad
        lines[hi - 1] = b'{"Key":"' + b"k" * 100 + b'","Value":"\x01"}\n'
        data = b"".join(lines)
        assert G.reduce_reference(data).bad_line == lo
        with pytest.raises(dgrep.DgrepError) as err:
            gpu_ctx.reduce(data)
        assert _line_named(err) == lo
    check(gpu_ctx, b"".join(GOOD), nkeys=1000)  # and the context still reduces


def test_rejects_shapes_go_would_take(gpu_ctx):
    import dgrep

    ok = b'{"Key":"a","Value":"b"}\n'
    for bad in (b'{"Key": "a","Value":"b"}\n', b'{"Key":"a","Value": "b"}\n', b'{"Key":"a", "Value":"b"}\n',
                b'{"Key":"a","Value":"b"}\r\n', b"\n", b'{"key":"a","Value":"b"}\n', b'{"Key":"a","value":"b"}\n',
                b'{"Key":"a","Value":"b","Third":"c"}\n', b'{"Value":"b","Key":"a"}\n', b'{"Key":"a","Value":"b"} \n',
                b' {"Key":"a","Value":"b"}\n', b'{"Key":"a","Value":"b"}{"Key":"c","Value":"d"}\n',
                b'{"Key":"a"}\n', b'{"Key":"a","Value":7}\n', b'{"Key":"a","Value":"b\\\'"}\n'):
        data = ok + ok + bad + ok
        assert G.reduce_reference(data).bad_line == 3, bad
        with pytest.raises(dgrep.DgrepError) as err:
            gpu_ctx.reduce(data)
        assert _line_named(err) == 3, bad
    with pytest.raises(dgrep.DgrepError):
        gpu_ctx.reduce(ok + ok[:-1])  # no '\n' at the end
    assert gpu_ctx.reduce(ok + ok) == b"a b\n"


# ---- newline geometry -------------------------------------------------------
def test_every_input_length_mod_16(gpu_ctx):
    for pad in range(16):
        lines = [kv_line(b"k%d" % i, b"v" * i) for i in range(5)] + [kv_line(b"pad", b"." * pad)]
        lines += [kv_line(b"k1", b"dup"), kv_line(b"tail\\n", b"\\u00e9")]
        data = b"".join(lines)
        check(gpu_ctx, data, nkeys=7)
        check(gpu_ctx, b"".join(lines[:6]), nkeys=6)  # the padded line last
    assert len({(len(b"".join(lines[:5])) + p) % 16 for p in range(16)}) == 16


@pytest.mark.parametrize("at", [K_SEG - 1, K_SEG, K_SEG + 1, 2 * K_SEG - 1, 2 * K_SEG])
def test_newline_at_segment_edges(gpu_ctx, at):
    """A '\\n' exactly at byte `at`; long plain values keep the line count low."""
    out, n, i = [], 0, 0
    fill = b"f" * 3000
    while True:
        line = kv_line(b"key %d" % i, fill[:2000 + i % 1000])
        if n + len(line) + 40 > at:
            break
        out.append(line)
        n += len(line)
        i += 1
    frame = len(kv_line(b"edge", b""))
    out.append(kv_line(b"edge", b"e" * (at + 1 - n - frame)))
    data = b"".join(out)
    assert len(data) == at + 1 and data[at] == 10
    data += b"".join(kv_line(b"after %d" % j, b"a" * j) for j in range(40)) + kv_line(b"edge", b"dup")
    check(gpu_ctx, data, nkeys=len(out) + 40)
    check(gpu_ctx, data[:at + 1], nkeys=len(out))  # the edge newline is the input's last byte


def test_value_longer_than_a_segment(gpu_ctx):
    big = b"v" * (K_SEG + 4097)
    data = kv_line(b"a", b"1") + kv_line(b"big", big) + kv_line(b"b\\u0062", big[:K_SEG * 2 // 3] + b"\\n\\u00e9") + \
        kv_line(b"big", b"again") + kv_line(b"c", big + big)
    check(gpu_ctx, data, nkeys=4)


def test_smallest_line_alone_and_repeated(gpu_ctx):
    one = kv_line(b"", b"")
    assert len(one) == 22
    assert check(gpu_ctx, one, nkeys=1) == b" \n"
    assert check(gpu_ctx, one * 70000, nkeys=1) == b" \n"
    assert check(gpu_ctx, kv_line(b"", b"x") + one * 300 + kv_line(b"\\u0041", b"") + one, nkeys=2) == b" x\nA \n"


# ---- writer phases ---------------------------------------------------------
@pytest.mark.parametrize("phase", [0, 1, 2, 3])
def test_writer_dword_phases(gpu_ctx, phase):
    """Plain lines whose values straddle the wave's 256-byte sweeps (64 lanes x
    one dword), after a line that shifts source and output by `phase` bytes;
    the key length moves the value's own phase against the line's."""
    lines = [kv_line(b"p", b"x" * phase)]
    for n, vlen in enumerate(list(range(250, 263)) + list(range(506, 519))):
        body = bytes(33 + (7 * n + k) % 90 for k in range(vlen)).replace(b'"', b"q").replace(b"\\", b"b")
        lines.append(kv_line(b"key" + b"k" * (n % 4) + b"%d" % n, body))
        if n % 5 == 0:
            lines.append(kv_line(b"esc\\n%d" % n, body[:251 + n] + b"\\t"))
    assert len(lines[0]) % 4 == (22 + 1 + phase) % 4
    check(gpu_ctx, b"".join(lines), nkeys=len(lines))
