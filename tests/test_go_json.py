"""tests/go_json.py (Go's json decoder over the reduce input, restated) against
independent witnesses: the oracle's C restatement of the ENCODER's
utf8.DecodeRune coercion, and Python's json module for escapes."""
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import go_json as G  # noqa: E402
import oracle_lib as O  # noqa: E402
import reduce_cases as C  # noqa: E402

VALID_RUNES = [b"a", b" ", b"<", b"\\", b'"', "é".encode(), "\u07ff".encode(), "\u0800".encode(), "€".encode(),
               "\ud7ff".encode(), "\ue000".encode(), "\ufffd".encode(), "\U00010000".encode(), "\U0001F600".encode(),
               "\U0010FFFF".encode()]


def test_decode_rune_known_answers():
    assert G.decode_rune(b"a") == (0x61, 1)
    assert G.decode_rune("é".encode()) == (0xE9, 2)
    assert G.decode_rune("€x".encode()) == (0x20AC, 3)
    assert G.decode_rune(b"zz\xf0\x9f\x98\x80", 2) == (0x1F600, 4)
    assert G.decode_rune(b"\xf4\x8f\xbf\xbf") == (0x10FFFF, 4)
    assert G.decode_rune(b"\xed\x9f\xbf") == (0xD7FF, 3)
    assert G.decode_rune(b"") == (0xFFFD, 0)
    for bad in C.INVALID + [b"\xc2", b"\xc2\x22", b"\xe2\x82\x22", b"\xf0\x8f\x80\x80", b"\xf4\x8f\xbf", b"\xe0\x9f\xbf"]:
        assert G.decode_rune(bad) == (0xFFFD, 1), bad
    # a bound inside the buffer truncates like the end of the slice
    assert G.decode_rune("€".encode(), 0, 2) == (0xFFFD, 1)


def test_coercion_vs_oracle_encoder():
    """coerce_utf8 (decode_rune + re-encode) == what survives json.Encoder as the
    oracle restates it (one \\ufffd per bad byte) and Python's json.loads."""
    rnd = random.Random(11)
    for _ in range(3000):
        k = b"".join(rnd.choice(C.INVALID) if rnd.random() < 0.5 else rnd.choice(VALID_RUNES)
                     for _ in range(rnd.randrange(0, 9)))
        want = json.loads(O.json_kv(k, k))["Key"].encode("utf-8")
        assert G.coerce_utf8(k) == want, k


ESCAPES = [b'\\"', b"\\\\", b"\\/", b"\\b", b"\\f", b"\\n", b"\\r", b"\\t", b"\\u0041", b"\\u00e9", b"\\u00E9",
           b"\\u003c", b"\\u003C", b"\\u20ac", b"\\u20AC", b"\\uffFD", b"\\u0000", b"\\u001f", b"\\uABCD", b"\\uabcd"]
SURROGATES = [b"\\ud83d\\ude00", b"\\uD83D\\uDE00", b"\\udbff\\udfff", b"\\ud800\\udc00",  # pairs
              b"\\ud800", b"\\udbff", b"\\uD83D",  # lone high
              b"\\udc00", b"\\udfff", b"\\uDE00",  # lone low
              b"\\ud800\\u0041", b"\\ud83d\\n", b"\\ud800\\ud800\\udc00", b"\\ud83dx", b"\\udc00\\ud800"]
RAW = [b"a", b"/", b" ", b"<", b"'", b"\x7f", "é".encode(), "€".encode(), "\U0001F600".encode(), "\u2028".encode()]


def _py_unquote(body: bytes) -> bytes:
    s = json.loads(b'"' + body + b'"')
    return "".join("\ufffd" if 0xD800 <= ord(ch) < 0xE000 else ch for ch in s).encode("utf-8")


def test_unquote_vs_python_json():
    """Valid-UTF-8 bodies of every escape kind, both hex cases and every
    surrogate arrangement (pair, lone high, lone low, high before a non-low
    escape, high as the last thing before the quote): Python's json.loads
    agrees once its lone surrogates are mapped to U+FFFD."""
    rnd = random.Random(12)
    bodies = [b"", b"\\ud800", b"x\\ud83d", b"\\ud83d\\ude00", b"\\ud800\\u0041"] + ESCAPES + SURROGATES
    for _ in range(1500):
        parts = [rnd.choice(rnd.choice((ESCAPES, SURROGATES, RAW))) for _ in range(rnd.randrange(0, 12))]
        if rnd.random() < 0.3:
            parts.append(rnd.choice((b"\\ud800", b"\\udbff", b"\\uD83D")))  # a high surrogate right before the quote
        bodies.append(b"".join(parts))
    for body in bodies:
        tail = rnd.choice((b"", b",x", b'"'))
        assert G.unquote(body + b'"' + tail) == (_py_unquote(body), len(body) + 1), body


def test_unquote_rejects():
    for bad in (b'\\x41"', b"\\'\"", b'\\u12G4"', b'\\u12', b'\\u12"', b'\\u', b"\\", b'a\x1fb"', b'a\nb"', b'a\x00"',
                b"no closing quote", b"", b'\\ud800\\u12"', b'ends in a backslash\\"'):
        assert G.unquote(bad) is None, bad
    assert G.unquote(b'"') == (b"", 1)
    assert G.unquote(b'a\\u0041\\/"rest') == (b"aA/", 10)


def test_unquote_raw_invalid_utf8():
    for seq in C.INVALID:
        assert G.unquote(b"a" + seq + b'z"') == (b"a" + C.FFFD * len(seq) + b"z", len(seq) + 3), seq
        # as the last thing before the closing quote: the quote is not swallowed
        assert G.unquote(seq + b'","Value"') == (C.FFFD * len(seq), len(seq) + 1), seq
    assert G.unquote(b'\xe2\x82\xac"') == ("€".encode(), 4)


def test_spelling_table_is_consistent():
    """Every spelling in reduce_cases.SPELLINGS decodes to its raw bytes."""
    for raw, spellings in C.SPELLINGS.items():
        for s in spellings:
            assert G.unquote(s + b'"') == (raw, len(s) + 1), (raw, s)
    # and the canonical (first) spelling is what json.Encoder writes
    for raw, spellings in C.SPELLINGS.items():
        line = O.json_kv(raw, b"")
        assert line == C.kv_line(spellings[0], b""), raw


def test_parse_kv_line():
    assert G.parse_kv_line(b'{"Key":"a","Value":"b"}') == (b"a", b"b")
    assert G.parse_kv_line(b'{"Key":"","Value":""}') == (b"", b"")
    assert G.parse_kv_line(b'{"Key":"\\u003c\\"","Value":"\xff\\/"}') == (b'<"', C.FFFD + b"/")
    for bad in (b"", b"{}", b'{"Key":"a","Value":"b"}\r', b'{"Key": "a","Value":"b"}', b'{"Key":"a", "Value":"b"}',
                b'{"key":"a","Value":"b"}', b'{"Value":"b","Key":"a"}', b'{"Key":"a","Value":"b","X":"c"}',
                b'{"Key":"a","Value":"b"} ', b' {"Key":"a","Value":"b"}', b'{"Key":"a","Value":"b"', b'{"Key":"a"}',
                b'{"Key":"a","Value":1}', b'{"Key":"a\\q","Value":"b"}', b'{"Key":"a","Value":"b\x01"}',
                b'{"Key":"a","Value":"b"}{"Key":"a","Value":"b"}'):
        assert G.parse_kv_line(bad) is None, bad


def test_reduce_reference():
    data = (b'{"Key":"k","Value":"first"}\n{"Key":"j","Value":"x y"}\n{"Key":"\\u006b","Value":"second"}\n'
            b'{"Key":"j","Value":"x y"}\n')
    ref = G.reduce_reference(data)
    assert ref.output == b"k first\nj x y\n" and ref.bad_line is None
    assert ref.kv == {b"k": {b"first", b"second"}, b"j": {b"x y"}}
    assert G.reduce_reference(b"") == G.ReduceRef(b"", None, {})
    assert G.reduce_reference(data + b"\n").bad_line == 5
    assert G.reduce_reference(data + b'{"Key":"a","Value":"b"}').bad_line == 5
    assert G.reduce_reference(b"x\n" + data + b"y\n")[:2] == (None, 1)
