"""Inputs of the reduce-language tests: the spellings a JSON string may give
one raw string, the invalid UTF-8 classes, and line builders. Shared by
tests/test_go_json.py (CPU) and tests/test_gpu_reduce_language.py."""
import go_json as G

FFFD = b"\xef\xbf\xbd"

# invalid raw sequences and the number of U+FFFD utf8.DecodeRune makes of them
# (one per byte): lone continuation bytes, truncated 2/3/4-byte heads, overlong
# C0 AF and E0 80 80, the surrogate ED A0 80, F4 90 80 80 (> U+10FFFF), F5..FF
INVALID = [b"\x80", b"\xbf", b"\xc3", b"\xe2", b"\xe2\x82", b"\xf0", b"\xf0\x9f", b"\xf0\x9f\x98", b"\xc0\xaf",
           b"\xc1\x81", b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xf5", b"\xfe", b"\xff"]

# raw bytes -> the ways a JSON string can spell them (the first is what
# json.Encoder writes)
SPELLINGS = {
    b"a": [b"a", b"\\u0061"],
    b"Z": [b"Z", b"\\u005a", b"\\u005A"],
    b"7": [b"7", b"\\u0037"],
    b" ": [b" ", b"\\u0020"],
    b")": [b")", b"\\u0029"],
    b"<": [b"\\u003c", b"\\u003C", b"<"],
    b">": [b"\\u003e", b"\\u003E", b">"],
    b"&": [b"\\u0026", b"&"],
    b"/": [b"/", b"\\/", b"\\u002f", b"\\u002F"],
    b'"': [b'\\"', b"\\u0022"],
    b"\\": [b"\\\\", b"\\u005c", b"\\u005C"],
    b"\x08": [b"\\u0008", b"\\b"],
    b"\x0c": [b"\\u000c", b"\\f", b"\\u000C"],
    b"\n": [b"\\n", b"\\u000a", b"\\u000A"],
    b"\r": [b"\\r", b"\\u000d"],
    b"\t": [b"\\t", b"\\u0009"],
    b"\x01": [b"\\u0001"],
    b"\x7f": [b"\x7f", b"\\u007f", b"\\u007F"],
    "é".encode(): ["é".encode(), b"\\u00e9", b"\\u00E9"],
    "€".encode(): ["€".encode(), b"\\u20ac", b"\\u20AC"],
    "\u2028".encode(): [b"\\u2028", "\u2028".encode()],
    "\U0001F600".encode(): ["\U0001F600".encode(), b"\\ud83d\\ude00", b"\\uD83D\\uDE00", b"\\ud83D\\uDe00"],
    # lone surrogate escapes and single invalid bytes all decode to U+FFFD
    FFFD: [FFFD, b"\\ufffd", b"\\uFFFD", b"\\ud800", b"\\udbff", b"\\udc00", b"\\udfff", b"\x80", b"\xbf", b"\xc0",
           b"\xc3", b"\xe2", b"\xf0", b"\xf5", b"\xfe", b"\xff"],
    FFFD * 2: [FFFD * 2, b"\\ufffd\\uFFFD", b"\xc0\xaf", b"\xe2\x82", b"\xf0\x9f", b"\\ud800\\udbff"],
    FFFD * 3: [FFFD * 3, b"\\ufffd\\ufffd\\ufffd", b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xf0\x9f\x98"],
    FFFD * 4: [FFFD * 4, b"\xf4\x90\x80\x80"],
}
ATOMS = list(SPELLINGS)


def kv_line(key_spelled: bytes, value_spelled: bytes) -> bytes:
    return b'{"Key":"' + key_spelled + b'","Value":"' + value_spelled + b'"}\n'


def canonical(atoms) -> bytes:
    return b"".join(SPELLINGS[a][0] for a in atoms)


def respell(atoms, rnd, tries=8) -> bytes:
    """A random spelling of the atoms' raw bytes. Neighbouring spellings can
    combine (a lone \\ud800 before \\udc00 pairs up, E2 before 80 80 is a valid
    rune), so the result is checked against the reference's unquote and drawn
    again; the canonical spelling is the fallback."""
    raw = b"".join(atoms)
    for _ in range(tries):
        s = b"".join(rnd.choice(SPELLINGS[a]) for a in atoms)
        if G.unquote(s + b'"') == (raw, len(s) + 1):
            return s
    return canonical(atoms)


def random_atoms(rnd, raw_len_lo, raw_len_hi, plain_bias=0.7):
    """Atoms whose raw bytes total between the two lengths (inclusive)."""
    target = rnd.randint(raw_len_lo, raw_len_hi)
    atoms, n = [], 0
    while n < target:
        a = rnd.choice((b"a", b"Z", b"7", b" ")) if rnd.random() < plain_bias else rnd.choice(ATOMS)
        if n + len(a) > target:
            a = b"a"
        atoms.append(a)
        n += len(a)
    return atoms
