"""What Go's encoding/json decoder (Go 1.18) makes of the reduce task's input,
restated in plain Python — test infrastructure only.

map_reduce/worker.go:44-68 (readReduceInput) decodes every line of an
mr-<map>-<r> file into a KeyValue with json.NewDecoder; dgrep_reduce accepts
the compact two-field form

    {"Key":"<json string>","Value":"<json string>"}\\n

with ANY JSON string the decoder accepts, and must give exactly the decoder's
strings for it. Restated here, in the decoder's own two passes:

  scan_string  the scanner (scanner.go stateInString*): finds the closing
               quote and rejects raw bytes < 0x20, unknown escapes, bad hex;
  unquote      decode.go unquoteBytes over the literal the scanner accepted:
               escapes, surrogate pairs, and utf8.DecodeRune coercion of raw
               bytes >= 0x80 (each byte of an invalid sequence -> U+FFFD).
"""
import re
from collections import namedtuple

RUNE_ERROR = 0xFFFD

# utf8.go: acceptRanges of the second byte, by first byte
_LOCB, _HICB = 0x80, 0xBF


def decode_rune(b: bytes, i: int = 0, end: int = None):
    """utf8.DecodeRune(b[i:end]) -> (rune, size); (U+FFFD, 1) for any invalid
    or truncated sequence (and (U+FFFD, 0) for an empty slice, as Go)."""
    if end is None:
        end = len(b)
    n = end - i
    if n < 1:
        return RUNE_ERROR, 0
    b0 = b[i]
    if b0 < 0x80:
        return b0, 1
    lo, hi = _LOCB, _HICB
    if 0xC2 <= b0 <= 0xDF:
        size = 2
    elif 0xE0 <= b0 <= 0xEF:
        size = 3
        if b0 == 0xE0:
            lo = 0xA0
        elif b0 == 0xED:
            hi = 0x9F
    elif 0xF0 <= b0 <= 0xF4:
        size = 4
        if b0 == 0xF0:
            lo = 0x90
        elif b0 == 0xF4:
            hi = 0x8F
    else:  # 80..BF, C0, C1, F5..FF
        return RUNE_ERROR, 1
    if n < size:
        return RUNE_ERROR, 1
    b1 = b[i + 1]
    if b1 < lo or b1 > hi:
        return RUNE_ERROR, 1
    if size == 2:
        return (b0 & 0x1F) << 6 | (b1 & 0x3F), 2
    b2 = b[i + 2]
    if b2 < _LOCB or b2 > _HICB:
        return RUNE_ERROR, 1
    if size == 3:
        return (b0 & 0x0F) << 12 | (b1 & 0x3F) << 6 | (b2 & 0x3F), 3
    b3 = b[i + 3]
    if b3 < _LOCB or b3 > _HICB:
        return RUNE_ERROR, 1
    return (b0 & 0x07) << 18 | (b1 & 0x3F) << 12 | (b2 & 0x3F) << 6 | (b3 & 0x3F), 4


def encode_rune(r: int) -> bytes:
    """utf8.EncodeRune (surrogates and out-of-range runes -> U+FFFD)."""
    if r < 0 or r > 0x10FFFF or 0xD800 <= r < 0xE000:
        r = RUNE_ERROR
    return chr(r).encode("utf-8")


def coerce_utf8(b: bytes) -> bytes:
    """string -> []rune -> string: every byte of an invalid sequence -> U+FFFD."""
    out, i = bytearray(), 0
    while i < len(b):
        r, size = decode_rune(b, i)
        out += encode_rune(r)
        i += size
    return bytes(out)


_HEX = b"0123456789abcdefABCDEF"
# a run of bytes that both passes take as they are: ASCII from 0x20 on but '"' and '\\'
_PLAIN_RUN = re.compile(rb"[\x20\x21\x23-\x5b\x5d-\x7f]+")
_SHORT = {ord('"'): 0x22, ord("\\"): 0x5C, ord("/"): 0x2F, ord("b"): 8, ord("f"): 12, ord("n"): 10, ord("r"): 13,
          ord("t"): 9}


def scan_string(s: bytes, i: int = 0):
    """The scanner over a string literal whose opening quote precedes s[i]:
    the index of its closing quote, or None (raw byte < 0x20, an escape other
    than \\" \\\\ \\/ \\b \\f \\n \\r \\t \\uXXXX, a non-hex digit, no closing quote)."""
    n = len(s)
    while i < n:
        m = _PLAIN_RUN.match(s, i)
        if m:
            i = m.end()
            continue
        c = s[i]
        if c == 0x22:
            return i
        if c < 0x20:
            return None
        if c != 0x5C:
            i += 1
            continue
        if i + 1 >= n:
            return None
        e = s[i + 1]
        if e == ord("u"):
            if i + 6 > n or any(h not in _HEX for h in s[i + 2:i + 6]):
                return None
            i += 6
        elif e in _SHORT:
            i += 2
        else:
            return None
    return None


def _getu4(s: bytes, r: int) -> int:
    if r + 6 > len(s) or s[r] != 0x5C or s[r + 1] != ord("u"):
        return -1
    h = s[r + 2:r + 6]
    return int(h, 16) if all(c in _HEX for c in h) else -1


def _unquote_literal(s: bytes) -> bytes:
    """unquoteBytes over the inside of a literal scan_string accepted."""
    out, r = bytearray(), 0
    while r < len(s):
        m = _PLAIN_RUN.match(s, r)
        if m:
            out += m.group()
            r = m.end()
            continue
        c = s[r]
        if c == 0x5C:
            e = s[r + 1]
            if e != ord("u"):
                out.append(_SHORT[e])
                r += 2
                continue
            rr = _getu4(s, r)
            r += 6
            if 0xD800 <= rr < 0xE000:
                rr1 = _getu4(s, r)
                if rr < 0xDC00 and 0xDC00 <= rr1 < 0xE000:  # utf16.DecodeRune: a valid pair, consumed
                    out += encode_rune(0x10000 + ((rr - 0xD800) << 10) + (rr1 - 0xDC00))
                    r += 6
                    continue
                rr = RUNE_ERROR  # the following escape is NOT consumed
            out += encode_rune(rr)
        elif c < 0x80:
            out.append(c)
            r += 1
        else:
            rr, size = decode_rune(s, r)
            out += encode_rune(rr)
            r += size
    return bytes(out)


def unquote(body: bytes):
    """body = the bytes after a string's opening quote (its closing quote and
    whatever follows included): (decoded bytes, index after the closing quote),
    or None if the decoder rejects the string."""
    q = scan_string(body, 0)
    if q is None:
        return None
    return _unquote_literal(body[:q]), q + 1


_KEY_OPEN = b'{"Key":"'
_VAL_OPEN = b',"Value":"'


def parse_kv_line(line: bytes):
    """line = one input line without its '\\n': (key, value), or None for
    anything but {"Key":"<string>","Value":"<string>"} byte for byte (no
    whitespace, no other field order or names, nothing after the brace)."""
    if not line.startswith(_KEY_OPEN):
        return None
    k = unquote(line[len(_KEY_OPEN):])
    if k is None:
        return None
    key, i = k
    i += len(_KEY_OPEN)
    if not line.startswith(_VAL_OPEN, i):
        return None
    i += len(_VAL_OPEN)
    v = unquote(line[i:])
    if v is None:
        return None
    value, j = v
    if line[i + j:] != b"}":
        return None
    return key, value


ReduceRef = namedtuple("ReduceRef", "output bad_line kv")


def reduce_reference(data: bytes) -> ReduceRef:
    """dgrep_reduce's contract: in input order, key + b" " + value + b"\\n" for
    each line whose decoded key is seen for the first time. output is None and
    bad_line the 1-based number of the first line outside the accepted form if
    there is one (a last line without '\\n' counts); kv = {key: set(values)}."""
    out, kv = bytearray(), {}
    lines = data.split(b"\n")
    tail = lines.pop()
    for no, line in enumerate(lines, 1):
        p = parse_kv_line(line)
        if p is None:
            return ReduceRef(None, no, kv)
        key, value = p
        if key not in kv:
            out += key + b" " + value + b"\n"
            kv[key] = set()
        kv[key].add(value)
    if tail:
        return ReduceRef(None, len(lines) + 1, kv)
    return ReduceRef(bytes(out), None, kv)
