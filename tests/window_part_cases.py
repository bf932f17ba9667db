"""Data and a pure-Python model for the windowed partition writer
(dgrep_stream_*_partitions / dgrep_map_partitions_windowed): no GPU, no library
but the oracle.

windowed_partitions() restates the contract of include/dgrep.h over
window_cases.windowed(): every window of a call that completed at least one
matching line is one ROW of nreduce cells; cell p holds, in line order, the
json.Encoder lines of the window's records whose key hashes to p. The keys carry
the stream's own line numbers. escape_width() restates the local width rule of
csrc/kernels/escape_width.h.
"""
import oracle_lib as O
import window_cases as WC


def encode_cells(records, filename, nreduce):
    """one row: records (line_no, value bytes) -> nreduce cells"""
    cells = [bytearray() for _ in range(nreduce)]
    for line_no, value in records:
        key = O.format_key(filename, line_no)
        cells[O.ihash(key) % nreduce] += O.json_kv(key, value)
    return [bytes(c) for c in cells]


def whole_partitions(data, match, filename, nreduce):
    """dgrep_map_partitions of the whole split: nreduce byte strings"""
    recs = [(ln, data[s:s + l]) for ln, s, l in WC.split_records(data, match)]
    return encode_cells(recs, filename, nreduce)


def windowed_partitions(pieces, window, match, filename, nreduce):
    """Every call's rows: one list of rows per feed, then the finish's; a row is
    a list of nreduce cells. The walk is window_cases.windowed()'s, kept per
    window: a window without a matching line gives no row."""
    calls, tail = [], b""
    line_base = 0
    for feed in pieces:
        rows = []
        for o in range(0, len(feed), window):
            fill = tail + feed[o:o + window]
            cut = fill.rfind(b"\n")
            if cut < 0:
                tail = fill
                continue
            recs = [(ln, fill[s:s + l]) for ln, s, l in WC.split_records(fill[:cut], match, line_base, 0)]
            if recs:
                rows.append(encode_cells(recs, filename, nreduce))
            line_base += fill[:cut + 1].count(b"\n")
            tail = fill[cut + 1:]
        calls.append(rows)
    recs = [(ln, tail[s:s + l]) for ln, s, l in WC.split_records(tail, match, line_base, 0)]
    calls.append([encode_cells(recs, filename, nreduce)] if recs else [])
    return calls


def joined(calls, nreduce):
    """cells (0,p), (1,p), ... of every call, concatenated per partition"""
    return [b"".join(row[p] for rows in calls for row in rows) for p in range(nreduce)]


def digits_split(W):
    """Line numbers that grow a digit inside a LATER window, not the first: five
    lines fill the first window, then 1,100 short ones -- 9 -> 10 and 99 -> 100
    fall into the second window, 999 -> 1000 into a later one. Every line holds
    `error`. No final '\\n': the last line is the finish's."""
    head = b"".join(b"error " + bytes([0x61 + k]) * (W // 5) + b"\n" for k in range(5))
    assert W < len(head) < W + 64
    return head + b"".join(b"error %d\n" % (k % 7) for k in range(1100)) + b"the last error"


def _cases():
    out = list(WC.CASES)
    for W in WC.WINDOWS:
        data = digits_split(W)
        for fname, cuts in (("whole", []), ("random", WC.random_cuts("digits", len(data), 5))):
            out.append(WC.Case("digits/%s/w%d" % (fname, W), W, data, cuts))
    return out


CASES = _cases()  # window_cases.CASES and the digit crossings


# ---- the local width rule (csrc/kernels/escape_width.h) ------------------------
def _seq_len(b, after):
    """length of the valid UTF-8 sequence starting at b[0] with `after` bytes behind it inside the value, or 0"""
    b0 = b[0]
    lo, hi = 0x80, 0xBF
    if 0xC2 <= b0 <= 0xDF:
        need = 2
    elif 0xE0 <= b0 <= 0xEF:
        need = 3
        if b0 == 0xE0:
            lo = 0xA0
        if b0 == 0xED:
            hi = 0x9F
    elif 0xF0 <= b0 <= 0xF4:
        need = 4
        if b0 == 0xF0:
            lo = 0x90
        if b0 == 0xF4:
            hi = 0x8F
    else:
        return 0
    if need - 1 > after:
        return 0
    if not lo <= b[1] <= hi:
        return 0
    if any(not 0x80 <= b[k] <= 0xBF for k in range(2, need)):
        return 0
    return need


def escape_width(s, i):
    """how many bytes byte i of the value s becomes under Go's JSON escaping, from bytes i-3 .. i+3 alone"""
    L, b = len(s), s[i]
    if b < 0x80:
        if b >= 0x20 and b not in b'"\\<>&':
            return 1
        return 2 if b in b'"\\\n\r\t' else 6
    if b <= 0xBF:
        for k in range(1, min(i, 3) + 1):
            if _seq_len(s[i - k:i - k + 4], L - 1 - (i - k)) > k:
                return 0
        return 6
    need = _seq_len(s[i:i + 4], L - 1 - i)
    if need == 0:
        return 6
    if s[i:i + 3] in (b"\xe2\x80\xa8", b"\xe2\x80\xa9"):
        return 6
    return need


EDGE_BYTES = bytes([0x00, 0x22, 0x41, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xA8, 0xA9, 0xBF, 0xC0, 0xC2, 0xDF, 0xE0,
                    0xE2, 0xED, 0xEF, 0xF0, 0xF4, 0xF5, 0xFF])

_FRAME_HEAD, _FRAME_TAIL = b'{"Key":"","Value":"', b'"}\n'


def go_escaped_len(value):
    """len of the value's body as json.Encoder writes it (the oracle)"""
    line = O.json_kv(b"", value)
    assert line.startswith(_FRAME_HEAD) and line.endswith(_FRAME_TAIL)
    return len(line) - len(_FRAME_HEAD) - len(_FRAME_TAIL)
