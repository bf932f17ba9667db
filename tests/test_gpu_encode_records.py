"""The partition + intermediate writer (dgrep_encode_device) over records the
test writes itself -- no scan -- so that the writer's own edges are reached:
64-bit line numbers, the 2 KiB LDS head boundary, nreduce beyond 256, records
touching the split's last bytes, an output buffer one byte short. Expected
partitions: the oracle's Sprintf key, ihash and json.Encoder line over the same
records in record order (map_reduce/worker.go:78-109). Bit-exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_lib as O  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def expected(data: bytes, recs, fname: bytes, nreduce: int):
    parts = [bytearray() for _ in range(nreduce)]
    for ln, st, le in recs:
        key = O.format_key(fname, ln)
        parts[O.ihash(key) % nreduce] += O.json_kv(key, data[st:st + le])
    return parts


class Split:
    """The split and its records in device memory. Bytes that would need
    escaping follow the split's n bytes, so a read past n shows."""

    def __init__(self, data: bytes, recs):
        import torch

        self.data, self.recs, self.n = data, recs, len(data)
        host = np.frombuffer(data + b'"\\<\xff' * 16, dtype=np.uint8).copy()
        self.buf = torch.from_numpy(host).cuda()
        cols = np.asarray(recs, dtype=np.uint64).reshape(-1, 3)  # (line number, start, length) rows
        self.cols = [torch.from_numpy(np.ascontiguousarray(cols[:, k]).view(np.int64).copy()).cuda() for k in range(3)]

    def encode(self, ctx, fname: bytes, nreduce: int, out=None, out_cap=None):
        """(begin, end, total, out tensor): sized by a first call unless `out` is given."""
        import torch

        ptr = [c.data_ptr() if len(self.recs) else 0 for c in self.cols]
        if out is None:
            _, _, total = ctx.encode_device(self.buf.data_ptr(), self.n, ptr[0], ptr[1], ptr[2], len(self.recs), fname,
                                            nreduce, 0, 0)
            out = torch.full((total + 64,), GUARD, dtype=torch.uint8, device="cuda")
            out_cap = total
        b, e, total = ctx.encode_device(self.buf.data_ptr(), self.n, ptr[0], ptr[1], ptr[2], len(self.recs), fname,
                                        nreduce, out.data_ptr(), out_cap)
        return b, e, total, out


def check(ctx, data: bytes, recs, fname: bytes, nreduce: int):
    sp = Split(data, recs)
    b, e, total, out = sp.encode(ctx, fname, nreduce)
    raw = out.cpu().numpy().tobytes()
    want = expected(data, sp.recs, fname, nreduce)
    assert total == sum(len(w) for w in want)
    assert raw[total:] == bytes([GUARD]) * 64
    for p in range(nreduce):
        if not want[p]:
            assert b[p] == e[p], p
        else:
            assert raw[b[p]:e[p]] == want[p], (p, raw[b[p]:e[p]][:200], bytes(want[p][:200]))
    # the partitions tile [0, total) in partition order
    at = 0
    for p in range(nreduce):
        if want[p]:
            assert b[p] == at
            at = e[p]
    assert at == total


def text_split(nlines=400, seed=3):
    """Lines of every length 0..40 (every start phase mod 4), some with bytes
    json.Encoder escapes; records = (line number, start, length) of every line."""
    rnd = np.random.RandomState(seed)
    lines = []
    for k in range(nlines):
        body = bytes(rnd.randint(0x23, 0x7b, size=k % 41).astype(np.uint8)).replace(b"\\", b"_").replace(b"<", b"_")
        body = body.replace(b">", b"_").replace(b"&", b"_")
        if k % 7 == 3:
            body = body[:k % 5] + b'<"\xff\xe2\x80\xa8\t' + body[k % 5:]
        lines.append(body)
    data = b"\n".join(lines)
    recs, at = [], 0
    for k, ln in enumerate(lines):
        recs.append((k + 1, at, len(ln)))
        at += len(ln) + 1
    return data, recs


LINE_NUMBERS = sorted({10 ** k - 1 for k in range(1, 20)} | {10 ** k for k in range(1, 20)} |
                      {2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1})


def test_oracle_formats_64_bit_line_numbers():
    for v in LINE_NUMBERS:
        assert O.format_key(b"f", v) == b"f (line number #%d)" % v


@pytest.mark.parametrize("nreduce", [1, 10])
def test_line_numbers_to_64_bits(gpu_ctx, nreduce):
    """9/10, 99/100, ..., 2^32 +- 1, 2^63, 2^64 - 1 side by side, so digit counts
    differ between neighbouring lanes of a wave; repeated to fill several
    waves, in both orders."""
    data = b"error: plain value\n<escaped> value"
    recs = []
    for rep in range(4):
        for k, v in enumerate(LINE_NUMBERS if rep % 2 == 0 else LINE_NUMBERS[::-1]):
            recs.append((v, 0, 18) if (k + rep) % 3 else (v, 19, 15))
    assert len(recs) > 64
    check(gpu_ctx, data, recs, b"split.log", nreduce)


def test_digit_rows_reused_across_rounds(gpu_ctx):
    """More records than one launch's waves take in one round (4096 workgroups
    x 4 waves x 64 lines): the second round rewrites the waves' LDS digit rows.
    nreduce = 1 keeps record order; the first and the last lines and the total
    are checked against the oracle."""
    data = b"error"
    count = 4096 * 4 * 64 + 333
    reps = -(-count // len(LINE_NUMBERS))
    ln = np.tile(np.array(LINE_NUMBERS, dtype=np.uint64), reps)[:count]
    ln[1::2] = ln[1::2][::-1].copy()  # neighbours with unrelated digit counts
    sp = Split(data, np.stack([ln, np.zeros(count, np.uint64), np.full(count, 5, np.uint64)], axis=1))
    ln = ln.tolist()
    b, e, total, out = sp.encode(gpu_ctx, b"f", 1)
    assert total == sum(len(b'{"Key":"f (line number #%d)","Value":"error"}\n' % v) for v in ln)
    assert (b[0], e[0]) == (0, total)
    raw = out.cpu().numpy().tobytes()
    head = b"".join(O.json_kv(O.format_key(b"f", v), data) for v in ln[:600])
    tail = b"".join(O.json_kv(O.format_key(b"f", v), data) for v in ln[-1200:])
    assert raw[:len(head)] == head
    assert raw[total - len(tail):total] == tail
    assert raw[total:] == bytes([GUARD]) * 64


def _fname_of_json_len(n: int, escaped: bool) -> bytes:
    name = b"<" * (n // 6 - 1) + b"e" * (n - 6 * (n // 6 - 1)) if escaped else b"f" * n
    assert len(O.json_kv(name, b"")) - len(O.json_kv(b"", b"")) == n
    return name


@pytest.mark.parametrize("escaped", [False, True])
@pytest.mark.parametrize("json_len", [2024, 2025, 2026])
def test_head_boundary(gpu_ctx, json_len, escaped):
    """`{"Key":"<file> (line number #` is 8 + json_len + 15 bytes: 2025 fills the
    wave writer's head[2048] exactly, 2026 takes the per-thread writer, whose
    dword copy runs at every source phase (plain values of 8 bytes and more)."""
    data, recs = text_split()
    assert {st % 4 for _, st, le in recs if le >= 8} == {0, 1, 2, 3}
    for nreduce in (1, 3):
        check(gpu_ctx, data, recs, _fname_of_json_len(json_len, escaped), nreduce)


@pytest.mark.parametrize("nreduce", [2, 255, 256, 257, 4096, 65535])
def test_nreduce_beyond_a_byte(gpu_ctx, nreduce):
    data, recs = text_split(3000, seed=nreduce)
    check(gpu_ctx, data, recs, b"split-0007.log", nreduce)


def test_nreduce_out_of_range(gpu_ctx):
    import dgrep

    sp = Split(b"error", [(1, 0, 5)])
    for nreduce in (0, 65536):
        with pytest.raises(dgrep.DgrepError):
            sp.encode(gpu_ctx, b"f", nreduce)
    check(gpu_ctx, b"error", [(1, 0, 5)], b"f", 65535)


@pytest.mark.parametrize("tail", [1, 2, 3, 0])
def test_record_shapes(gpu_ctx, tail):
    """Split lengths n with n % 4 == tail; records at both ends of the split."""
    body = b"first line\n" + b"p" * 300 + b"\nlast plain value"
    body += b"." * ((tail - len(body)) % 4)
    esc = body[:-3] + b'"<\xe2'  # an escaped value (and a truncated rune) ending at n - 1
    for data in (body, esc):
        n = len(data)
        assert n % 4 == tail
        last = data.rfind(b"\n") + 1
        recs = [(1, 0, 0), (2, n, 0), (3, 0, n), (4, last, n - last), (5, n - 1, 1), (6, n - 5, 5), (7, n - 9, 9),
                (8, n - 300, 300), (9, 0, 10), (10, 11, 300), (2 ** 40, n - 4, 4), (12, n - 8, 8)]
        for fname in (b"s.log", b"f" * 2026):
            check(gpu_ctx, data, recs, fname, 1)
            check(gpu_ctx, data, recs[::-1], fname, 1)  # order inside a partition follows record order
            check(gpu_ctx, data, recs[::-1] + recs, fname, 3)
    check(gpu_ctx, body, [], b"s.log", 5)  # count == 0


@pytest.mark.parametrize("fname", [b"s.log", b"f" * 2026], ids=["wave-writer", "thread-writer"])
@pytest.mark.parametrize("nreduce", [1, 3])
def test_capacity_one_byte_short(gpu_ctx, fname, nreduce):
    import torch

    data, recs = text_split(300)
    sp = Split(data, recs)
    want = expected(data, recs, fname, nreduce)
    whole = b"".join(bytes(w) for w in want)
    total = len(whole)
    out = torch.full((total + 64,), GUARD, dtype=torch.uint8, device="cuda")
    b, e, t, _ = sp.encode(gpu_ctx, fname, nreduce, out=out, out_cap=total - 1)
    assert t == total  # the bytes needed, as with room
    raw = out.cpu().numpy().tobytes()
    # only the last line does not fit: it is left out whole, nothing lands at or past out_cap
    last = len(bytes(want[-1]).rstrip(b"\n").rpartition(b"\n")[2]) + 1 if want[-1] else None
    assert last is not None
    assert raw[:total - last] == whole[:total - last]
    assert raw[total - last:] == bytes([GUARD]) * (64 + last)
    b, e, t, _ = sp.encode(gpu_ctx, fname, nreduce, out=out, out_cap=total)
    assert t == total
    raw = out.cpu().numpy().tobytes()
    assert raw[:total] == whole and raw[total:] == bytes([GUARD]) * 64
    assert [raw[x:y] for x, y in zip(b, e)] == [bytes(w) for w in want]
