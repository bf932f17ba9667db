"""Long escaped values through the resident writer (encode.hip), the batch
writer (encode_batch.hip) and what is built on them (dgrep_grep_job, the pack
route of a windowed job): a value of at least `long value` bytes that needs
escaping takes the chunked path of encode_long.h, and dgrep_last_encode_stats
says how many did. Every expected byte is the oracle's (writer_edge_cases,
window_part_cases, test_gpu_encode_records.expected), never another writer's.

In the host forms the split lies in the library's own buffer, which is aligned
far beyond 16 bytes, so a byte's address phase is its index's; in the device
forms the tests choose the address themselves."""
import numpy as np
import pytest

import window_part_cases as PC
import writer_edge_cases as C
from test_gpu_encode_records import GUARD, _fname_of_json_len, expected
from test_gpu_writer_edges import _same

pytestmark = pytest.mark.gpu

PLAIN = b"edges.log"
CHUNK, STEP = 16384, 4096  # kLongChunk, kLongStep (encode_window.h)
ONE_LANE = 1 << 30         # the largest long value the setter takes: nothing is chunked
ROCKET = b"\xf0\x9f\x98\x80"
_cache = {}


@pytest.fixture
def ctx(gpu_ctx):
    gpu_ctx.load(b"")  # every line matches
    gpu_ctx.set_long_value(256)  # the setter's floor; the tests that say 0 run the writers' default (768)
    yield gpu_ctx
    gpu_ctx.set_long_value(0)


def _whole(data, nreduce=3, fname=PLAIN, match=lambda line: True):
    return PC.whole_partitions(data, match, fname, nreduce)


def _chunks_at(start, length):
    """ceil((end - start rounded down to 16) / kLongChunk), on addresses"""
    return -(-(start + length - (start & ~15)) // CHUNK)


def _long_chunks_of_split(data, base=0, lv=256):
    """the chunks of a split's chunked values when its byte 0 lies at address phase `base`"""
    total, at = 0, base
    for line in data.split(b"\n"):
        if len(line) >= lv and C.needs_escape(line):
            total += _chunks_at(at, len(line))
        at += len(line) + 1
    return total


def _resident(ctx, data, nreduce=3, fname=PLAIN, what="map_partitions"):
    _same(ctx.map_partitions(fname, data, nreduce), _whole(data, nreduce, fname), what)
    return ctx.encode_stats()


def _batch(ctx, files, nreduce=3, what="map_partitions_batch"):
    got = ctx.map_partitions_batch(files, nreduce)
    assert len(got) == len(files)
    for s, (fname, d) in enumerate(files):
        _same(got[s], _whole(d, nreduce, fname), "%s file %d" % (what, s))
    return ctx.encode_stats()


# ---- 1. the de Bruijn values: every 4-gram at every block phase --------------------------
@pytest.mark.parametrize("lv", [0, ONE_LANE])
def test_long_split_resident(ctx, lv):
    data = C.long_split()
    ctx.set_long_value(lv)
    _same(ctx.map_partitions(PLAIN, data, 10), C.partitions("long", data, PLAIN, 10), "map_partitions lv %d" % lv)
    st = ctx.encode_stats()
    assert st["records"] == 33 and st["long_values"] == (16 if lv == 0 else 0), st
    assert st["long_chunks"] == (_long_chunks_of_split(data) if lv == 0 else 0), st
    assert st["encode_ms"] == ctx.last_encode_ms() > 0


@pytest.mark.parametrize("lv", [0, ONE_LANE])
def test_long_split_batch(ctx, lv):
    files = C.cut_files(C.long_split(), 5, b"long")
    ctx.set_long_value(lv)
    got = ctx.map_partitions_batch(files, 10)
    for s, (fname, d) in enumerate(files):
        _same(got[s], C.partitions("long/%d" % s, d, fname, 10), "map_partitions_batch file %d lv %d" % (s, lv))
    st = ctx.encode_stats()
    assert st["records"] == 33 and st["long_values"] == (16 if lv == 0 else 0), st
    at, chunks = 0, 0
    for _, d in files:
        chunks += _long_chunks_of_split(d, at)
        at += len(d) + 1
    assert st["long_chunks"] == (chunks if lv == 0 else 0), st


def _long_job_want():
    if "job" not in _cache:
        _cache["job"] = C.job_outputs(C.long_split(), PLAIN, 10)
    return _cache["job"]


@pytest.mark.parametrize("lv", [0, ONE_LANE])
def test_long_split_grep_job(ctx, lv):
    outs, lines = _long_job_want()
    ctx.set_long_value(lv)
    _same(ctx.grep_job([(PLAIN, C.long_split())], 10), outs, "grep_job lv %d" % lv)
    assert ctx.last_lines_in == lines
    st = ctx.encode_stats()
    assert st["records"] == 33 and st["long_values"] == (16 if lv == 0 else 0), st


@pytest.mark.parametrize("lv", [0, ONE_LANE])
def test_long_split_job_pack_route(ctx, lv):
    """a file given whole, below the window: the pack route's batch encode"""
    data = C.long_split()
    outs, lines = _long_job_want()
    window = 8 << 20
    assert len(data) < window
    ctx.set_long_value(lv)
    with ctx.job(window, 10) as job:
        job.add(PLAIN, data)
        got = job.finish()
        stats = job.stats()
    _same(got, outs, "job, packed, lv %d" % lv)
    assert ctx.last_lines_in == lines
    assert stats["files_packed"] == 1 and stats["files_windowed"] == 0, stats
    assert stats["long_values"] == 0, stats  # the window route's count only
    st = ctx.encode_stats()  # the sums over the job's packs
    assert st["records"] == 33 and st["long_values"] == (16 if lv == 0 else 0), st


def test_job_stats_sum_over_packs(ctx):
    """two packs (the second file does not fit beside the first): the sums, not the last pack's"""
    a = b'first "a" ' + b"a" * 5000 + b"\nplain"
    b = b"plain\n" + b'second "b" ' + b"b" * 6000 + b'\nthird "c" ' + b"c" * 300
    files = [(b"a.log", a), (b"b.log", b)]
    with ctx.job(8192, 3) as job:
        for f, d in files:
            job.add(f, d)
        job.finish()
        stats = job.stats()
    assert stats["packs"] == 2 and stats["files_packed"] == 2, stats
    assert sum(ctx.last_lines_in) == 5
    st = ctx.encode_stats()
    assert (st["records"], st["long_values"], st["long_chunks"]) == (5, 3, 3), st


# ---- 2. random values: the counts on both sides of the switch -------------------------------------
@pytest.mark.parametrize("lv", [256, ONE_LANE])
def test_random_split_resident(ctx, lv):
    data = C.random_split()
    ctx.set_long_value(lv)
    _same(ctx.map_partitions(PLAIN, data, 10), C.partitions("random", data, PLAIN, 10), "map_partitions lv %d" % lv)
    st = ctx.encode_stats()
    assert st["long_values"] == C.chunked(C.values_of(data), lv), st
    assert st["long_chunks"] == _long_chunks_of_split(data, 0, lv), st


@pytest.mark.parametrize("lv", [256, ONE_LANE])
def test_random_split_batch(ctx, lv):
    files = C.cut_files(C.random_split(), 5, b"random")
    ctx.set_long_value(lv)
    got = ctx.map_partitions_batch(files, 10)
    for s, (fname, d) in enumerate(files):
        _same(got[s], C.partitions("random/%d" % s, d, fname, 10), "map_partitions_batch file %d lv %d" % (s, lv))
    st = ctx.encode_stats()
    assert st["long_values"] == sum(C.chunked(C.values_of(d), lv) for _, d in files), st


# ---- 3. the threshold --------------------------------------------------------------------
@pytest.mark.parametrize("lv", [256, 320])
def test_threshold(ctx, lv):
    ctx.set_long_value(lv)
    for length, want in ((lv - 1, 0), (lv, 1), (lv + 1, 1)):
        value = b"a" * 100 + b'"' + b"a" * (length - 101)
        data = b"before\n" + value + b"\nafter"
        assert _resident(ctx, data)["long_values"] == want, (lv, length)
        assert _batch(ctx, [(PLAIN, data)])["long_values"] == want, (lv, length)
        plain = b"a" * length  # nothing to escape: never chunked
        assert _resident(ctx, b"before\n" + plain)["long_values"] == 0


# ---- 4. block, step and chunk edges ----------------------------------------------------------
@pytest.mark.parametrize("seq", [ROCKET, b"\xe2\x80"], ids=["whole", "truncated"])
@pytest.mark.parametrize("edge", [16, STEP, CHUNK])
def test_sequence_across_an_edge(ctx, edge, seq):
    """a single value: a 4-byte sequence (or a cut-off one, then ASCII) with
    its lead 3, 2, 1 and 0 bytes before a 16-byte block edge, a 4 KiB step edge
    and the 16 KiB chunk edge. The value is the split, so it starts at phase 0."""
    for back in (3, 2, 1, 0):
        value = b"a" * (edge - back) + seq + b"z" * 300
        st = _resident(ctx, value, 1, what="edge %d back %d" % (edge, back))
        assert st["long_values"] == 1 and st["long_chunks"] == _chunks_at(0, len(value)), (edge, back, st)
        st = _batch(ctx, [(b"x", b"xy"), (PLAIN, value)], 1)  # the value starts at phase 3
        assert st["long_values"] == 1 and st["long_chunks"] == _chunks_at(3, len(value)), (edge, back, st)


@pytest.mark.parametrize("phase", [0, 1, 15])
def test_values_of_one_chunk(ctx, phase):
    """16,384 - 1, 16,384 and 16,384 + 1 bytes, the value's first byte at phase 0, 1 and 15"""
    lead = b"" if phase == 0 else b"p" * (phase - 1) + b"\n"
    for length in (CHUNK - 1, CHUNK, CHUNK + 1):
        value = b'"' + b"a" * (length - 2) + b"\xc3"
        st = _resident(ctx, lead + value, 1, what="length %d at phase %d" % (length, phase))
        assert st["long_values"] == 1 and st["long_chunks"] == _chunks_at(phase, length), (phase, length, st)
        st = _batch(ctx, [(PLAIN, lead + value)], 1)
        assert st["long_values"] == 1 and st["long_chunks"] == _chunks_at(phase, length), (phase, length, st)
    assert {_chunks_at(p, n) for p in (0, 1, 15) for n in (CHUNK - 1, CHUNK, CHUNK + 1)} == {1, 2}


# ---- 5. the device form over the caller's buffer ------------------------------------------------
def _device_case(tail):
    """(data, records): plain lines, a short escaped one, and a last line that is a long
    escaped value of more than one chunk, without '\\n', ending at n with n % 16 == tail"""
    lines = [b"plain line", b'short "escaped" <line>', b"p" * 40]
    head = b"\n".join(lines) + b"\n"
    value = b'\xe2\x80\xa8"' + (b"abcdefg\\" * 2200) + ROCKET + b"\xf0\x9f"
    value += b"." * ((tail - len(head) - len(value)) % 16)
    data = head + value
    assert len(data) % 16 == tail and len(value) > CHUNK
    recs, at = [], 0
    for k, ln in enumerate(lines + [value]):
        recs.append((k + 1, at, len(ln)))
        at += len(ln) + 1
    return data, recs


@pytest.mark.parametrize("tail", [0, 1, 15])
def test_encode_device_at_every_address_phase(ctx, tail):
    """d_data = a tensor of exactly off + n bytes, + off: the long value ends with the allocation"""
    import torch

    data, recs = _device_case(tail)
    n = len(data)
    want = expected(data, recs, PLAIN, 2)
    cols = np.asarray(recs, dtype=np.uint64)
    dev = [torch.from_numpy(np.ascontiguousarray(cols[:, k]).view(np.int64).copy()).cuda() for k in range(3)]
    for off in range(16):
        buf = torch.from_numpy(np.frombuffer(b"\xf0" * off + data, dtype=np.uint8).copy()).cuda()
        assert buf.numel() == off + n and buf.data_ptr() % 16 == 0
        ptr = buf.data_ptr() + off
        _, _, total = ctx.encode_device(ptr, n, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), len(recs),
                                        PLAIN, 2, 0, 0)
        assert total == sum(len(w) for w in want), off
        out = torch.full((total + 64,), GUARD, dtype=torch.uint8, device="cuda")
        b, e, total2 = ctx.encode_device(ptr, n, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), len(recs),
                                         PLAIN, 2, out.data_ptr(), total)
        raw = out.cpu().numpy().tobytes()
        assert total2 == total and raw[total:] == bytes([GUARD]) * 64, off
        _same([raw[x:y] for x, y in zip(b, e)], [bytes(w) for w in want], "encode_device off %d tail %d" % (off, tail))
        st = ctx.encode_stats()
        assert st["records"] == 4 and st["long_values"] == 1, (off, st)
        assert st["long_chunks"] == _chunks_at(ptr + recs[-1][1], recs[-1][2]), (off, st)


# ---- 6. the capacity contract with a long value ---------------------------------------------------
def _capacity_records():
    value = b'say "' + b"0123456789abcde<" * 1100 + b'"'
    lines = [b"first line", b'a "short" one', value, b"after the long line", b"last"]
    data = b"\n".join(lines)
    recs, at = [], 0
    for k, ln in enumerate(lines):
        recs.append((k + 1, at, len(ln)))
        at += len(ln) + 1
    return data, recs


def _caps(lines_enc):
    """out_cap: 0; inside the long line's head; inside its value; total - 1; total"""
    before = sum(len(x) for x in lines_enc[:2])
    total = sum(len(x) for x in lines_enc)
    return [0, before + 10, before + len(lines_enc[2]) // 2, total - 1, total]


def _check_capacity(encode, lines_enc, what):
    """encode(out tensor, out_cap) -> total. Lines are in output order."""
    import torch

    whole = b"".join(lines_enc)
    total = len(whole)
    ends = np.cumsum([len(x) for x in lines_enc]).tolist()
    out = torch.full((total + 64,), GUARD, dtype=torch.uint8, device="cuda")
    for cap in _caps(lines_enc):
        out.fill_(GUARD)
        assert encode(out, cap) == total, (what, cap)  # the bytes needed, whatever the room
        raw = out.cpu().numpy().tobytes()
        fit = max([0] + [x for x in ends if x <= cap])  # a line that does not fit is left out whole
        assert raw[:fit] == whole[:fit], (what, cap)
        assert raw[fit:] == bytes([GUARD]) * (total + 64 - fit), (what, cap, fit)
        # a following call with the full buffer: the short call left nothing behind
        assert encode(out, total) == total, (what, cap)
        raw = out.cpu().numpy().tobytes()
        assert raw[:total] == whole and raw[total:] == bytes([GUARD]) * 64, (what, cap)


def test_capacity_encode_device(ctx):
    import torch

    data, recs = _capacity_records()
    lines_enc = [bytes(expected(data, [r], PLAIN, 1)[0]) for r in recs]
    buf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    cols = np.asarray(recs, dtype=np.uint64)
    dev = [torch.from_numpy(np.ascontiguousarray(cols[:, k]).view(np.int64).copy()).cuda() for k in range(3)]

    def encode(out, cap):
        b, e, total = ctx.encode_device(buf.data_ptr(), len(data), dev[0].data_ptr(), dev[1].data_ptr(),
                                        dev[2].data_ptr(), len(recs), PLAIN, 1, out.data_ptr(), cap)
        assert (b[0], e[0]) == (0, total) and ctx.encode_stats()["long_values"] == 1
        return total

    _check_capacity(encode, lines_enc, "encode_device")


def test_capacity_encode_batch_device(ctx):
    """two splits in one packed buffer; the long line is the first split's third"""
    import torch

    data, recs = _capacity_records()
    second = b"a second split\nwith an <escaped> line"
    recs2 = [(1, 0, 14), (2, 15, 22)]
    names = [PLAIN, b"second.log"]
    lines_enc = [bytes(expected(data, [r], names[0], 1)[0]) for r in recs]
    lines_enc += [bytes(expected(second, [r], names[1], 1)[0]) for r in recs2]
    packed = data + b"\n" + second
    buf = torch.from_numpy(np.frombuffer(packed, dtype=np.uint8).copy()).cuda()
    cols = np.asarray(recs + recs2, dtype=np.uint64)
    dev = [torch.from_numpy(np.ascontiguousarray(cols[:, k]).view(np.int64).copy()).cuda() for k in range(3)]
    split = torch.from_numpy(np.array([0] * len(recs) + [1] * len(recs2), dtype=np.int32)).cuda()
    off = [0, sum(len(x) for x in lines_enc[:len(recs)]), sum(len(x) for x in lines_enc)]

    def encode(out, cap):
        cell_off, total = ctx.encode_batch_device(buf.data_ptr(), len(packed), [len(data), len(second)],
                                                  dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(),
                                                  split.data_ptr(), len(cols), names, 1, out.data_ptr(), cap)
        assert cell_off == off and ctx.encode_stats()["long_values"] == 1
        return total

    _check_capacity(encode, lines_enc, "encode_batch_device")


# ---- 7. the writers' corners ------------------------------------------------------------------
LONG_A = b'{"k":"' + b'v","k":"' * 700 + b'"}'        # 5.6 KB of minified JSON
LONG_B = b"\xff" * 300                                # every byte 6 wide
LONG_C = (ROCKET + b"\xe2\x80\xa9") * 3000 + b"\xf0"  # 21 KB: two chunks, valid sequences across every edge


def test_a_long_value_alone(ctx):
    for value in (LONG_A, LONG_B, LONG_C):
        assert _resident(ctx, value)["long_values"] == 1
        assert _batch(ctx, [(PLAIN, value)])["long_values"] == 1


def test_a_long_value_that_keeps_its_length(ctx):
    """valid UTF-8 and nothing else to escape: measured by the chunk pass, its bytes unchanged"""
    value = "zażółć gęślą jaźń ".encode() * 40
    assert len(C.body(value)) == len(value) and C.needs_escape(value)
    data = b"before\n" + value + b"\n" + value[1:] + b"\nafter"
    assert _resident(ctx, data)["long_values"] == 2
    assert _batch(ctx, [(PLAIN, data), (b"second", value)])["long_values"] == 3


def test_no_records(ctx):
    ctx.load(b"no line has this")
    data = b"before\n" + LONG_A + b"\nafter"
    assert ctx.map_partitions(PLAIN, data, 3) == [b""] * 3
    st = ctx.encode_stats()
    assert (st["records"], st["long_values"], st["long_chunks"]) == (0, 0, 0), st
    assert ctx.map_partitions_batch([(PLAIN, data), (b"b", data)], 3) == [[b""] * 3] * 2
    st = ctx.encode_stats()
    assert (st["records"], st["long_values"], st["long_chunks"]) == (0, 0, 0), st


def test_two_long_values_on_adjacent_lines(ctx):
    data = LONG_A + b"\n" + LONG_C + b"\n" + LONG_B
    assert _resident(ctx, data)["long_values"] == 3
    assert _batch(ctx, [(PLAIN, data)])["long_values"] == 3


def test_many_long_values(ctx):
    """300 values of 300 escaped bytes: more long records than a workgroup has lanes, a chunk each"""
    values = [bytes([0x22, 0x5C, 0x3C, 0xFF, 0x41 + k % 26]) * 60 for k in range(300)]
    data = b"\n".join(values)
    st = _resident(ctx, data, 10)
    assert (st["records"], st["long_values"]) == (300, 300) and st["long_chunks"] == _long_chunks_of_split(data), st
    files = C.cut_files(data, 3, b"many")
    st = _batch(ctx, files, 10)
    assert (st["records"], st["long_values"]) == (300, 300), st


def test_more_chunks_than_the_grid(ctx):
    """One value of 4,100 chunks: the chunk kernels launch at most 4,096
    workgroups, so some take a second chunk and reuse their LDS partials."""
    unit = b'abcdefg"' + ROCKET + b"\xe2\x80\xa8xy<" + b"0123456789" + b"\xff"
    value = (unit * (4100 * CHUNK // len(unit) + 1))[:4100 * CHUNK - 5]
    data = b"before\n" + value + b"\nafter"
    st = _resident(ctx, data, 1, what="4,100 chunks")
    assert st["long_values"] == 1 and st["long_chunks"] == _chunks_at(7, len(value)) > 4096, st
    st = _batch(ctx, [(PLAIN, data)], 1, what="4,100 chunks")
    assert st["long_values"] == 1 and st["long_chunks"] == _chunks_at(7, len(value)), st


def test_file_name_past_the_lds_head(ctx):
    """the per-thread line writer leaves the value's place to the chunk pass"""
    fname = _fname_of_json_len(2026, True)
    data = b"before\n" + LONG_A + b"\n" + LONG_C + b"\nafter"
    assert _resident(ctx, data, 3, fname)["long_values"] == 2
    assert _batch(ctx, [(fname, data), (PLAIN, data)], 3)["long_values"] == 4


def test_batch_splits_at_every_phase(ctx):
    """17 splits of a multiple of 16 bytes each: with the separators, begin[] takes every phase"""
    files = []
    for s in range(17):
        body = b"split %d\n" % s
        if s in (0, 8, 16):
            body += LONG_C[:-1 - s] + b"\n"
        body += b"last line of the split "
        body += b"." * (-len(body) % 16)
        files.append((b"phase-%d.log" % s, body))
    begins = np.cumsum([0] + [len(d) + 1 for _, d in files[:-1]])
    assert {int(b) % 16 for b in begins} == set(range(16))
    st = _batch(ctx, files, 3)
    assert st["long_values"] == 3, st
    assert st["long_chunks"] == sum(_long_chunks_of_split(d, int(b)) for (_, d), b in zip(files, begins)), st


def test_only_the_long_lines_match(ctx):
    ctx.load(b"error")
    lines = []
    for k in range(40):
        lines.append(b"nothing to see in line %d" % k)
        if k % 13 == 5:
            lines.append(b'{"level":"error","blob":"' + bytes([0x80 + k, 0x22]) * (200 + 40 * k) + b'"}')
    data = b"\n".join(lines)

    def match(line):
        return b"error" in line

    _same(ctx.map_partitions(PLAIN, data, 3), _whole(data, 3, PLAIN, match), "map_partitions, error")
    st = ctx.encode_stats()
    assert (st["records"], st["long_values"]) == (3, 3), st
    got = ctx.map_partitions_batch([(PLAIN, data), (b"none", b"no match here\n")], 3)
    _same(got[0], _whole(data, 3, PLAIN, match), "map_partitions_batch, error")
    assert got[1] == [b""] * 3
    assert ctx.encode_stats()["long_values"] == 3


def test_regressions_as_long_values(ctx):
    """every value that ever failed on a writer, made long, alone between two plain lines"""
    for name, value in C.REGRESSIONS:
        data = b"before\n" + b"a" * 256 + value + b"\nafter"
        assert _resident(ctx, data, what=name)["long_values"] == 1, name
        assert _batch(ctx, [(PLAIN, data)], what=name)["long_values"] == 1, name


def test_overlapping_records_fall_back_to_one_lane(ctx):
    """Records made by hand may overlap, so that their chunks outnumber the
    tables' bound, which assumes values that lie apart: the values that do not
    fit are written by one lane, and the bytes are the same."""
    import torch

    data = b'"' + b"a" * 299 + b"<"
    recs = [(k + 1, k % 40, len(data) - k % 40) for k in range(12)]
    want = expected(data, recs, PLAIN, 1)
    buf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    cols = np.asarray(recs, dtype=np.uint64)
    dev = [torch.from_numpy(np.ascontiguousarray(cols[:, k]).view(np.int64).copy()).cuda() for k in range(3)]
    total = len(want[0])
    out = torch.full((total + 64,), GUARD, dtype=torch.uint8, device="cuda")
    b, e, t = ctx.encode_device(buf.data_ptr(), len(data), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(),
                                len(recs), PLAIN, 1, out.data_ptr(), total)
    raw = out.cpu().numpy().tobytes()
    assert t == total and raw[total:] == bytes([GUARD]) * 64
    _same([raw[:total]], [bytes(want[0])], "overlapping records")
    st = ctx.encode_stats()
    assert st["records"] == 12 and 1 <= st["long_values"] < 12 and st["long_chunks"] == st["long_values"], st
