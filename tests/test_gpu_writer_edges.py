"""Every UTF-8 and escape edge through all four partition writers on the GPU:
the resident writer (encode.hip), the batch writer (encode_batch.hip), the
windowed writer (encode_window.hip: the one-lane escaper and the chunked
long-value path) and the job's pack and window routes that reuse them. The
inputs are tests/writer_edge_cases.py's; every comparison is byte for byte
against the oracle (oracle_lib.json_kv, format_key, ihash), never one writer
against another. tests/test_writer_edge_cases.py holds the same values against
the host-compiled escapers, so a mismatch here is a device-side fault.

What only the device code has, and what reaches it here: json_body compiled for
the device (measure and write) on every string of 0..4 bytes over the edge
alphabet, as lines and as records inside a buffer; special_bytes, range_mask and
the ballot on every byte alone among plain ASCII; long_chunk_kernel's 24-byte
window with its halo dwords, the clips at the value's ends, the per-step
workgroup scan and the chunk offsets on a de Bruijn value at 16 paddings, where
no two lanes of a step share a width sum.
"""
import numpy as np
import pytest

import job_window_cases as JW
import window_cases as WC
import window_part_cases as PC
import writer_edge_cases as C
from test_gpu_encode_records import GUARD, Split, _fname_of_json_len

pytestmark = pytest.mark.gpu

PLAIN = b"edges.log"
PIECE = 10007  # the streams' feeds: cuts at no line, block or window edge
NAMES = {"plain": PLAIN, "truncated": b"n\xe2\x80", "thread-writer": _fname_of_json_len(2026, True), "empty": b""}

# (split, long_value) -> the long_values a stream over the split reported, for the tally
_seen = {}


def _same(got, want, what):
    """byte for byte, partition by partition; the message names the first byte that differs"""
    assert len(got) == len(want), (what, len(got), len(want))
    for p, (g, w) in enumerate(zip(got, want)):
        if g != w:
            k = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
            lo = max(w.rfind(b"\n", 0, k) + 1, k - 200)
            raise AssertionError("%s: partition %d has %d bytes, the oracle %d; first difference at %d: %r, the oracle's %r"
                                 % (what, p, len(g), len(w), k, g[lo:k + 40], w[lo:k + 40]))


def _stream(ctx, name, pieces, W, R, lv):
    """a partition stream over the pieces: the cells joined per partition, and its long_values"""
    with ctx.partition_stream(W, PLAIN, R) as st:
        calls = [st.feed(p) for p in pieces] + [st.finish()]
        stats = st.stats()
    _seen[(name, lv)] = stats["long_values"]
    return PC.joined(calls, R), stats


def _fed(data, step=PIECE):
    return [data[i:i + step] for i in range(0, len(data), step)]


def _job_want(name, files, R):
    k = ("job", name, R)
    if k not in C._parts:
        C._parts[k] = JW.expected_job(b"", files, R)
    return C._parts[k]


@pytest.fixture
def ctx(gpu_ctx):
    gpu_ctx.load(b"")  # every line matches
    yield gpu_ctx
    gpu_ctx.set_long_value(0)


# ---- 1. short values, split form ------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NAMES))
def test_short_values_resident(ctx, name):
    data, fname = C.short_split(), NAMES[name]
    _same(ctx.map_partitions(fname, data, 10), C.partitions("short", data, fname, 10), "map_partitions " + name)


def _short_files():
    return C.cut_files(C.short_split(), 7, b"short")


def test_short_values_batch(ctx):
    files = _short_files()
    got = ctx.map_partitions_batch(files, 10)
    assert len(got) == 7
    for s, (fname, d) in enumerate(files):
        _same(got[s], C.partitions("short/%d" % s, d, fname, 10), "map_partitions_batch file %d" % s)


@pytest.mark.parametrize("lv", [256, 1 << 30])
def test_short_values_windowed(ctx, lv):
    data = C.short_split()
    want = C.partitions("short", data, PLAIN, 10)
    ctx.set_long_value(lv)
    _same(ctx.map_partitions_windowed(PLAIN, data, 10, 4096), want, "map_partitions_windowed lv %d" % lv)
    got, stats = _stream(ctx, "short", _fed(data), 4096, 10, lv)
    _same(got, want, "partition_stream fed %d bytes a call, lv %d" % (PIECE, lv))
    assert stats["long_values"] == 0 and stats["windows"] >= len(data) // 4096, stats


def test_short_values_job_and_windowed_job(ctx):
    """the pack route and the window route, and every edge through the reduce parser"""
    files = _short_files()
    outs, lines = _job_want("short", files, 10)
    assert sum(lines) == C.short_split().count(b"\n") + 1
    _same(ctx.grep_job(files, 10), outs, "grep_job")
    assert ctx.last_lines_in == lines
    _same(ctx.grep_job_windowed(files, 10, 8192), outs, "grep_job_windowed")
    assert ctx.last_lines_in == lines


# ---- 2. short values, record form ---------------------------------------------------------
def test_records_encode_device(ctx):
    buf, recs = C.record_cases()
    want, _ = C.record_expected(buf, recs, [PLAIN])
    sp = Split(buf, recs)
    b, e, total, out = sp.encode(ctx, PLAIN, 1)
    assert total == len(want) and (b[0], e[0]) == (0, total)
    raw = out.cpu().numpy().tobytes()
    _same([raw[:total]], [want], "encode_device")
    assert raw[total:] == bytes([GUARD]) * 64


def test_records_encode_batch_device(ctx):
    """the buffer twice, packed as two splits: the second begins at no aligned
    offset, and its records are the second half of the records"""
    import torch

    buf, recs = C.record_cases()
    half = len(recs) // 2
    names = [PLAIN, b'second "split".log']
    split_of = [0] * half + [1] * (len(recs) - half)
    want, off = C.record_expected(buf, recs, names, split_of)
    packed = buf + b"\n" + buf
    assert (len(buf) + 1) % 16 != 0
    data_t = torch.from_numpy(np.frombuffer(packed + b'"\\<\xff' * 16, dtype=np.uint8).copy()).cuda()
    cols = [torch.from_numpy(np.ascontiguousarray(recs[:, k]).view(np.int64).copy()).cuda() for k in range(3)]
    sp_t = torch.from_numpy(np.array(split_of, dtype=np.int32)).cuda()

    def encode(out_ptr, cap):
        return ctx.encode_batch_device(data_t.data_ptr(), len(packed), [len(buf), len(buf)], cols[0].data_ptr(),
                                       cols[1].data_ptr(), cols[2].data_ptr(), sp_t.data_ptr(), len(recs), names, 1,
                                       out_ptr, cap)

    cell_off, total = encode(0, 0)
    assert total == len(want) and cell_off == off
    out = torch.full((total + 64,), GUARD, dtype=torch.uint8, device="cuda")
    cell_off, total2 = encode(out.data_ptr(), total)
    assert total2 == total and cell_off == off
    raw = out.cpu().numpy().tobytes()
    _same([raw[off[0]:off[1]], raw[off[1]:off[2]]], [want[off[0]:off[1]], want[off[1]:off[2]]], "encode_batch_device")
    assert raw[total:] == bytes([GUARD]) * 64


# ---- 3. long values -----------------------------------------------------------------------------
@pytest.mark.parametrize("W", [65536, 1 << 20])
def test_long_values_windowed(ctx, W):
    """At 64 KiB the 280 KB lines grow the carried tail; at 1 MiB several lines share a window."""
    data = C.long_split()
    want = C.partitions("long", data, PLAIN, 10)
    ctx.set_long_value(256)
    _same(ctx.map_partitions_windowed(PLAIN, data, 10, W), want, "map_partitions_windowed W %d" % W)


def test_long_values_stream_random_cuts(ctx):
    data = C.long_split()
    ctx.set_long_value(256)
    pieces = WC.pieces_of(data, WC.random_cuts("writer edges long", len(data), 9))
    got, stats = _stream(ctx, "long", pieces, 65536, 10, 256)
    _same(got, C.partitions("long", data, PLAIN, 10), "partition_stream with random cuts")
    assert stats["long_values"] == 16 and stats["max_carry"] >= len(C.de_bruijn()), stats


def test_long_values_job_window_route(ctx):
    data = C.long_split()
    outs, lines = C.job_outputs(data, PLAIN, 10)
    ctx.set_long_value(256)
    with ctx.job(65536, 10) as job:
        job.begin(PLAIN)
        for piece in _fed(data, 300007):
            job.feed(piece)
        job.end()
        got = job.finish()
        stats = job.stats()
    _same(got, outs, "job, streamed")
    assert ctx.last_lines_in == lines
    assert stats["long_values"] == 16 and stats["files_windowed"] == 1, stats


def test_long_values_resident(ctx):
    """the one-lane escaper over 280 KB a value: slow by design, run once"""
    data = C.long_split()
    _same(ctx.map_partitions(PLAIN, data, 10), C.partitions("long", data, PLAIN, 10), "map_partitions")


# ---- 4. random values ------------------------------------------------------------------------------
def test_random_values_resident(ctx):
    data = C.random_split()
    _same(ctx.map_partitions(PLAIN, data, 10), C.partitions("random", data, PLAIN, 10), "map_partitions")


def test_random_values_batch(ctx):
    files = C.cut_files(C.random_split(), 5, b"random")
    got = ctx.map_partitions_batch(files, 10)
    for s, (fname, d) in enumerate(files):
        _same(got[s], C.partitions("random/%d" % s, d, fname, 10), "map_partitions_batch file %d" % s)


@pytest.mark.parametrize("lv", [256, 1 << 30])
@pytest.mark.parametrize("W", [8192, 65536])
def test_random_values_windowed(ctx, W, lv):
    data = C.random_split()
    want = C.partitions("random", data, PLAIN, 10)
    ctx.set_long_value(lv)
    _same(ctx.map_partitions_windowed(PLAIN, data, 10, W), want, "map_partitions_windowed W %d lv %d" % (W, lv))
    got, stats = _stream(ctx, "random", _fed(data), W, 10, lv)
    _same(got, want, "partition_stream W %d lv %d" % (W, lv))
    assert stats["long_values"] == C.chunked(C.values_of(data), lv), (W, lv, stats)


def test_regressions(ctx):
    """every value that ever failed, alone between two plain lines, through the three writers"""
    ctx.set_long_value(256)
    for name, value in C.REGRESSIONS:
        data = b"before\n" + value + b"\nafter"
        want = PC.whole_partitions(data, lambda line: True, PLAIN, 3)
        _same(ctx.map_partitions(PLAIN, data, 3), want, name)
        _same(ctx.map_partitions_batch([(PLAIN, data)], 3)[0], want, name)
        _same(ctx.map_partitions_windowed(PLAIN, data, 3, 4096), want, name)


# ---- 5. the tally ------------------------------------------------------------------------------------
def test_every_planted_class_was_reached(ctx):
    """What the inputs put before the device code, and how many values took
    each path. The classes are counted for every position of the split against
    the 16-byte blocks of the window buffer, since the carried tail moves it.
    A (split, long_value) whose stream no test of this run ran is run here."""
    splits = {"short": C.short_split(), "long": C.long_split(), "random": C.random_split()}
    for name, data in splits.items():
        plain, one_lane, chunked = C.paths(C.values_of(data))
        for lv, want in ((256, chunked), (1 << 30, 0)):
            if (name, lv) not in _seen:
                ctx.set_long_value(lv)
                _stream(ctx, name, _fed(data, 300007), 65536, 10, lv)
            assert _seen[(name, lv)] == want, (name, lv, _seen[(name, lv)], want)
        print("writer paths: %-6s %7d values: %6d plain, %6d escaped by one lane, %4d chunked at long_value 256"
              % (name, plain + one_lane + chunked, plain, one_lane, chunked))
    assert C.paths(C.values_of(splits["long"]))[2] == 16
    for shift in range(16):
        t = C.long_classes(shift)
        e = C.edge_classes(splits["long"], shift) + C.edge_classes(splits["random"], shift)
        if shift == 0:
            print("long values, per class (split at a block boundary):",
                  " ".join("%s=%d" % (k, t[k]) for k in C.LONG_CLASSES),
                  " ".join("%s=%d" % (k, e[k]) for k in C.EDGE_CLASSES), "distinct lane sums in a step >= %d" % t["sums"])
        assert all(t[k] > 0 for k in C.LONG_CLASSES) and t["sums"] >= 16, (shift, t)
        assert all(e[k] > 0 for k in C.EDGE_CLASSES), (shift, e)
