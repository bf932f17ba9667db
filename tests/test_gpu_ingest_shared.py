"""The one staging-ring ingest (csrc/runtime/ingest.h) behind every host entry
point, and the close path of self-freeing buffers (csrc/runtime/device_buf.h).
One fresh Context for the module, pattern `error`, synthetic corpora with a
'\\n' forced at each staging-piece edge. Every result is the oracle's: Map for
the scans (oracle_lib, batch_cases), the reduce reference for the reduces
(go_json, job_window_cases)."""
import numpy as np
import pytest

import batch_cases as B
import go_json as G
import job_window_cases as J
import oracle_lib as O
import reduce_batch_cases as C

pytestmark = pytest.mark.gpu

PATTERN = b"error"
MiB = 1 << 20
SIZES = (4 * MiB - 1, 4 * MiB, 4 * MiB + 1)  # the direct path's last size; four pieces; five, the last of 1 byte


@pytest.fixture(scope="module")
def ctx():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import dgrep

    c = dgrep.Context(0)
    c.load(PATTERN)
    yield c
    c.close()


_corpora = {}


def _corpus(n, seed, piece=MiB):
    """n synthetic bytes with a '\\n' as the last byte of every staging piece; made once, never changed"""
    import dgrep

    if (n, seed, piece) not in _corpora:
        buf = bytearray(dgrep.synth_corpus_host(n, seed, 0))
        for edge in range(piece, n + 1, piece):
            buf[edge - 1] = 10
        _corpora[n, seed, piece] = bytes(buf)
    return _corpora[n, seed, piece]


_maps = {}


def _check_scan(got, data):
    if data not in _maps:
        _maps[data] = O.grep_map(PATTERN, data)
    want = _maps[data]
    assert len(got[0]) == len(want[0]) > 0
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def _check_batch(c, splits):
    B.assert_same(c.scan_batch(splits), B.expected(PATTERN, splits), "%d splits" % len(splits))


def _two_splits(size):
    """two splits whose packed buffer (one separator between them) has `size` bytes"""
    data = _corpus(size, 31)
    cut = 3 * MiB // 2 + 7
    return [data[:cut], data[cut + 1:]]


def _reduce_inputs(size):
    """two reduce inputs of whole KeyValue lines, `size` bytes together"""
    first = b"".join(C.plain_line(b"ring-%d (line number #%d)" % (i % 3, i % 30000), b"v" * (i % 10))
                     for i in range(36000))
    lines, left = [], size - len(first)
    empty = len(C.plain_line(b"k", b""))
    i = 0
    while left:
        v = min(left - empty, 40 + i % 10)
        if 0 < left - empty - v < empty:  # the line after this one would be shorter than an empty value's
            v -= empty
        assert v >= 0
        lines.append(C.plain_line(b"k", b"w" * v))
        left -= len(lines[-1])
        i += 1
    out = [first, b"".join(lines)]
    assert sum(map(len, out)) == size and len(first) % 4096 and len(first) < size
    return out


# ---- 1. the direct-path threshold and a 1-byte last piece -------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_threshold_and_last_piece(ctx, size):
    ring = size >= 4 * MiB
    try:
        ctx.set_ingest(MiB, 2, 2)  # above the threshold every staging buffer is reused
        data = _corpus(SIZES[-1], 30)[:size]
        _check_scan(ctx.scan(data), data)
        assert (ctx.last_ingest_ms() > 0) == ring
        _check_batch(ctx, _two_splits(size))
        assert (ctx.last_ingest_ms() > 0) == ring
        inputs = _reduce_inputs(size)
        got = ctx.reduce_batch(inputs)
        assert (ctx.last_ingest_ms() > 0) == ring
        assert got == [G.reduce_reference(x).output for x in inputs]
        assert ctx.last_lines_in == [x.count(b"\n") for x in inputs]
    finally:
        ctx.set_ingest(64 * MiB, 4, 4)


# ---- 2. one ring under every entry point, its shape changed in between ------------------
def test_one_ring_every_entry_point(ctx):
    first = _corpus(5 * MiB, 32)
    W = J.WINDOWS[0]
    case = {c.name: c for c in J.cases(W)}["window_between_packs"]
    files = [f for f in case.files if f[0] in (b"s1", b"big")]  # one for the pack route, one for the window route
    assert len(files) == 2 and len(files[0][1]) < W < len(files[1][1]) and case.pattern == PATTERN
    try:
        ctx.set_ingest(MiB, 2, 2)
        _check_scan(ctx.scan(first), first)
        assert ctx.last_ingest_ms() > 0
        ctx.set_ingest(MiB + 4097, 3, 1)  # the ring is reallocated: its DMAs are complete
        piece = MiB + 4097
        data = _corpus(5 * MiB, 33, piece)
        _check_batch(ctx, [data[:piece - 1], data[piece:3 * piece + 11], data[3 * piece + 12:]])
        assert ctx.last_ingest_ms() > 0
        ctx.set_ingest(MiB, 2, 2)  # and again, for the window feed
        wide = _corpus(9 * MiB, 34)
        _check_scan(ctx.scan_windowed(wide, 4 * MiB), wide)
        got = ctx.grep_job_windowed(files, case.nreduce, W)
        assert (got, list(ctx.last_lines_in)) == J.expected_job(PATTERN, files, case.nreduce)
        _check_scan(ctx.scan(first), first)
    finally:
        ctx.set_ingest(64 * MiB, 4, 4)


# ---- 3. close with everything allocated ------------------------------------------------
@pytest.mark.parametrize("job_first", [True, False], ids=["job_streams_context", "streams_job_context"])
def test_close_with_everything_allocated(job_first):
    """A context whose value stream, bounded stream, partition stream and job
    have all been fed one window-sized piece is closed, objects first in either
    order, then the context. A second context then scans correctly: the close
    path neither faulted nor took anything another context needs."""
    import dgrep

    W = 64 << 10
    data = _corpus(MiB, 35)
    piece = data[:W]
    c = dgrep.Context(0)
    c.load(PATTERN)
    values = c.stream(W, values=True)
    bounded = c.stream(W, bounded=True)
    parts = c.partition_stream(W, b"close.log", 10)
    job = c.job(W, 10)
    want = O.grep_map(PATTERN, piece[:piece.rindex(b"\n")])  # the lines the one window completes
    got = values.feed(piece)
    assert len(got[0]) == len(want[0]) > 0 and got[3] == [piece[int(s):int(s + n)] for s, n in zip(want[1], want[2])]
    np.testing.assert_array_equal(bounded.feed(piece)[0], want[0])
    assert sum(len(cell) for row in parts.feed(piece) for cell in row) > 0
    job.add(b"small.log", data[:1000])
    job.begin(b"fed.log")
    job.feed(piece)
    streams = [values, bounded, parts]
    for obj in ([job] + streams if job_first else streams + [job]):
        obj.close()
    c.close()
    c2 = dgrep.Context(0)
    try:
        c2.load(PATTERN)
        _check_scan(c2.scan(data), data)
    finally:
        c2.close()
