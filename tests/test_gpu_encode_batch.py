"""The batch partition writer on the GPU (dgrep_map_partitions_batch /
dgrep_encode_batch_device): every cell byte-exact against the oracle's files of
that split alone (encode_batch_cases.expected_cells: each split through the
oracle's Map, ihash and json.Encoder restatements, with its own filename)."""
import random

import numpy as np
import pytest

import batch_cases as B
import encode_batch_cases as E
from test_gpu_encode import SPECIAL

pytestmark = pytest.mark.gpu

C3 = b"^[0-9]{4}-[0-9]{2}.*(WARN|ERROR) [a-z_]+"
# test_gpu_encode's names and its two heads beyond the single form's 2 KiB LDS limit
NAMES8 = E.FNAMES + [b"f" * 2100, b"dir/" + b"<&>" * 700]

_expected = {}


def _want(name, pattern, files, nreduce):
    """the oracle's cells of a named file list: computed once, shared, never changed"""
    key = (name, bytes(pattern), nreduce)
    if key not in _expected:
        _expected[key] = E.expected_cells(pattern, files, nreduce)
    return _expected[key]


def _check_host(ctx, name, pattern, files, nreduce, load=True):
    if load:
        ctx.load(pattern)
    got = ctx.map_partitions_batch(files, nreduce)
    raw, off = _want(name, pattern, files, nreduce)
    want = E.split_cells(raw, off, len(files), nreduce)
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, pattern, nreduce, s, files[s][0][:40])
    return got


def _device_records(ctx, splits):
    """dgrep_scan_batch_device over the packed splits: (packed tensor, n_packed,
    lens, record tensors, count)"""
    import torch

    packed = np.frombuffer(B.pack(splits), np.uint8).copy()
    n_packed = len(packed)
    packed_t = torch.from_numpy(packed if n_packed else np.zeros(1, np.uint8)).cuda()
    lens = [len(s) for s in splits]
    cap = B.pack(splits).count(b"\n") + 1  # at most one record per line
    ln, st, le = (torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(3))
    sp = torch.empty(cap, dtype=torch.int32, device="cuda")
    count = ctx.scan_batch_device(packed_t.data_ptr(), n_packed, lens, ln.data_ptr(), st.data_ptr(), le.data_ptr(),
                                  sp.data_ptr(), 0, cap)
    assert count <= cap
    return packed_t, n_packed, lens, (ln, st, le, sp), count


def _encode_device(ctx, dev, names, nreduce, out_t, out_cap):
    packed_t, n_packed, lens, (ln, st, le, sp), count = dev
    return ctx.encode_batch_device(packed_t.data_ptr(), n_packed, lens, ln.data_ptr(), st.data_ptr(), le.data_ptr(),
                                   sp.data_ptr(), count, names, nreduce, out_t.data_ptr() if out_cap else 0, out_cap)


# ---- 1. the batch tests' fixed list, all eight kinds of filename -----------------
@pytest.mark.parametrize("nreduce", [1, 7, 10, 256])
def test_fixed_splits_every_name(gpu_ctx, nreduce):
    files = E.with_names(B.FIXED_SPLITS, NAMES8)
    for pattern in (b"error", b"", b"^$", b"zzz_never", b"k"):
        got = _check_host(gpu_ctx, "fixed", pattern, files, nreduce)
        # and the single form on the same GPU, split by split
        for s, (f, d) in enumerate(files):
            assert got[s] == gpu_ctx.map_partitions(f, d, nreduce), (pattern, nreduce, s)


# ---- 2. values that need escaping: in one split, and with a head per line --------
def test_special_values_one_split_and_one_split_per_line(gpu_ctx):
    one = [(b"special.log", SPECIAL)]
    per_line = [(b"%d-" % i + NAMES8[i % len(NAMES8)], line) for i, line in enumerate(SPECIAL.split(b"\n"))]
    assert len({f for f, _ in per_line}) == len(per_line)
    for pattern in (b"error", b"", b"^$"):
        for nreduce in (1, 7):
            _check_host(gpu_ctx, "special-one", pattern, one, nreduce)
            _check_host(gpu_ctx, "special-lines", pattern, per_line, nreduce, load=False)


# ---- 3. waves that span many files, waves inside one file, the seam between ------
def _phase_files():
    lines = [b"error", b"", b"error\xff\"<"] + [b"error" + b"x" * (k % 9) for k in range(3000)]
    small = []
    for j in range(200):  # dealt round-robin from the first 600 lines: 1-3 lines per split
        mine = lines[j:600:200][:1 + j % 3]
        small.append(b"\n".join(mine) + (b"\n" if j % 2 else b""))
    splits = small + [b"\n".join(lines[600:3000])]
    assert all(1 <= s.count(b"\n") + 1 <= 4 for s in small) and splits[-1].count(b"\n") + 1 == 2400
    return E.with_names(splits, [b"n" * j for j in range(8)])


def test_head_and_edge_phases(gpu_ctx):
    files = _phase_files()
    assert len(files) == 201
    got = _check_host(gpu_ctx, "phases", b"error|^$", files, 7)
    assert sum(len(c) for cells in got[:200] for c in cells) > 0 and sum(map(len, got[200])) > 2400 * 38


# ---- 4. many tiny splits: 50,000 cells, most of them empty ----------------------
def _tiny_files():
    splits = B.random_splits(11, 5000, max_pieces=6)
    for at in (1200, 3100):
        splits[at:at + 300] = [b""] * 300
    return [(b"split-%05d.log" % i, s) for i, s in enumerate(splits)]


def test_many_tiny_splits(gpu_ctx):
    files = _tiny_files()
    assert len(files) == 5000
    _check_host(gpu_ctx, "tiny", b"", files, 10)
    raw, off = _want("tiny", b"", files, 10)
    assert len(off) == 50001 and (np.diff(off.astype(np.int64)) == 0).mean() > 0.5


# ---- 5. the packed buffer's tail, device form -------------------------------------
@pytest.mark.parametrize("pad", [0, 1, 2])
def test_packed_tail_device_form(gpu_ctx, pad):
    import torch

    splits = [b"", b"x\nan error\n", b"k", b"", b"ok\nerror " + b"y" * pad + b"\nthe last line ends in error"]
    n_packed = sum(map(len, splits)) + len(splits) - 1
    assert n_packed % 4 == 1 + pad and n_packed % 16 != 0
    names = [b"t%d.log" % i for i in range(len(splits))]
    files = list(zip(names, splits))
    for pattern in (b"^$", b"error", b"error|^$"):
        gpu_ctx.load(pattern)
        dev = _device_records(gpu_ctx, splits)
        raw, off = _want("tail%d" % pad, pattern, files, 3)
        assert len(raw) > 0
        if pattern != b"error":
            assert off[1:4].max() > 0  # the empty first split holds a match
        cell_off, total = _encode_device(gpu_ctx, dev, names, 3, None, 0)
        assert (cell_off, total) == (off.tolist(), len(raw))
        out = torch.zeros(total, dtype=torch.uint8, device="cuda")
        cell_off, total2 = _encode_device(gpu_ctx, dev, names, 3, out, total)
        assert (cell_off, total2) == (off.tolist(), total)
        assert out.cpu().numpy().tobytes() == raw, pattern


# ---- 6. above the direct-ingest path: 6 MiB cut at arbitrary bytes -----------------
def test_synth_corpus_cut_anywhere(gpu_ctx):
    import dgrep

    corpus = dgrep.synth_corpus_host(6 << 20, 9, 1)
    rnd = random.Random(257)
    cuts = [0] + sorted(rnd.randrange(len(corpus) + 1) for _ in range(257)) + [len(corpus)]
    files = [(b"split-%05d.log" % i, corpus[a:b]) for i, (a, b) in enumerate(zip(cuts, cuts[1:]))]
    assert len(files) == 258 and sum(len(d) for _, d in files) + 257 > (4 << 20)
    got = _check_host(gpu_ctx, "synth6", C3, files, 10)
    assert sum(len(c) for cells in got for c in cells) > 100000


# ---- 7. the device form's capacity contract ----------------------------------------
def test_encode_batch_device_capacity_retry(gpu_ctx):
    import torch

    import dgrep

    corpus = dgrep.synth_corpus_host(1 << 20, 3, 0)
    splits = [corpus[i << 16:(i + 1) << 16] for i in range(16)]
    names = [b"split-%05d.log" % i for i in range(16)]
    files = list(zip(names, splits))
    gpu_ctx.load(b"error")
    dev = _device_records(gpu_ctx, splits)
    raw, off = _want("capacity", b"error", files, 10)
    small = torch.full((1000 + 4096,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    cell_off, total = _encode_device(gpu_ctx, dev, names, 10, small, 1000)
    assert total == len(raw) > 1000
    assert cell_off == off.tolist()                      # valid although nothing fits
    assert (small[1000:].cpu().numpy() == 0xAB).all()    # nothing at or past out_cap
    out = torch.empty(total, dtype=torch.uint8, device="cuda")
    cell_off, total2 = _encode_device(gpu_ctx, dev, names, 10, out, total)
    assert total2 == total and cell_off == off.tolist()
    assert out.cpu().numpy().tobytes() == raw
    assert gpu_ctx.last_encode_ms() > 0


# ---- 8. small cases -------------------------------------------------------------------
def test_one_split_no_match_and_nothing(gpu_ctx):
    data = b"x\nan error\n\nerror \xff<\nlast error"
    for pattern in (b"error", b"", b"^$"):
        gpu_ctx.load(pattern)
        # one split: every wave's lines share it, also with a head longer than the wave's LDS row
        for name in (b"one.log", b"", b"f" * 2100):
            got = gpu_ctx.map_partitions_batch([(name, data)], 10)
            assert got == [gpu_ctx.map_partitions(name, data, 10)] == [E.expected_partitions(pattern, name, data, 10)]
    import dgrep

    cp = gpu_ctx.load(b"[^\\x00-\\x{10FFFF}]")  # matches nothing
    assert cp.flags & dgrep.DFA_MATCH_NONE
    files = [(b"a", b"error\n"), (b"b", b""), (b"c", b"k")]
    assert gpu_ctx.map_partitions_batch(files, 4) == [[b""] * 4] * 3
    dev = _device_records(gpu_ctx, [d for _, d in files])
    assert dev[4] == 0
    assert _encode_device(gpu_ctx, dev, [f for f, _ in files], 4, None, 0) == ([0] * 13, 0)
    assert gpu_ctx.map_partitions_batch([], 10) == []
