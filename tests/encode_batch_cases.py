"""Shared by the batch partition writer's tests (test_encode_batch_emulation.py
on the CPU, test_gpu_encode_batch.py on the GPU): what the cells of
dgrep_map_partitions_batch must hold, derived two ways from the oracle.

Cell (s, p) = the content of mr-<s>-<p>: the json.Encoder lines of split s's
KeyValues with ihash(Key) % nreduce == p (map_reduce/worker.go:78-109), Key =
Sprintf("%s (line number #%v)", filename[s], line) with the line counted within
split s. Cells are contiguous, split-major then partition: cell c = s * nreduce
+ p is bytes[cell_off[c] : cell_off[c + 1]).
"""
import numpy as np

import batch_cases as B
import oracle_lib as O

# the names of test_gpu_encode.FNAMES, restated
FNAMES = [b"log.txt", b"a<b>&\"q\\.log", "ünï€.log".encode(), b"bad\xff\xfe.log", b"",
          b"tab\there\n.log"]


def expected_partitions(pattern, filename, data, nreduce):
    """test_gpu_encode.expected_partitions, restated: one map task's files."""
    ln, st, le = O.grep_map(pattern, data, threads=16)
    parts = [bytearray() for _ in range(nreduce)]
    for a, b, c in zip(ln.tolist(), st.tolist(), le.tolist()):
        key = O.format_key(filename, a)
        parts[O.ihash(key) % nreduce] += O.json_kv(key, data[b:b + c])
    return [bytes(p) for p in parts]


def expected_cells(pattern, files, nreduce):
    """files = [(filename, contents)]: every split on its own through the
    oracle, flattened to (bytes, cell_off)."""
    cells = [p for f, d in files for p in expected_partitions(pattern, f, d, nreduce)]
    off = np.zeros(len(cells) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in cells], dtype=np.uint64)
    return b"".join(cells), off


def emulate_cells(pattern, files, nreduce):
    """The batch pipeline in numpy: the oracle's records over the packed buffer,
    rebased per split (batch_cases.rebase), stable-sorted by cell id, encoded in
    that order; cell_off by binary search of the sorted cell ids."""
    names = [f for f, _ in files]
    splits = [d for _, d in files]
    ln, st, le, sp, _ = (np.asarray(x).astype(np.int64) for x in B.rebase(splits, *O.grep_map(pattern, B.pack(splits))))
    keys = [O.format_key(names[s], n) for s, n in zip(sp.tolist(), ln.tolist())]
    cell = np.array([s * nreduce + O.ihash(k) % nreduce for s, k in zip(sp.tolist(), keys)], np.uint64)
    order = np.argsort(cell, kind="stable")
    lines = [O.json_kv(keys[r], splits[int(sp[r])][int(st[r]):int(st[r]) + int(le[r])]) for r in order.tolist()]
    pos = np.zeros(len(lines) + 1, np.uint64)
    pos[1:] = np.cumsum([len(x) for x in lines], dtype=np.uint64)
    first = np.searchsorted(cell[order], np.arange(len(files) * nreduce + 1, dtype=np.uint64), side="left")
    return b"".join(lines), pos[first]


def split_cells(raw, off, nsplits, nreduce):
    """(bytes, cell_off) -> [[cell bytes] * nreduce] * nsplits"""
    off = [int(x) for x in off]
    assert len(off) == nsplits * nreduce + 1
    return [[raw[off[s * nreduce + p]:off[s * nreduce + p + 1]] for p in range(nreduce)] for s in range(nsplits)]


def with_names(splits, names):
    """[(name, split)] with the names cycling"""
    return [(names[i % len(names)], s) for i, s in enumerate(splits)]
