"""Shared by the batch tests (test_batch_emulation.py on the CPU,
test_gpu_batch.py on the GPU): the split lists, the packing and rebasing that
dgrep_scan_batch rests on restated in numpy, and the per-split expectation.

Packing: P = s_0 '\\n' s_1 '\\n' ... '\\n' s_{k-1}. strings.Split(P, "\\n") is the
concatenation of the splits' own line lists, so the oracle's Map over P holds
every split's matching lines in order, with P-wide line numbers and starts;
begin[i] = sum_{j<i} (len_j + 1) and the '\\n' count before begin[i] rebase them.
"""
import random

import numpy as np

import oracle_lib as O

# empty splits, "\n", an unterminated split, a trailing '\n', runs of empty
# splits, and a UTF-8 sequence cut by a split boundary (\xe2\x82 | \xac)
FIXED_SPLITS = [
    b"", b"\n", b"error", b"error\n", b"", b"", b"", b"x\nerror", b"\nerror\n\n", b"key\nk\n", b"k",
    b"an error here\nok\nkey k", b"\n\n", b"", b"2024-01-02 WARN retry_later\n2024-05-01 ERROR disk_full",
    b"abc \xe2\x82", b"\xac def\n", b"\xe2\x82\xac\n\xff\xfe\n", b"", b"", b"k\n", b"\n", b"", b"kk\nK\nk",
    b"a" * 5000 + b"error" + b"b" * 5000 + b"\nerror", b"timeout while waiting for lock\n", b"",
]

# the alphabet of test_gpu_parity.test_random_small
ALPHABET = [b"a", b"e", b"r", b"o", b"x", b"k", b"K", b" ", b"_", b"1", b"-", b"\n", b"\n", b"\r", b"\xe2\x82\xac",
            b"\xe2\x82", b"\xff", b"\xc5\xbf", b"WARN", b"ERROR", b"error", b"2024-01", b"key "]


def random_splits(seed, count, max_pieces=40, alphabet=ALPHABET):
    rnd = random.Random(seed)
    return [b"".join(rnd.choice(alphabet) for _ in range(rnd.randrange(max_pieces + 1))) for _ in range(count)]


def pack(splits):
    return b"\n".join(splits)


def begins(splits):
    """begin[0..k]: split i's first byte in the packed buffer; begin[k] = n_packed + 1."""
    b = np.zeros(len(splits) + 1, np.uint64)
    b[1:] = np.cumsum([len(s) + 1 for s in splits], dtype=np.uint64)
    return b


def rebase(splits, ln, st, le):
    """The packed buffer's records (ln, st, le) -> (line_no, start, len, split,
    split_begin) per split, as the batch kernels compute them."""
    k = len(splits)
    packed = np.frombuffer(pack(splits), np.uint8)
    begin = begins(splits)
    nl_before = np.concatenate([[0], np.cumsum(packed == 10, dtype=np.uint64)])  # '\n' in P[0 : i)
    lines_before = nl_before[begin[:k].astype(np.int64)]                         # first_line - 1
    split = (np.searchsorted(begin[:k], st, side="right") - 1).astype(np.int64)
    split_begin = np.concatenate([np.searchsorted(st, begin[:k], side="left"), [len(st)]]).astype(np.uint64)
    return (ln - lines_before[split], st - begin[:k][split], le.copy(), split.astype(np.uint32), split_begin)


def emulate(pattern, splits):
    return rebase(splits, *O.grep_map(pattern, pack(splits)))


def expected(pattern, splits):
    """[Map(split) for split in splits] from the oracle, in the batch layout."""
    per = [O.grep_map(pattern, s) for s in splits]
    counts = [len(p[0]) for p in per]
    cat = lambda j: np.concatenate([p[j] for p in per]) if per else np.zeros(0, np.uint64)
    split = np.repeat(np.arange(len(splits), dtype=np.uint32), counts)
    split_begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return cat(0), cat(1), cat(2), split, split_begin


def assert_same(got, want, what=""):
    names = ("line_no", "start", "len", "split", "split_begin")
    for name, g, w in zip(names, got, want):
        assert len(g) == len(w), (what, name, len(g), len(w))
        np.testing.assert_array_equal(np.asarray(g, dtype=np.uint64), np.asarray(w, dtype=np.uint64),
                                      err_msg="%s %s" % (what, name))
