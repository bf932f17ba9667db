"""The argument dgrep_scan_batch rests on, on the CPU: the oracle's Map over
the packed buffer, rebased with newline counts taken by numpy
(batch_cases.rebase), equals the per-split oracle results -- for splits that
are empty, end with or without '\\n', come in runs of empty ones or cut a UTF-8
sequence, and for patterns anchored to the text (\\A, \\z), the line and word
boundaries."""
import pytest

import batch_cases as B
import test_gpu_parity

PATTERNS = test_gpu_parity.PATTERNS + [b"\\Aerror", b"k\\z", b"(?m)^k$", b"\\Bk"]

RANDOM_SPLITS = B.random_splits(20240, 300)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_packed_oracle_rebased_equals_per_split_oracle(pattern):
    for name, splits in (("fixed", B.FIXED_SPLITS), ("random", RANDOM_SPLITS),
                         ("fixed+random", B.FIXED_SPLITS + RANDOM_SPLITS[:50] + B.FIXED_SPLITS[::-1])):
        B.assert_same(B.emulate(pattern, splits), B.expected(pattern, splits), "%r %s" % (pattern, name))


@pytest.mark.parametrize("splits", [[b""], [b"", b""], [b"\n"], [b"k"], [b"k", b""], [b"", b"k"], [b"k\n", b"\nk"]])
def test_smallest_batches(splits):
    for pattern in (b"", b"^$", b"k", b"k\\z"):
        B.assert_same(B.emulate(pattern, splits), B.expected(pattern, splits), "%r %r" % (pattern, splits))


def test_begin_closes_the_last_region():
    b = B.begins([b"ab", b"", b"c"])
    assert b.tolist() == [0, 3, 4, 6] and len(B.pack([b"ab", b"", b"c"])) + 1 == 6
