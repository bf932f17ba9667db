"""The batch partition writer's pipeline restated in numpy
(encode_batch_cases.emulate_cells: records of the packed buffer, rebased, stable
sort by split * nreduce + ihash(Key) % nreduce, cell offsets by binary search)
gives exactly the per-split files of the oracle (expected_cells). No GPU."""
import numpy as np
import pytest

import batch_cases as B
import encode_batch_cases as E

LISTS = {"fixed": B.FIXED_SPLITS, "random": B.random_splits(3, 300)}


@pytest.mark.parametrize("nreduce", [1, 7, 256])
@pytest.mark.parametrize("name", sorted(LISTS))
def test_emulated_cells_equal_per_split_files(name, nreduce):
    files = E.with_names(LISTS[name], E.FNAMES)
    for pattern in (b"error", b"", b"^$", b"k\\z"):
        raw, off = E.emulate_cells(pattern, files, nreduce)
        want_raw, want_off = E.expected_cells(pattern, files, nreduce)
        np.testing.assert_array_equal(off, want_off, err_msg="%s %r" % (name, pattern))
        assert raw == want_raw, (name, pattern)
        assert off[0] == 0 and int(off[-1]) == len(raw)
        if pattern != b"k\\z":
            assert len(raw) > 0
