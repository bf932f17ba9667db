"""Different keys that share their 64-bit hash, through dgrep_reduce and the
whole job on the GPU. Both dedupe kernels (reduce.hip dedupe_kernel,
reduce_batch.hip dedupe_batch_kernel) sort the lines by (FNV-1a 64 of the
decoded key, line) and let a line walk back over its equal-hash run; only such
keys make the walk's compare answer "different": the length check's continue,
the escaped compare's and the decoded compare's same = false, and the walk going
on past an unequal entry to an equal one further back. The keys come from
tests/golden/fnv64_collisions.json, the inputs from tests/fnv64_collisions.py
(verified on the CPU by tests/test_fnv64_collisions.py); the reference is
go_json.reduce_reference, for the job job_window_cases.expected_job. The batch
reduce's cases are reduce_batch_cases' collide-* (tests/test_gpu_reduce_batch.py).
A wrong verdict shows as a line missing from the output, or one too many."""
import pytest

import fnv64_collisions as F
import job_window_cases as J
from test_gpu_reduce_language import check

pytestmark = pytest.mark.gpu


def _ids(inputs):
    return [i.name for i in inputs]


def _check_all(ctx, inputs):
    for inp in inputs:
        try:
            check(ctx, inp.data, nkeys=inp.nkeys)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (inp.name, e)) from None


# ---- single reduce -------------------------------------------------------------------------
@pytest.mark.parametrize("inp", F.stay_apart(), ids=_ids(F.stay_apart()))
def test_equal_length_keys_stay_apart(gpu_ctx, inp):
    got = check(gpu_ctx, inp.data, nkeys=2)
    first = inp.data.split(b"\n")[:2]
    # each key with its first value, in input order
    assert got == b"".join(line[8:-2].replace(b'","Value":"', b" ") + b"\n" for line in first)


@pytest.mark.parametrize("inp", F.different_lengths(), ids=_ids(F.different_lengths()))
def test_different_lengths(gpu_ctx, inp):
    got = check(gpu_ctx, inp.data, nkeys=2)
    assert got.count(b"\n") == 2 and b" v0\n" in got


def test_walk_goes_past_the_unequal_entries(gpu_ctx):
    inputs = F.walk_past()
    assert len(inputs) == 3 * (24 + 4) + 7
    _check_all(gpu_ctx, inputs)


def test_respelled_collisions(gpu_ctx):
    _check_all(gpu_ctx, F.respelled())


@pytest.mark.parametrize("inp", F.long_keys(), ids=_ids(F.long_keys()))
def test_long_keys(gpu_ctx, inp):
    check(gpu_ctx, inp.data, nkeys=inp.nkeys)


def test_a_crowd(gpu_ctx):
    (inp,) = F.crowd()
    got = check(gpu_ctx, inp.data, nkeys=708)
    for k in F.FOUR + F.MIXED_FOUR:
        assert got.count(k + b" ") == 1 and k + b" " + k[:4] + b" 0\n" in got


# ---- the whole job: files named by colliding keys -----------------------------------------
@pytest.mark.parametrize("nreduce", [1, 2, 3])
@pytest.mark.parametrize("fam", ["pair", "four"])
def test_whole_job_with_colliding_file_names(gpu_ctx, fam, nreduce):
    """Every line number gives keys that collide across the files; on the
    `shared` lines they also fall into one partition (computed with the test's
    own ihash and asserted), elsewhere the batch kernel meets them in other
    partitions. Each name comes twice, so every key has a duplicate to find
    behind the other names' keys."""
    names = F.FAMILIES[fam]
    W = J.WINDOWS[0]
    gpu_ctx.load(b"error")
    for big in (None, names[1]):  # every file on the pack route; one on the window route
        files, shared = F.job_files(names, nreduce, big=big, big_bytes=W)
        assert len(shared) >= 3
        for n in shared:
            assert len({F.ihash(F.job_key(f, n)) % nreduce for f in names}) == 1
            assert len({F.fnv64(F.job_key(f, n)) for f in names}) == 1
        assert [len(d) > W for _, d in files].count(True) == (big is not None)
        want = J.expected_job(b"error", files, nreduce)
        kept = b"".join(want[0])
        for f in names:
            assert kept.count(F.job_key(f, shared[0]) + b" ") == 1
            assert F.job_key(f, shared[0]) + b" error 0.%d\n" % shared[0] in kept  # the first file's value
        assert (gpu_ctx.grep_job(files, nreduce), list(gpu_ctx.last_lines_in)) == want, big
        assert (gpu_ctx.grep_job_windowed(files, nreduce, W), list(gpu_ctx.last_lines_in)) == want, big
