"""The batch reduce and the whole-job call on the GPU (dgrep_reduce_batch,
dgrep_reduce_batch_device, dgrep_grep_job). Expected, byte for byte: per
partition go_json.reduce_reference of the partition's concatenated segments
(reduce_batch_cases.expected); for the job, reduce_reference over partitions
built from the oracle's Map, ihash and json.Encoder restatements, and the
existing map_partitions_batch + reduce path on the same GPU."""
import re

import numpy as np
import pytest

import encode_batch_cases as E
import go_json as G
import reduce_batch_cases as C

pytestmark = pytest.mark.gpu

C3 = b"^[0-9]{4}-[0-9]{2}.*(WARN|ERROR) [a-z_]+"
GOOD = C.good_cases()
BAD = C.bad_cases()
BY_NAME = {c.name: c for c in GOOD}
SENTINEL = 0xAB

_expected = {}


def _want(case):
    """computed once per case, shared, never changed"""
    if case.name not in _expected:
        _expected[case.name] = C.expected(case)
    return _expected[case.name]


def _on_device(case):
    import torch

    buf = np.frombuffer(case.data, np.uint8).copy() if case.data else np.zeros(1, np.uint8)
    return torch.from_numpy(buf).cuda()


def _device_call(ctx, case, d_data, out_cap, tail=4096):
    """dgrep_reduce_batch_device into a sentinel-filled buffer of out_cap + tail
    bytes: (part_off, lines_in, total, the whole buffer's bytes)"""
    import torch

    out = torch.full((out_cap + tail,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    off, lin, total = ctx.reduce_batch_device(d_data.data_ptr(), len(case.data), case.seg_off, case.nparts,
                                              out.data_ptr() if out_cap else 0, out_cap)
    return off, lin, total, out.cpu().numpy()


def _split(raw: bytes, off):
    return [raw[a:b] for a, b in zip(off, off[1:])]


# ---- 1. every case through both forms ----------------------------------------------
@pytest.mark.parametrize("case", GOOD, ids=[c.name for c in GOOD])
def test_host_form(gpu_ctx, case):
    want = _want(case)
    # R separate inputs: each partition's segments concatenated by the caller
    got = gpu_ctx.reduce_batch(C.partition_inputs(case))
    assert got == want.outputs
    assert gpu_ctx.last_lines_in == want.lines_in


@pytest.mark.parametrize("case", GOOD, ids=[c.name for c in GOOD])
def test_device_form(gpu_ctx, case):
    want = _want(case)
    d = _on_device(case)
    off, lin, total, _ = _device_call(gpu_ctx, case, d, 0)
    raw = b"".join(want.outputs)
    assert total == len(raw) and lin == want.lines_in
    assert _split(raw, off) == want.outputs
    off2, lin2, total2, buf = _device_call(gpu_ctx, case, d, total)
    assert (off2, lin2, total2) == (off, lin, total)
    assert buf[:total].tobytes() == raw
    assert (buf[total:] == SENTINEL).all()
    if len(case.data):
        assert gpu_ctx.last_reduce_ms() > 0


# ---- 2. the two rules that are new ---------------------------------------------------
def test_same_key_in_two_partitions_and_in_two_segments(gpu_ctx):
    case = BY_NAME["new-rules"]
    p0, p1 = gpu_ctx.reduce_batch(C.partition_inputs(case))
    d = _on_device(case)
    off, _, total, buf = _device_call(gpu_ctx, case, d, 4096)
    assert _split(buf[:total].tobytes(), off) == [p0, p1] == _want(case).outputs
    # the same decoded key in both partitions: kept in both, with each partition's first value
    assert p0.startswith(b"both p0\n") and p1.startswith(b"both p1\n")
    assert p0.count(b"both ") == 1 and p1.count(b"both ") == 1
    # the same key in two segments of partition 0, the second in another spelling: the first segment's value
    assert p0.count(b"first\n") == 1 and b"second spelling" not in p0
    assert p1.count(b"p1 spelled\n") == 1
    assert p0.endswith(b"new n\n")


# ---- 3. equality with the existing path -----------------------------------------------
@pytest.mark.parametrize("case", [c for c in GOOD if c.nparts <= 64], ids=[c.name for c in GOOD if c.nparts <= 64])
def test_equals_single_reduce(gpu_ctx, case):
    inputs = C.partition_inputs(case)
    got = gpu_ctx.reduce_batch(inputs)
    lines = list(gpu_ctx.last_lines_in)
    for p, data in enumerate(inputs):
        assert got[p] == gpu_ctx.reduce(data), (case.name, p)
        assert lines[p] == data.count(b"\n")


def test_sparse_partitions_equal_single_reduce(gpu_ctx):
    case = BY_NAME["nparts-65535"]
    inputs = C.partition_inputs(case)
    got = gpu_ctx.reduce_batch(inputs)
    for p in (0, 1, 2, 3, 40000, 65532, 65533, 65534):
        assert got[p] == gpu_ctx.reduce(inputs[p]), p


# ---- 4. malformed input ------------------------------------------------------------------
def _reported(err):
    m = re.search(r"partition (\d+): line (\d+)", str(err))
    assert m, str(err)
    return int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("case,agrees", BAD, ids=[c.name for c, _ in BAD])
def test_malformed_input_fails_the_call(gpu_ctx, case, agrees):
    import dgrep

    want = C.expected(case)
    p, line = want.bad
    if agrees:  # what reduce_reference gives for the lowest such partition
        assert G.reduce_reference(C.partition_inputs(case)[p]).bad_line == line
    good = BY_NAME["dealt-n3-k2"]
    d = _on_device(case)
    with pytest.raises(dgrep.DgrepError) as e:
        _device_call(gpu_ctx, case, d, 1 << 16)
    assert e.value.code == dgrep.DGREP_E_INVALID
    assert _reported(e.value) == (p, line)
    # the context is as good as before
    dg = _on_device(good)
    off, lin, total, buf = _device_call(gpu_ctx, good, dg, 1 << 16)
    assert _split(buf[:total].tobytes(), off) == _want(good).outputs and lin == _want(good).lines_in
    # the host form sees each partition's input as one segment
    inputs = C.partition_inputs(case)
    host = C.expected(C.from_segments(case.name + "-host", inputs, case.nparts))
    if host.bad is None:  # the unfinished line was fused on the host: nothing is left to report
        assert not agrees
        assert gpu_ctx.reduce_batch(inputs) == host.outputs
    else:
        with pytest.raises(dgrep.DgrepError) as e:
            gpu_ctx.reduce_batch(inputs)
        assert e.value.code == dgrep.DGREP_E_INVALID and _reported(e.value) == host.bad
    assert gpu_ctx.reduce_batch(C.partition_inputs(good)) == _want(good).outputs


def test_nothing_is_written_for_malformed_input(gpu_ctx):
    import dgrep

    case = BAD[0][0]
    d = _on_device(case)
    import torch

    out = torch.full((1 << 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(dgrep.DgrepError):
        gpu_ctx.reduce_batch_device(d.data_ptr(), len(case.data), case.seg_off, case.nparts, out.data_ptr(), 1 << 16)
    assert (out.cpu().numpy() == SENTINEL).all()


# ---- 5. the device form's capacity contract ---------------------------------------------
@pytest.mark.parametrize("name", ["dealt-n10-k3", "kept-63-64-65-then-ones", "phases-0-9", "block-edge+1"])
def test_device_form_capacity_contract(gpu_ctx, name):
    case = BY_NAME[name]
    want = _want(case)
    raw = b"".join(want.outputs)
    d = _on_device(case)
    fresh = _device_call(gpu_ctx, case, d, len(raw))
    assert fresh[3][:len(raw)].tobytes() == raw
    for cap in (0, 1, len(raw) - 1, len(raw), len(raw) + 64):
        off, lin, total, buf = _device_call(gpu_ctx, case, d, cap)
        assert total == len(raw), cap                       # exact whatever fits
        assert _split(raw, off) == want.outputs and lin == want.lines_in, cap
        assert (buf[cap:] == SENTINEL).all(), cap            # nothing at or past out_cap
        written = buf[:min(cap, total)]
        ok = (written == np.frombuffer(raw, np.uint8)[:len(written)]) | (written == SENTINEL)
        assert ok.all(), cap                                 # below it: the right byte or none
        if cap >= total:
            assert buf[:total].tobytes() == raw, cap
            assert (buf[total:] == SENTINEL).all(), cap
        else:  # a short call, then a full one: the same bytes as a fresh full call
            again = _device_call(gpu_ctx, case, d, len(raw))
            assert again[:3] == fresh[:3] and again[3][:len(raw)].tobytes() == raw, cap


# ---- 6. inputs above the direct-ingest path: the ring, pieces straddling inputs ----------
def test_host_form_through_the_staging_ring(gpu_ctx):
    inputs = []
    for p in range(3):
        lines = [C.plain_line(b"ring-%d (line number #%d)" % (i % 3, i % 30000), b"v" * (i % 10 + 20 * p))
                 for i in range(36000 + 1000 * p)]
        inputs.append(b"".join(lines))
    assert sum(map(len, inputs)) > (4 << 20) and all(len(x) % 4096 for x in inputs)
    want = [G.reduce_reference(x) for x in inputs]
    try:
        gpu_ctx.set_ingest(1 << 20, 3, 2)
        got = gpu_ctx.reduce_batch(inputs + [b""])
    finally:
        gpu_ctx.set_ingest(64 << 20, 4, 4)
    assert got == [w.output for w in want] + [b""]
    assert gpu_ctx.last_lines_in == [x.count(b"\n") for x in inputs] + [0]
    assert got[1] == gpu_ctx.reduce(inputs[1])


# ---- 7. the whole job ----------------------------------------------------------------------
def _job_files():
    import dgrep

    return [
        (b"split-0.log", dgrep.synth_corpus_host(3 << 20, 21, 0)),
        (b"split-1.log", dgrep.synth_corpus_host(5 << 20, 22, 1) + b"\nerror <&> \"q\" \xff\xe2\x80\xa8 tail"),
        ("ünï-2.log".encode(), b"error one\nnothing\nerror \x01\x7f\n\nerror"),
        (b"empty.log", b""),
        (b"no-match.log", b"nothing here\nnor here\n"),
        (b"twice.log", b"error A\nfine\nerror B\n"),
        (b"twice.log", b"error C\nerror D\nerror E\n"),   # the same name: duplicate keys across splits
    ]


@pytest.mark.parametrize("nreduce", [1, 5, 64])
def test_job_equals_map_partitions_batch_then_reduce(gpu_ctx, nreduce):
    files = _job_files()
    gpu_ctx.load(b"error")
    got = gpu_ctx.grep_job(files, nreduce)
    lines = list(gpu_ctx.last_lines_in)
    cells = gpu_ctx.map_partitions_batch(files, nreduce)
    assert len(got) == nreduce
    for r in range(nreduce):
        data = b"".join(cells[s][r] for s in range(len(files)))
        assert got[r] == gpu_ctx.reduce(data), r
        assert got[r] == G.reduce_reference(data).output, r
        assert lines[r] == data.count(b"\n")
    every = b"".join(got)
    # the two splits named twice.log share the keys of lines 1 and 2: the first split's value stays
    assert every.count(b"twice.log (line number #1) error A\n") == 1 and b"error C\n" not in every
    assert every.count(b"twice.log (line number #2) error D\n") == 1
    assert every.count(b"twice.log (line number #3) error B\n") == 1 and b"error E\n" not in every
    st = gpu_ctx.scan_stats()
    assert st["matches"] == sum(lines) > 0
    assert gpu_ctx.last_encode_ms() > 0 and gpu_ctx.last_reduce_ms() > 0


@pytest.mark.parametrize("pattern", [b"error", b"", C3], ids=["error", "match-all", "c3"])
def test_job_equals_the_oracle(gpu_ctx, pattern):
    import dgrep

    files = [(b"a.log", dgrep.synth_corpus_host(1 << 20, 31, 0)),
             (b"b<&>.log", dgrep.synth_corpus_host((1 << 20) + 4097, 32, 1) + b"\n\nerror last\n\n"),
             (b"a.log", dgrep.synth_corpus_host(1 << 20, 33, 0) + b"\n\n")]
    nreduce = 7
    gpu_ctx.load(pattern)
    got = gpu_ctx.grep_job(files, nreduce)
    parts = [E.expected_partitions(pattern, f, d, nreduce) for f, d in files]
    total = 0
    for r in range(nreduce):
        ref = G.reduce_reference(b"".join(p[r] for p in parts))
        assert ref.bad_line is None
        assert got[r] == ref.output, (pattern, r)
        total += len(ref.output)
    assert total > 0
    if pattern == b"":
        assert any(b") \n" in g for g in got)  # empty lines match and are kept


def test_job_with_nothing_to_write(gpu_ctx):
    import dgrep

    files = [(b"a", b"error\n"), (b"b", b""), (b"c", b"k")]
    gpu_ctx.load(b"zzz_never")
    assert gpu_ctx.grep_job(files, 4) == [b""] * 4
    assert gpu_ctx.last_lines_in == [0] * 4
    cp = gpu_ctx.load(b"[^\\x00-\\x{10FFFF}]")  # matches nothing
    assert cp.flags & dgrep.DFA_MATCH_NONE
    assert gpu_ctx.grep_job(files, 4) == [b""] * 4
    assert gpu_ctx.grep_job([], 4) == []
    gpu_ctx.load(b"error")
    assert gpu_ctx.grep_job(files, 4).count(b"a (line number #1) error\n") == 1


def test_module_level_grep_job(gpu_ctx):
    import dgrep

    files = [("x.log", "ok\nan error\n"), ("y.log", b"error \xff\nfine\nerror")]
    dgrep.set_pattern("error")
    gpu_ctx.load(b"error")
    assert dgrep.GrepJob(files, 3) == gpu_ctx.grep_job(files, 3)
    assert sorted(b"".join(dgrep.GrepJob(files, 3)).split(b"\n")) == sorted(
        [b"", b"x.log (line number #2) an error", b"y.log (line number #1) error \xef\xbf\xbd",
         b"y.log (line number #3) error"])
    assert dgrep.GrepJob([], 3) == []
