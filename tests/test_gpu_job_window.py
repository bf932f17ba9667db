"""The windowed whole job on the GPU (dgrep_job_*, dgrep_grep_job_windowed,
GrepJobWindowed). Every job is compared byte for byte, lines_in included, with
two references: job_window_cases.expected_job (the reduce reference over
partitions from the oracle's Map) and Context.grep_job on the same GPU -- the
resident job, which this feature leaves as it is. The job's stats are compared
with job_window_cases.model_job, which follows the planner: routes, packs,
rows, segments, arena bytes and the arena's growth."""
import ctypes

import pytest

import job_window_cases as J
import window_cases as WC

pytestmark = pytest.mark.gpu

C3 = b"^[0-9]{4}-[0-9]{2}.*(WARN|ERROR) [a-z_]+"
CASES = {W: {c.name: c for c in J.cases(W)} for W in J.WINDOWS}
NAMES = list(CASES[J.WINDOWS[0]])
MODES = ("add", "stream_1", "stream_7", "stream_4096", "stream_random", "mixed")

_ref = {}


def _want(ctx, case, W):
    """(outputs, lines_in) of the case: the oracle's, checked once against the
    resident job on this GPU; computed once, shared, never changed. The
    case's pattern must be loaded."""
    if (case.name, W) not in _ref:
        want = J.expected_job(case.pattern, case.files, case.nreduce)
        got = ctx.grep_job(case.files, case.nreduce)
        assert (got, list(ctx.last_lines_in)) == want, (case.name, W)
        _ref[case.name, W] = want
    return _ref[case.name, W]


def _plan(case, mode):
    k = len(case.files)
    if mode == "add":
        return ("add",) * k, J.whole(case)
    if mode == "mixed":
        return J.mixed(case), J.random_cuts(case)
    if mode == "stream_random":
        return ("stream",) * k, J.random_cuts(case)
    return ("stream",) * k, J.step_cuts(case, int(mode.split("_")[1]))


def _run(ctx, case, W, routes, feeds):
    """the job object: (outputs, lines_in, stats)"""
    with ctx.job(W, case.nreduce) as job:
        for (name, data), route, cuts in zip(case.files, routes, feeds):
            if route == "add":
                job.add(name, data)
                continue
            job.begin(name)
            for piece in WC.pieces_of(data, cuts):
                job.feed(piece)
            job.end()
        out = job.finish()
        return out, list(ctx.last_lines_in), job.stats()


def _check(ctx, case, W, routes, feeds):
    ctx.load(case.pattern)
    want = _want(ctx, case, W)
    out, lines, st = _run(ctx, case, W, routes, feeds)
    assert (out, lines) == want, (case.name, W, routes)
    m = J.model_job(case.pattern, case.files, W, case.nreduce, routes, feeds)
    assert (m.outputs, m.lines_in) == want
    assert st["files"] == len(case.files)
    assert (st["files_packed"], st["files_windowed"], st["packs"]) == (m.files_packed, m.files_windowed, m.packs), st
    assert st["segments"] == len(m.seg_off) - 1 and st["rows"] == m.rows, st
    assert st["arena_bytes"] == len(m.arena), st
    assert (st["arena_device_bytes"], st["arena_growths"]) == (m.arena_cap, m.growths), st
    if st["arena_device_bytes"] > J.ARENA_INITIAL:
        assert st["arena_device_bytes"] < 2 * st["arena_bytes"], st
    assert ctx.scan_stats()["matches"] == sum(want[1])  # the job's sum over its packs and windows
    return m, st


# ---- 1. every case, every route and feed cut ---------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("W", J.WINDOWS)
def test_every_case(gpu_ctx, W, name, mode):
    case = CASES[W][name]
    routes, feeds = _plan(case, mode)
    m, st = _check(gpu_ctx, case, W, routes, feeds)
    if name == "names" and mode == "stream_random":
        # every head and tail length of the append kernel: the model's offsets are the job's (arena_bytes above)
        at, total = J.residues(m)
        assert at == set(range(16)) and total == set(range(16))
    if name == "long_value" and mode != "add":
        assert st["long_values"] >= 2, st  # the two escaped lines of the windowed file took the chunked path
    if name == "long_line" and mode == "add":
        assert st["window_device_bytes"] > 2 * W  # the carried tail grew the buffers


# ---- 2. every stepper; a pattern over the compiler's budget -------------------------
@pytest.mark.parametrize("force", ["auto", "table", "pair", "filter"])
def test_every_stepper(gpu_ctx, force):
    W = 4096
    case = CASES[W]["window_between_packs"]
    try:
        gpu_ctx.set_stepper(force)
        _check(gpu_ctx, case, W, J.mixed(case), J.random_cuts(case))
        _check(gpu_ctx, case, W, ("add",) * len(case.files), J.whole(case))
        if force != "auto":
            assert gpu_ctx.scan_stats()["stepper"] == force
    finally:
        gpu_ctx.set_stepper("auto")
        gpu_ctx.load(b"error")


def test_partial_pattern(gpu_ctx):
    import dgrep

    data = dgrep.synth_corpus_host(60 * 1000, 21, 0)
    files = [(b"a.log", data[:3000]), (b"big.log", data[3000:40000]), (b"c.log", data[40000:45000]),
             (b"d.log", data[45000:])]
    case = J.Case("c3_partial", C3, files, 10)
    cp = gpu_ctx.load(dgrep.CompiledPattern(C3, state_budget=16))
    assert cp.partial
    want = J.expected_job(C3, files, 10)
    assert sum(want[1]) > 0
    assert (gpu_ctx.grep_job(files, 10), list(gpu_ctx.last_lines_in)) == want
    for routes in (("add",) * 4, J.mixed(case), ("stream",) * 4):
        out, lines, st = _run(gpu_ctx, case, 8192, routes, J.random_cuts(case))
        assert (out, lines) == want, routes
        assert st["files_windowed"] >= 2 and gpu_ctx.scan_stats()["stepper"] == "filter"
    gpu_ctx.load(b"error")


# ---- 3. stats against the existing stream and the model ------------------------------
@pytest.mark.parametrize("name", ["long_line", "window_between_packs"])
@pytest.mark.parametrize("W", J.WINDOWS)
def test_window_buffers_are_a_partition_streams(gpu_ctx, W, name):
    """window_device_bytes = what a PartitionStream of the same window reports
    after the job's largest windowed file alone (here its only one)."""
    case = CASES[W][name]
    _, st = _check(gpu_ctx, case, W, ("add",) * len(case.files), J.whole(case))
    windowed = [(n, d) for n, d in case.files if len(d) > W]
    assert len(windowed) == 1 and st["files_windowed"] == 1
    fname, data = windowed[0]
    with gpu_ctx.partition_stream(W, fname, case.nreduce) as ps:
        ps.feed(data)
        ps.finish()
        assert st["window_device_bytes"] == ps.stats()["data_bytes"], (st, ps.stats())


@pytest.mark.parametrize("W", J.WINDOWS)
def test_arena_growth_between_the_windows_of_one_file(gpu_ctx, W):
    """small first appends, then one file fed in one piece whose windows grow the
    arena several times: the contents survive every growth (the outputs are the
    resident job's) and the arena stays below twice what is used"""
    case = CASES[W]["growth"]
    m, st = _check(gpu_ctx, case, W, ("add", "add", "stream"), J.whole(case))
    assert m.appends[0][1] < 100 and st["arena_growths"] >= 3, st
    assert st["arena_device_bytes"] < 2 * st["arena_bytes"], st
    assert st["windows"] >= 6 and st["rows"] >= 7, st


def test_many_small_files_share_packs(gpu_ctx):
    case = J.many_small()
    m, st = _check(gpu_ctx, case, 65536, ("add",) * 64, J.whole(case))
    assert (st["packs"], st["files_packed"], st["files_windowed"]) == (2, 64, 0) and m.packs == 2, st
    assert st["rows"] == 64 and st["windows"] == 0, st


def test_times_are_summed_over_the_job(gpu_ctx):
    W = 4096
    case = CASES[W]["window_between_packs"]
    _, st = _check(gpu_ctx, case, W, ("add",) * len(case.files), J.whole(case))
    assert st["scan_ms"] > 0 and st["encode_ms"] > 0 and st["append_ms"] > 0 and st["reduce_ms"] > 0, st
    assert gpu_ctx.last_kernel_ms() == pytest.approx(st["scan_ms"], rel=1e-5)
    assert gpu_ctx.last_encode_ms() == pytest.approx(st["encode_ms"], rel=1e-5)
    assert gpu_ctx.last_reduce_ms() == pytest.approx(st["reduce_ms"], rel=1e-5)


# ---- 4. the one-shot forms ------------------------------------------------------------
@pytest.mark.parametrize("W", J.WINDOWS)
def test_one_shot_forms_equal_the_job_object(gpu_ctx, W):
    import dgrep

    case = CASES[W]["window_between_packs"]
    gpu_ctx.load(case.pattern)
    want = _want(gpu_ctx, case, W)
    out, lines, _ = _run(gpu_ctx, case, W, ("add",) * len(case.files), J.whole(case))
    assert (out, lines) == want
    assert gpu_ctx.grep_job_windowed(case.files, case.nreduce, W) == out
    assert list(gpu_ctx.last_lines_in) == lines
    assert gpu_ctx.grep_job_windowed([], 3, W) == []
    dgrep.set_pattern("error")
    pieces = lambda d: iter(WC.pieces_of(d, WC.random_cuts("one shot", len(d), 4)))
    files = [(n, d if i & 1 else pieces(d)) for i, (n, d) in enumerate(case.files)]
    assert dgrep.GrepJobWindowed(files, case.nreduce, W) == out
    assert dgrep.GrepJobWindowed([("x.log", "ok\nan error\n"), ("y.log", [b"err", b"or \xff\nfine"])], 3, W) == \
        gpu_ctx.grep_job([("x.log", "ok\nan error\n"), ("y.log", b"error \xff\nfine")], 3)


def test_no_file_no_match_and_match_none(gpu_ctx):
    import dgrep

    files = [(b"a", b"error\n"), (b"b", b""), (b"c", b"k" * 5000)]
    gpu_ctx.load(b"error")
    with gpu_ctx.job(4096, 4) as job:  # no file at all
        assert job.finish() == [b""] * 4 and gpu_ctx.last_lines_in == [0] * 4
        assert job.stats()["files"] == 0
    for pattern in (b"zzz_never", b"[^\\x00-\\x{10FFFF}]", b"("):
        cp = gpu_ctx.load(pattern)
        case = J.Case("none", pattern, files, 4)
        out, lines, st = _run(gpu_ctx, case, 4096, ("add", "stream", "add"), J.whole(case))
        assert out == [b""] * 4 and lines == [0] * 4, pattern
        assert st["files"] == 3 and st["arena_bytes"] == 0 and st["segments"] == 0, st
        if cp.flags & dgrep.DFA_MATCH_NONE:
            assert st["windows"] == 0 and st["window_device_bytes"] == 0  # nothing was copied or scanned
            assert gpu_ctx.scan_stats()["tiles"] == 0
    gpu_ctx.load(b"error")


# ---- 5. states and errors ---------------------------------------------------------------
def test_call_order_is_checked_and_finish_is_final(gpu_ctx):
    import dgrep

    L, h = dgrep.lib(), gpu_ctx._h
    gpu_ctx.load(b"error")
    data = ctypes.create_string_buffer(b"an error\nok\n", 12)
    INV = dgrep.DGREP_E_INVALID

    def finish(j):
        r = dgrep._ReduceBatchOut()
        ctypes.memset(ctypes.byref(r), 0xAB, ctypes.sizeof(r))
        rc = L.dgrep_job_finish(j, ctypes.byref(r))
        if rc != dgrep.DGREP_OK:
            assert bytes(r) == bytes(ctypes.sizeof(r))  # zeroed
        return rc, r

    j = ctypes.c_void_p()
    assert L.dgrep_job_open(h, 4096, 3, ctypes.byref(j)) == dgrep.DGREP_OK
    try:
        assert L.dgrep_job_file_feed(j, data, 12) == INV and b"without dgrep_job_file_begin" in L.dgrep_last_error(h)
        assert L.dgrep_job_file_end(j) == INV and b"without dgrep_job_file_begin" in L.dgrep_last_error(h)
        assert L.dgrep_job_add(j, None, 12, b"f", 1) == INV  # n without data
        assert L.dgrep_job_add(j, data, 12, None, 1) == INV  # fn without filename
        assert L.dgrep_job_file_begin(j, None, 1) == INV
        assert L.dgrep_job_file_begin(j, b"f", 1) == dgrep.DGREP_OK
        assert L.dgrep_job_file_feed(j, None, 12) == INV
        assert L.dgrep_job_add(j, data, 12, b"g", 1) == INV and b"inside a file" in L.dgrep_last_error(h)
        assert L.dgrep_job_file_begin(j, b"g", 1) == INV and b"inside a file" in L.dgrep_last_error(h)
        assert finish(j)[0] == INV and b"inside a file" in L.dgrep_last_error(h)
        assert L.dgrep_job_file_feed(j, data, 12) == dgrep.DGREP_OK  # none of the refusals was sticky
        assert L.dgrep_job_file_end(j) == dgrep.DGREP_OK
        assert L.dgrep_job_add(j, data, 12, b"g", 1) == dgrep.DGREP_OK
        # the sized getter never writes past out_size, and zeroes a longer caller struct's tail
        buf = (ctypes.c_uint8 * 256)(*([0xAB] * 256))
        assert L.dgrep_job_stats_get(j, ctypes.cast(buf, ctypes.POINTER(dgrep._JobStats)), 0) == INV
        assert L.dgrep_job_stats_get(j, ctypes.cast(buf, ctypes.POINTER(dgrep._JobStats)), 8) == dgrep.DGREP_OK
        assert int.from_bytes(bytes(buf[:8]), "little") == 2 and bytes(buf[8:]) == b"\xab" * 248
        size = ctypes.sizeof(dgrep._JobStats)
        assert L.dgrep_job_stats_get(j, ctypes.cast(buf, ctypes.POINTER(dgrep._JobStats)), size + 40) == dgrep.DGREP_OK
        assert bytes(buf[size:size + 40]) == bytes(40) and bytes(buf[size + 40:]) == b"\xab" * (256 - size - 40)
        rc, r = finish(j)
        assert rc == dgrep.DGREP_OK and r.nparts == 3
        got = gpu_ctx._reduce_batch_parts(r)
        assert got == gpu_ctx.grep_job([(b"f", b"an error\nok\n"), (b"g", b"an error\nok\n")], 3)
        # any call after finish
        assert L.dgrep_job_add(j, data, 12, b"h", 1) == INV and b"after dgrep_job_finish" in L.dgrep_last_error(h)
        assert L.dgrep_job_file_begin(j, b"h", 1) == INV
        assert L.dgrep_job_file_feed(j, data, 12) == INV
        assert L.dgrep_job_file_end(j) == INV
        assert finish(j)[0] == INV and b"after dgrep_job_finish" in L.dgrep_last_error(h)
    finally:
        L.dgrep_job_close(j)


def test_a_load_mid_job_is_refused(gpu_ctx):
    import dgrep

    gpu_ctx.load(b"error")
    job = gpu_ctx.job(4096, 3)
    try:
        job.add(b"f", b"an error\n")
        gpu_ctx.load(b"ok")
        for call in (lambda: job.add(b"g", b"ok\n"), lambda: job.begin(b"g"), job.finish):
            with pytest.raises(dgrep.DgrepError) as e:
                call()
            assert e.value.code == dgrep.DGREP_E_INVALID and "pattern was loaded" in str(e.value)
    finally:
        job.close()
    gpu_ctx.load(b"error")
    assert gpu_ctx.grep_job_windowed([(b"f", b"an error\n")], 3, 4096) == gpu_ctx.grep_job([(b"f", b"an error\n")], 3)
