"""The windowed whole job's contract on the CPU (job_window_cases.py): the
model that follows the planner -- packs, flushes, windows, the arena and its
segment table -- gives the resident job's outputs for every case, window,
route assignment and feed cut; every segment table is well formed; and the
cases reach every head and tail path of the arena's append kernel."""
import pytest

import job_window_cases as J

_want = {}


def _expected(case, W):
    """computed once per case (its files follow the window), shared, never changed"""
    if (case.name, W) not in _want:
        _want[case.name, W] = J.expected_job(case.pattern, case.files, case.nreduce)
    return _want[case.name, W]


def _check(case, W, routes, feeds):
    m = J.model_job(case.pattern, case.files, W, case.nreduce, routes, feeds)
    want = _expected(case, W)
    assert (m.outputs, m.lines_in) == want, (case.name, W, routes)
    seg = m.seg_off
    assert seg[0] == 0 and seg[-1] == len(m.arena) and seg == sorted(seg), (case.name, W, routes)
    assert (len(seg) - 1) % case.nreduce == 0 and len(seg) - 1 == m.rows * case.nreduce, (case.name, W, routes)
    assert m.files_packed + m.files_windowed == len(case.files)
    if m.arena_cap > J.ARENA_INITIAL:
        assert m.arena_cap < 2 * len(m.arena)
    return m


@pytest.mark.parametrize("W", J.CPU_WINDOWS)
def test_every_route_assignment_gives_the_resident_job(W):
    """every add / stream assignment the API allows, one random cut of every streamed file"""
    for case in J.cases(W):
        for routes in J.route_assignments(case):
            _check(case, W, routes, J.random_cuts(case))


@pytest.mark.parametrize("step", [1, 7, 4096])
@pytest.mark.parametrize("W", J.CPU_WINDOWS)
def test_feed_cuts(W, step):
    """feeds of `step` bytes: every file streamed, and add / stream alternating"""
    for case in J.cases(W):
        k = len(case.files)
        for routes in (("stream",) * k, J.mixed(case)):
            _check(case, W, routes, J.step_cuts(case, step))


@pytest.mark.parametrize("W", J.CPU_WINDOWS)
def test_the_planner_as_the_cases_need_it(W):
    by = {c.name: c for c in J.cases(W)}
    add = lambda c: ("add",) * len(c.files)
    m = _check(by["route_edge"], W, add(by["route_edge"]), J.whole(by["route_edge"]))
    assert (m.files_packed, m.files_windowed, m.packs) == (2, 1, 2)  # W and W - 1 are packed, each alone; W + 1 is not
    m = _check(by["pack_full"], W, add(by["pack_full"]), J.whole(by["pack_full"]))
    assert sum(len(d) for _, d in by["pack_full"].files[:2]) + 1 == W and m.packs == 2
    m = _check(by["pack_overflow"], W, add(by["pack_overflow"]), J.whole(by["pack_overflow"]))
    assert sum(len(d) for _, d in by["pack_overflow"].files[:2]) + 1 == W + 1 and m.packs == 2
    assert [rows for _, _, rows in m.appends] == [1, 2]  # a alone, then b with c
    m = _check(by["window_between_packs"], W, add(by["window_between_packs"]), J.whole(by["window_between_packs"]))
    assert (m.files_packed, m.files_windowed, m.packs) == (4, 1, 2)
    assert [rows for _, _, rows in m.appends][0] == 2 and [rows for _, _, rows in m.appends][-1] == 2
    m = _check(by["nreduce_1000"], W, add(by["nreduce_1000"]), J.whole(by["nreduce_1000"]))
    assert len(m.seg_off) - 1 > sum(m.lines_in)  # more segments than lines
    for name in ("no_match", "syntax_error"):
        m = _check(by[name], W, add(by[name]), J.whole(by[name]))
        assert m.arena == b"" and m.seg_off == [0] and m.outputs == [b""] * 10
    m = _check(by["growth"], W, ("add", "add", "stream"), J.whole(by["growth"]))
    assert m.growths >= 3 and m.appends[0][1] < 100
    m = _check(by["same_name"], W, add(by["same_name"]), J.whole(by["same_name"]))
    every = b"".join(m.outputs)
    assert every.count(b"twice.log (line number #1) error A\n") == 1 and b"error C" not in every
    assert b"twice.log (line number #3) error D\n" in every


def test_many_small_files_share_packs():
    case = J.many_small()
    m = _check(case, 65536, ("add",) * 64, J.whole(case))
    assert (m.packs, m.files_packed, m.files_windowed) == (2, 64, 0)  # 63 files and 62 separators fit; not 64 packs


@pytest.mark.parametrize("W", J.CPU_WINDOWS)
def test_the_names_case_reaches_every_residue(W):
    """every file streamed whole: one append per file; the arena offset before
    an append and the appended total each take every residue modulo 16, so the
    append kernel's head is 0..15 bytes long and so is its tail"""
    case = {c.name: c for c in J.cases(W)}["names"]
    m = _check(case, W, ("stream",) * len(case.files), J.whole(case))
    assert len(m.appends) == len(case.files)
    at, total = J.residues(m)
    assert at == set(range(16)) and total == set(range(16)), (sorted(at), sorted(total))
    # head and tail lengths of the kernel's split (job_plan.h job_copy_split)
    heads, tails = set(), set()
    for a, t, _ in m.appends:
        head = min((16 - a % 16) % 16, t)
        heads.add(head)
        tails.add((t - head) % 16)
    assert heads == set(range(16)) and tails >= set(range(1, 16)), (sorted(heads), sorted(tails))
    assert len(J.LONG_NAME) > 2048 and any(len(n) == 1 for n, _ in case.files)
