"""Every scan-kernel instantiation dgrep_load_dfa can pick, at the DFA sizes
where its choice changes (tests/stepper_cells.py: Sheng, the four pair
builds, the five table builds with one and two chunks per lane, filter),
against the CPU oracle on inputs built for the shapes a stepper can get wrong:
an event at every byte of a load block, several '\\n' in one word, chunk,
stream and tile edges, more matching lines than a lane's slots, lines longer
than several chunks, and the split's last line.

Each case is compared bit-exactly with the oracle; scan_stats must report the
cell's stepper, the lane chunk the input was built for and the tile count of
the cell's stream count. tests/test_stepper_cells.py checks on the CPU that
the inputs hold what they are about.
"""
import numpy as np
import pytest

import oracle_lib as O
import stepper_cells as SC

pytestmark = pytest.mark.gpu


def _probe(ctx):
    """The default lane chunk and a lane's record capacity of the loaded
    pattern's stepper, from a scan of a few bytes."""
    ctx.set_lane_chunk(0)
    ctx.scan(b"probe\n")
    st = ctx.scan_stats()
    return st["lane_chunk"], st["lane_slots"]


def _scan_check(ctx, cell, case, geo):
    got = ctx.scan(case.data)
    st = ctx.scan_stats()
    want = O.grep_map(cell.pattern, case.data, threads=16)
    print("%s %s: n=%d records=%d stepper=%s lane_chunk=%d lane_slots=%d tiles=%d pending=%d overflow_lanes=%d" % (
        cell.name, case.name, len(case.data), len(want[0]), st["stepper"], st["lane_chunk"], st["lane_slots"],
        st["tiles"], st["pending"], st["overflow_lanes"]))
    assert len(got[0]) == len(want[0]), (cell.name, case.name, len(got[0]), len(want[0]))
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (cell.name, case.name))
    assert st["stepper"] == cell.expected["stepper"], st
    assert st["lane_chunk"] == geo.C, st
    if st["stepper"] == "table":
        assert st["lane_chunk"] == 2048, st
    # the host's tile: 64 lanes x the cell's chunks per lane
    assert st["tiles"] == -(-len(case.data) // SC.tile_bytes(geo)), (st, geo)
    assert st["matches"] == len(want[0]), st
    SC.check_planted(case, geo, want)
    return st


@pytest.mark.parametrize("gen", list(SC.GENERATORS))
@pytest.mark.parametrize("cell", SC.CELLS, ids=lambda c: c.name)
def test_cell(gpu_ctx, cell, gen):
    ctx = gpu_ctx
    try:
        ctx.set_stepper(cell.force)
        cp = ctx.load(cell.pattern)
        assert (cp.nstates, cp.nclasses) == (cell.S, cell.K)
        C, cap = _probe(ctx)
        default = SC.geometry(cell)
        # the inputs are those the CPU tests checked: same chunk, same capacity
        assert (C, cap) == (default.C, default.cap), (C, cap, default)
        geo, cases = SC.cases(cell, gen, SC.geometry(cell, C, cap))
        ctx.set_lane_chunk(geo.force_chunk)
        for case in cases:
            st = _scan_check(ctx, cell, case, geo)
            if gen == "dense":
                if case.planted["overflow"]:
                    assert st["overflow_lanes"] > 0, st
            else:
                # sparse enough for every lane's slots: the scan kernel itself
                # wrote these records, not the overflow pass
                assert st["overflow_lanes"] == 0, st
            if gen == "long":
                if cell.name in SC.NO_PARKING:
                    # above 256 states the long-line table is not built: the
                    # pair stepper's lanes read their long lines to the end
                    assert st["pending"] == 0, st
                elif cell.S <= 256:
                    assert st["pending"] > 0, st
    finally:
        ctx.set_lane_chunk(0)
        ctx.set_stepper("auto")


def test_table_refuses_257_states_and_the_context_stays_usable(gpu_ctx):
    import dgrep

    ctx = gpu_ctx
    cell = SC.REFUSED
    try:
        ctx.set_stepper(cell.force)
        with pytest.raises(dgrep.DgrepError) as e:
            ctx.load(cell.pattern)
        assert e.value.code == dgrep.DGREP_E_UNSUPPORTED
        ctx.set_stepper("auto")
        ctx.load(b"error")
        data = b"ok\nan error\n" + cell.hit + b"\nerror"
        got = ctx.scan(data)
        want = O.grep_map(b"error", data)
        assert len(want[0]) == 2
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
        assert ctx.scan_stats()["stepper"] == "sheng"
        # and the refused pattern itself runs where the loader would put it
        ctx.load(cell.pattern)
        got = ctx.scan(data)
        want = O.grep_map(cell.pattern, data)
        assert len(want[0]) == 1
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
        assert ctx.scan_stats()["stepper"] == "pair"
    finally:
        ctx.set_stepper("auto")


def test_a_refused_load_leaves_the_loaded_pattern_whole(gpu_ctx):
    """dgrep_load_dfa's failure rule (dgrep.h): a refusal found on the host
    leaves the context exactly as it was. pair-9 stays loaded through three
    refusals -- a pair table that does not fit, a filter of 3 rows, and a row
    cap that leaves a 257-state DFA without a stepper -- its scan gives the same
    lines after each, and a stream opened before them still feeds."""
    import dgrep

    ctx = gpu_ctx
    cells = {c.name: c for c in SC.CELLS}
    pair9 = cells["pair-9"]
    try:
        ctx.set_stepper("auto")
        ctx.load(pair9.pattern)
        data = bytes(SC.pad(4096 - len(pair9.hit) - 1, pair9)) + pair9.hit + b"\n"
        for at in (100, 1500, 3000):
            data = data[:at] + b"\n" + pair9.hit + b"\n" + data[at + len(pair9.hit) + 2:]
        assert len(data) == 4096
        want = O.grep_map(pair9.pattern, data)
        assert len(want[0]) >= 4

        def check():
            got = ctx.scan(data)
            for g, w in zip(got, want):
                np.testing.assert_array_equal(g, w)
            assert ctx.scan_stats()["stepper"] == "pair"

        check()
        half = len(data) // 2
        with ctx.stream(1 << 16) as s:
            first = s.feed(data[:half])
            attempts = (
                ("pair", 0, cells["table-auto-32"],
                 "dgrep_load_dfa: the pair stepper's two-byte table does not fit this DFA"),
                ("filter", 3, pair9, "dgrep_load_dfa: the filter stepper cannot hold this DFA's first states"),
                ("auto", 3, cells["filter-257"], "dgrep_load_dfa: a DFA of 257 states needs the filter stepper"),
            )
            for force, rows, cell, message in attempts:
                ctx.set_stepper(force, rows)
                with pytest.raises(dgrep.UnsupportedPattern) as e:
                    ctx.load(cell.pattern)
                assert e.value.code == dgrep.DGREP_E_UNSUPPORTED and str(e.value).endswith(": " + message), e.value
                check()
            rest = [s.feed(data[half:]), s.finish()]
            got = [np.concatenate([first[k]] + [r[k] for r in rest]) for k in range(3)]
            for g, w in zip(got, want):
                np.testing.assert_array_equal(g, w)
    finally:
        ctx.set_stepper("auto")
