"""The stepper cells (tests/stepper_cells.py) on the CPU: every cell compiles
to the tabled DFA size, the loader's rule -- restated from the constants the
sources name -- picks the tabled instantiation, the compiled DFA agrees with
the oracle on every generated input, and every input holds what its generator
planted. A GPU failure of tests/test_gpu_stepper_cells.py then points at the
kernel or the loader, not at the compiler or a generator."""
import numpy as np
import pytest

import dfa_runner
import dgrep
import oracle_lib as O
import stepper_cells as SC

ALL = SC.CELLS + [SC.REFUSED]
_compiled = {}


def compiled(cell):
    if cell.name not in _compiled:
        _compiled[cell.name] = dgrep.CompiledPattern(cell.pattern)
    return _compiled[cell.name]


def test_cell_names_are_distinct_and_cover_every_choice():
    names = [c.name for c in ALL]
    assert len(set(names)) == len(names)
    lim = SC.limits()
    assert {c.expected["stepper"] for c in SC.CELLS} == {"sheng", "pair", "table", "filter"}
    # every table row step with every stream count it runs, every pair build
    assert ({(c.expected["rows"], c.expected["streams"]) for c in SC.CELLS if c.expected["stepper"] == "table"} ==
            {(r, lim["table_streams"] if r <= lim["stream_rows"] else 1) for r in lim["table_rows"]})
    assert ({(c.expected["entry"], c.expected["lds"]) for c in SC.CELLS if c.expected["stepper"] == "pair"} ==
            {("u32", lim["pair32_small"]), ("u32", lim["kPairW32MaxImage"]), ("u16", lim["pair16_small"]),
             ("u16", lim["kPairMaxImage"])})
    # the state counts on both sides of every table edge, and of the Sheng and filter limits
    forced = {c.S for c in SC.CELLS if c.force == "table"}
    assert forced == {16, 17, 32, 33, 64, 65, 128, 129, 256}
    auto = {c.S for c in SC.CELLS if c.force == "auto"}
    assert {lim["sheng_max"], lim["sheng_max"] + 1, 255, 256, 257} <= auto
    assert set(SC.NO_PARKING) == {c.name for c in SC.CELLS if c.expected["stepper"] == "pair" and c.S > 256}


@pytest.mark.parametrize("cell", ALL, ids=lambda c: c.name)
def test_cell_compiles_to_its_size_and_the_loader_rule_picks_it(cell):
    cp = compiled(cell)
    assert (cp.nstates, cp.nclasses) == (cell.S, cell.K)
    assert not cp.partial and not cp.go_syntax_error
    got = SC.choose(cp.nstates, cp.nclasses, SC.pair_shadow_states(cp), cell.force, SC.limits())
    assert got == cell.expected


@pytest.mark.parametrize("cell", ALL, ids=lambda c: c.name)
def test_hit_and_miss_do_what_the_generators_assume(cell):
    cp = compiled(cell)
    m = cell.miss
    for line, want in ((cell.hit, True), (m * 7 + cell.hit, True), (m * 7, False), (b"", False),
                       (cell.hit[1:], False), (cell.hit[:-1] + m, False)):
        assert dfa_runner.match_line(cp, line) == want, line[:40]
        assert O.Regexp(cell.pattern).match(line) == want, line[:40]


@pytest.mark.parametrize("gen", list(SC.GENERATORS))
@pytest.mark.parametrize("cell", SC.CELLS, ids=lambda c: c.name)
def test_generated_input(cell, gen):
    """run_blob on the compiled DFA == the oracle, and the planted shapes are
    among the oracle's records."""
    cp = compiled(cell)
    geo, cases = SC.cases(cell, gen, SC.geometry(cell))
    assert cases
    visited = set()
    for case in cases:
        assert len(case.data) <= (5 << 18), (case.name, len(case.data))
        want = O.grep_map(cell.pattern, case.data, threads=8)
        got = dfa_runner.run_blob(cp, case.data, visited)
        assert len(got[0]) == len(want[0]), case.name
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g.astype(np.uint64), w, err_msg=case.name)
        SC.check_planted(case, geo, want)
    # the walk enters the table image's last row (a truncated image shows): at
    # 256 states that is state id 255, the highest a u8 entry holds
    if cell.expected["stepper"] == "table":
        assert cell.S - 1 in visited, (cell.name, gen)
    if gen == "dense":
        # the dense input overflows a lane wherever the hit is short enough
        assert cases[0].planted["overflow"] == (len(cell.hit) <= 40), cell.name


def test_a_moved_limit_moves_a_cell():
    """choose() follows the constants: one row less in a table step, a smaller
    u32 image limit or one Sheng state more changes a cell's instantiation."""
    lim = SC.limits()

    def pick(cell, **change):
        cp = compiled(cell)
        return SC.choose(cp.nstates, cp.nclasses, SC.pair_shadow_states(cp), cell.force, dict(lim, **change))

    by = {c.name: c for c in SC.CELLS}
    assert pick(by["table-64"], table_rows=[16, 32, 63, 128, 256])["rows"] == 128
    assert pick(by["table-64"], stream_rows=32)["streams"] == 1
    assert pick(by["pair-302"], kPairW32MaxImage=14000)["entry"] == "u16"
    assert pick(by["pair-9"], sheng_max=9)["stepper"] == "sheng"
    assert pick(by["pair-u16-edge"], kPairMaxT2=28187)["stepper"] == "table"  # its T2 is 28,188 B
