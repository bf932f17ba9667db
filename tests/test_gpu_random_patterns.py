"""Random patterns on the GPU (tests/random_pattern_cases.py): every selected
pattern through every stepper the loader can be made to pick and every scan
entry point -- resident, batch, windowed, bounded -- bit for bit against the
oracle's records. The inputs cross chunk and tile edges and hold long lines
that the runtime parks (resident scan) or folds (bounded scan).

The hand-written patterns of the other GPU tests fix the DFA's size; these
vary its structure, which is what the loader's images (Sheng's shuffle table,
the pair image with its shadow states, the u8 table, the filter's rows with
CAND_END and the whole-DFA image, the long-line table, the carry table with
its absorbing flags, the NFA program) depend on.
tests/test_random_pattern_cases.py checks the same cases on the CPU.

Modes: `auto` (the loader's own choice, which must be the one
stepper_cells.choose predicts), `table` (DFAs of at most 256 states), `pair`
(accepted exactly when the pair image fits; a refusal where it does not is the
expected outcome), `filter` (as many LDS rows as fit), `filter-few` (a cap of 3
rows is refused for every DFA, since start, start_m, CAND and CAND_END take
four; at 4 rows nearly every line is a candidate) and `partial` (state budget
3: the NFA program decides the lines that leave the kept states, and the
bounded scan refuses the blob).
"""
import collections

import numpy as np
import pytest
import torch  # noqa: F401  the cases load libdgrep.so while they are collected: torch's HIP runtime goes first

import random_pattern_cases as R

pytestmark = pytest.mark.gpu

MODES = ("auto", "table", "pair", "filter", "filter-few", "partial")
PIECE = 10007  # the bounded stream's feeds: cuts at no line, chunk or window edge

# what the tests saw, for the tallies: (mode, bucket) -> [(case, pending, whether the runtime parks there)]
_pending = collections.defaultdict(list)
_pair_refused = []
_nfa_share = []


def _applies(case, mode):
    return mode != "table" or case.nstates <= 256


def _params():
    out = []
    for case in R.selected() + R.regressions():
        for mode in MODES:
            if _applies(case, mode):
                out.append(pytest.param(case, mode, id="%s-%s" % (case.name, mode)))
    return out


def _same(got, want, case, mode, entry):
    """exact on (line_no, start, len); the message names the first record that differs"""
    g = list(zip(*[np.asarray(x, np.uint64).tolist() for x in got[:3]]))
    w = list(zip(*[x.tolist() for x in want]))
    if g == w:
        return
    k = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
    raise AssertionError("pattern %r mode %s entry %s: %d records, the oracle %d; record %d is %r, the oracle's %r" % (
        case.pattern, mode, entry, len(g), len(w), k, g[k] if k < len(g) else None, w[k] if k < len(w) else None))


def _load(ctx, case, mode):
    """Sets the mode and loads the pattern: (the CompiledPattern, the stepper
    the scans must report), or None where the load was refused as predicted."""
    import dgrep

    cp = R.compiled(case.pattern)
    if mode == "auto":
        ctx.set_stepper("auto", 0)
        ctx.load(cp)
        return cp, R.auto_choice(cp)["stepper"]
    if mode == "table":
        ctx.set_stepper("table", 0)
        ctx.load(cp)
        return cp, "table"
    if mode == "pair":
        ctx.set_stepper("pair", 0)
        if R.pair_fits(cp) is None:
            with pytest.raises(dgrep.UnsupportedPattern) as e:
                ctx.load(cp)
            assert e.value.code == dgrep.DGREP_E_UNSUPPORTED and "pair" in str(e.value), (case.pattern, str(e.value))
            return None
        ctx.load(cp)  # a refusal here fails the test: the image fits
        return cp, "pair"
    if mode == "filter":
        ctx.set_stepper("filter", 0)
        ctx.load(cp)
        return cp, "filter"
    if mode == "filter-few":
        ctx.set_stepper("filter", 3)
        with pytest.raises(dgrep.UnsupportedPattern) as e:
            ctx.load(cp)
        assert e.value.code == dgrep.DGREP_E_UNSUPPORTED, (case.pattern, str(e.value))
        ctx.set_stepper("filter", 4)
        ctx.load(cp)
        return cp, "filter"
    assert mode == "partial"
    ctx.set_stepper("auto", 0)
    cp = R.compiled(case.pattern, R.PARTIAL_BUDGET)
    assert cp.partial, case
    ctx.load(cp)
    return cp, "filter"


def _scan_b(ctx, case, mode, stepper, cp, entry="scan(B)"):
    """the resident scan of corpus B and what it parked"""
    data = R.corpus_b()[0]
    _same(ctx.scan(data), R.want(case.pattern, "B"), case, mode, entry)
    st = ctx.scan_stats()
    assert st["stepper"] == stepper, (case.pattern, mode, entry, st)
    assert st["matches"] == len(R.want(case.pattern, "B")[0]), (case.pattern, mode, entry, st)
    parks = R.parks(stepper, cp.nstates, cp.partial)
    if not parks:
        assert st["pending"] == 0, (case.pattern, mode, entry, st)
    return st, parks


@pytest.mark.parametrize("case,mode", _params())
def test_random_pattern(gpu_ctx, case, mode):
    import dgrep

    ctx = gpu_ctx
    a, b = R.corpus_a(), R.corpus_b()[0]
    try:
        loaded = _load(ctx, case, mode)
        if loaded is None:
            _pair_refused.append(case.name)
            return
        cp, stepper = loaded

        # resident
        _same(ctx.scan(a), R.want(case.pattern, "A"), case, mode, "scan(A)")
        st = ctx.scan_stats()
        assert st["stepper"] == stepper, (case.pattern, mode, st)
        if mode == "partial":
            # the lines that leave the kept states are staged as candidates and decided by the NFA
            # program: the dropped ones are counted, the kept ones are among the matches
            cand, direct = R.partial_counts(cp, a)
            assert cand > 0, case
            assert st["matches"] + st["candidates"] == cand + direct, (case.pattern, st, cand, direct)
            _nfa_share.append((cand, a.count(b"\n") + 1))
        st, parks = _scan_b(ctx, case, mode, stepper, cp)
        _pending[(mode, case.bucket)].append((case.name, st["pending"], parks))
        _same(ctx.scan(b""), R.want(case.pattern, ("split", 3)), case, mode, "scan(b'')")

        # batch: every split's records against the oracle's for that split
        splits = R.splits_of(a)
        ln, start, length, split, begin = ctx.scan_batch(splits)
        assert begin[0] == 0 and begin[-1] == len(ln) and len(begin) == len(splits) + 1, (case.pattern, mode, begin)
        for i in range(len(splits)):
            lo, hi = int(begin[i]), int(begin[i + 1])
            assert lo <= hi and (split[lo:hi] == i).all(), (case.pattern, mode, "scan_batch", i)
            _same((ln[lo:hi], start[lo:hi], length[lo:hi]), R.want(case.pattern, ("split", i)), case, mode,
                  "scan_batch split %d" % i)

        # windowed
        for w in (4096, 65536):
            _same(ctx.scan_windowed(b, w), R.want(case.pattern, "B"), case, mode, "scan_windowed(B, %d)" % w)

        # bounded: every long line of B is longer than the window, so it is folded
        if mode == "partial":
            with pytest.raises(dgrep.UnsupportedPattern) as e:
                ctx.scan_windowed(b, 4096, bounded=True)
            assert e.value.code == dgrep.DGREP_E_UNSUPPORTED and "PARTIAL" in str(e.value), str(e.value)
        else:
            _same(ctx.scan_windowed(b, 4096, bounded=True), R.want(case.pattern, "B"), case, mode,
                  "scan_bounded(B, 4096)")
            with ctx.stream(4096, bounded=True) as s:
                calls = [s.feed(b[i:i + PIECE]) for i in range(0, len(b), PIECE)] + [s.finish()]
                folds = s.carry_stats()["folds"]
            _same([np.concatenate([c[k] for c in calls]) for k in range(3)], R.want(case.pattern, "B"), case, mode,
                  "bounded stream fed %d bytes a call" % PIECE)
            assert folds > 0, (case.pattern, mode, folds)

        # chunk edges elsewhere
        if mode == "auto":
            ctx.set_lane_chunk(8192)
            st, _ = _scan_b(ctx, case, mode, stepper, cp, "scan(B) at lane chunk 8192")
            if stepper != "table":
                assert st["lane_chunk"] == 8192, st
    finally:
        ctx.set_stepper("auto", 0)
        ctx.set_lane_chunk(0)


def test_parked_lines_were_exercised(gpu_ctx):
    """Some pattern of every mode and bucket where the runtime parks at all
    had lines parked in corpus B (pending > 0). A (mode, bucket) that no test
    of this run covered (a deselected one) is scanned here."""
    ctx = gpu_ctx
    rows = []
    try:
        for mode in MODES:
            for bucket, _, _ in R.BUCKETS:
                seen = _pending.get((mode, bucket))
                if seen is None:
                    seen = []
                    for case in (c for c in R.selected() if c.bucket == bucket and _applies(c, mode)):
                        loaded = _load(ctx, case, mode)
                        if loaded is None:
                            continue
                        st, parks = _scan_b(ctx, case, mode, loaded[1], loaded[0])
                        seen.append((case.name, st["pending"], parks))
                        if st["pending"]:
                            break
                could = [x for x in seen if x[2]]
                did = [x for x in could if x[1] > 0]
                rows.append((mode, bucket, len(seen), len(could), len(did), max([x[1] for x in seen] or [0])))
    finally:
        ctx.set_stepper("auto", 0)
        ctx.set_lane_chunk(0)
    for r in rows:
        print("parked lines: mode %-10s bucket %-6s scanned %2d, the runtime parks for %2d, pending > 0 for %2d "
              "(most: %d)" % r)
    print("pair loads refused as predicted: %d (%s)" % (len(_pair_refused), " ".join(sorted(_pair_refused))))
    if _nfa_share:
        print("partial: the NFA program decided %d of %d lines of corpus A over %d patterns" % (
            sum(c for c, _ in _nfa_share), sum(n for _, n in _nfa_share), len(_nfa_share)))
    for mode, bucket, scanned, could, did, _ in rows:
        if could:
            assert did > 0, (mode, bucket)
