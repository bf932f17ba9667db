"""The whole-DFA resolution of parked filter lines (long_dfa_seg1_kernel,
long_dfa_fix_kernel) against the oracle AND against the CPU model of its
segment guesses (tests/test_long_guess_emulation.py): the scan's
long_segments / long_guess_misses counters must equal the model's counts
exactly -- both are functions of the DFA and the bytes alone -- so the serial
re-run of a segment whose guesses miss is known to run where the model says
it must (k count mod 5 / mod 7, mod 3 with 300 keywords, a u32 DFA with five
memory classes), and a seed-selection regression fails a test instead of
only slowing a scan down. The u32 kernels see parked lines here too.

Model = kernels on the MI355X (segments walked, segments re-run):

    case          states   segments  misses
    kw100            709       46       0
    kw100_mod2     1,416       55       0
    kw100_mod3     2,123       60       0
    kw100_mod5     3,537       51      10
    kw100_mod7     4,951       53      13
    kw300_mod3     6,350       50      10
    kw300_mod5    10,582       64      19
    u32_window   131,073       59       0
    u32_mod5      65,538       56       9

Also here: the pending list outgrown by one scan (more than 1,024 parked
lines), on every stepper that parks."""
import functools
import random

import numpy as np
import pytest

import long_guess_cases as C
import oracle_lib as O

pytestmark = pytest.mark.gpu


def _check(ctx, pattern, data, want=None):
    """Bit-exact records (line numbers, starts, 64-bit lengths) vs the oracle."""
    ln, st, le = ctx.scan(data)
    oln, ost, ole = want if want is not None else O.grep_map(pattern, data, threads=16)
    assert len(ln) == len(oln), (len(ln), len(oln))
    np.testing.assert_array_equal(ln, oln)
    np.testing.assert_array_equal(st, ost)
    np.testing.assert_array_equal(le.astype(np.uint64), ole.astype(np.uint64))
    return ctx.scan_stats()


@pytest.mark.parametrize("name", C.CASE_IDS)
def test_parked_filter_lines_guess_counts(gpu_ctx, name):
    import test_long_guess_emulation as M

    case = C.CASES[C.CASE_IDS.index(name)]
    lines = C.long_lines(case)
    data, _ = C.split_of(lines)
    segments, misses, _, _ = M.model(name)
    try:
        gpu_ctx.set_lane_chunk(4096)
        pattern = C.pattern_of(case)
        cp = gpu_ctx.load(pattern)
        assert (cp.nstates > 65535) == name.startswith("u32"), cp.nstates
        st = _check(gpu_ctx, pattern, data)
        print("%s: states %d model (%d, %d) kernels (%d, %d) pending %d" % (
            name, cp.nstates, segments, misses, st["long_segments"], st["long_guess_misses"], st["pending"]))
        assert st["stepper"] == "filter" and st["lane_chunk"] == 4096, st
        assert st["pending"] == len(lines), st
        assert st["long_segments"] == segments, (st, segments, misses)
        assert st["long_guess_misses"] == misses, (st, segments, misses)
    finally:
        gpu_ctx.set_lane_chunk(0)


def test_counters_zero_without_parked_filter_lines(gpu_ctx):
    """No parked line on the filter, and parked lines on a <= 256-state stepper."""
    import dgrep

    short = dgrep.synth_corpus_host(1 << 20, 3, 1)
    pattern = C.pattern_of(C.CASES[0])
    gpu_ctx.load(pattern)
    st = _check(gpu_ctx, pattern, short)
    assert st["stepper"] == "filter" and st["pending"] == 0, st
    assert st["long_segments"] == 0 and st["long_guess_misses"] == 0, st
    data = short + b"q" * 300000 + b" error\n" + short
    gpu_ctx.load(b"error")
    st = _check(gpu_ctx, b"error", data)
    assert st["stepper"] == "sheng" and st["pending"] > 0, st
    assert st["long_segments"] == 0 and st["long_guess_misses"] == 0, st


@functools.lru_cache(maxsize=None)
def _many_parked_lines(plant, nlines=1300):
    """About 16 MiB: lines of 10-14 KiB (parked at 4 KiB lane chunks), a third
    with `plant` inside, one or two short lines after each."""
    rnd = random.Random(1300)
    fill = bytes(rnd.choice(b"abcdfghij ") for _ in range(16384))
    out = []
    for i in range(nlines):
        n = rnd.randrange(10 << 10, 14 << 10)
        q = rnd.randrange(16384 - n)
        body = bytearray(fill[q:q + n])
        if i % 3 == 0:
            at = rnd.choice([0, n - len(plant), rnd.randrange(n - len(plant))])
            body[at:at + len(plant)] = plant
        out.append(bytes(body))
        out.append(b"short line %d" % i)
        if i % 2:
            out.append(b"%d an " % i + plant)
    return b"\n".join(out) + b"\n"


# None: the 100-keyword filter pattern, built in the test; the anchored pattern
# has 8 states (Sheng by default), so the pair stepper is asked for
REGROW = [("auto", b"error", "sheng"), ("pair", b"^[a-j ]*error[a-j ]*$", "pair"), ("table", b"error$", "table"),
          ("auto", None, "filter")]


@pytest.mark.parametrize("force,pattern,stepper", REGROW, ids=[r[2] for r in REGROW])
def test_pending_list_regrows(force, pattern, stepper):
    """More parked lines than a fresh context's pending list holds (1,024): the
    list grows to the scan's count and the scan runs again; the next scan of
    the same bytes fits at once and gives the same records."""
    import torch

    import dgrep

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    pattern = pattern or C.pattern_of(C.CASES[0])
    many_parked = _many_parked_lines(dgrep.synth_keywords(4, 1)[0].upper() if stepper == "filter" else b"error")
    want = O.grep_map(pattern, many_parked, threads=16)
    assert 400 < len(want[0]) < 1300
    ctx = dgrep.Context(0)
    try:
        ctx.set_stepper(force)
        ctx.set_lane_chunk(4096)
        ctx.load(pattern)
        st = _check(ctx, pattern, many_parked, want=want)
        assert st["stepper"] == stepper, st
        assert st["pending"] > 1024, st
        assert st["scan_attempts"] >= 2, st
        st = _check(ctx, pattern, many_parked, want=want)
        assert st["scan_attempts"] == 1 and st["pending"] > 1024, st
    finally:
        ctx.close()
