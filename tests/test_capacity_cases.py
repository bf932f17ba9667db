"""The inputs of the capacity matrix (capacity_cases.py), checked with the
oracle alone: every (configuration, shape) holds at least four matching lines,
so the capacities C // 2, C - 1, C and C + 1 are distinct and neither 0 nor 1,
and every shape is what its pass needs -- found here, not on a GPU."""
import numpy as np
import pytest

import capacity_cases as K

CASES = [(cfg, shape) for cfg in K.CONFIGS for shape in K.SHAPES]
IDS = ["%s-%s" % (cfg.name, shape) for cfg, shape in CASES]


@pytest.mark.parametrize("cfg,shape", CASES, ids=IDS)
def test_count_is_at_least_four(cfg, shape):
    data, (ln, st, le) = K.case(cfg, shape)
    count = len(ln)
    assert count >= 4, (cfg.name, shape, count)
    caps = K.capacities(count)
    assert caps[:8] == [0, 1, count // 2, count - 1, count, count + 1, 0, count]
    assert caps[8:] == [count - 1, count // 2, 1]  # short calls on a context that has seen a larger one
    assert 1 < count // 2 < count - 1 < count < count + 1
    assert 30000 < len(data) <= 4 << 20  # the single-thread oracle stays well under a second
    assert K.case(cfg, shape)[1][0] is ln  # computed once


@pytest.mark.parametrize("cfg", K.CONFIGS, ids=[c.name for c in K.CONFIGS])
def test_shapes_are_what_their_pass_needs(cfg):
    # plain: a '\n' on both sides of every edge
    data, _ = K.case(cfg, "plain")
    assert all(data[e] == 10 for e in K.EDGES)
    # dense: every line matches, and a lane chunk holds more of them than the
    # lane has record slots and spill records, so the overflow pass must run
    data, (ln, _, _) = K.case(cfg, "dense")
    assert len(ln) == data.count(b"\n") + 1
    chunk = K.lane_chunk(cfg, "dense") or {"table": 2048, "pair": 4608}.get(cfg.stepper, 4096)  # the compiled chunks
    records = {"sheng": 23 + 240, "pair": 16 + 240, "table": 6, "filter": 4 + 240}[cfg.stepper]  # slots + spill
    assert chunk // (len(cfg.hit) + 1) > records, (cfg.name, chunk, records)
    # parked: long lines that match and long lines that do not
    data, (_, _, le) = K.case(cfg, "parked")
    lines = data.split(b"\n")
    long_lines = sum(len(l) >= K.LONG for l in lines)
    long_hits = int(np.count_nonzero(le >= K.LONG))
    assert 0 < long_hits < long_lines, (cfg.name, long_hits, long_lines)
    # dense_long: the one long line does not match, hundreds of lines before it do
    data, (_, _, le) = K.case(cfg, "dense_long")
    assert max(map(len, data.split(b"\n"))) > 6 * 4096 and int(le.max()) < 100 and len(le) > 300
