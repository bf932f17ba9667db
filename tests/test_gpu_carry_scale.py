"""The bounded stream's walk and cut at windows past one cut tile and one batch
of the fix kernel (carry_cases.SCALE_WINDOWS: 64 KiB, 128 KiB, 1 MiB). At the
windows of window_cases.WINDOWS a walk is at most 64 chunks of 256 bytes and
the cut pass one workgroup; tests/test_carry_emulation.py lists, from the
model, what these splits reach beyond that.

Records are compared as in test_gpu_carry.py. What is new is that the stream's
figures equal the model's exactly: `chunks` pins the plan of every walk, and
`guess_misses` is the only observable of the chunk kernel's lookback -- the
records do not depend on the guesses, so a lookback at the wrong offset, seeds
that collapse or a guess in the wrong slot shows nowhere else."""
import pytest

import carry_cases as CC
import oracle_lib as O
import test_gpu_carry as TG
import window_cases as WC

pytestmark = pytest.mark.gpu


def _num_cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _pairs():
    return [(W, p) for W in CC.SCALE_WINDOWS for p in CC.SCALE_PATTERNS if W < (1 << 20) or p in CC.SCALE_1M]


def _load(ctx, pname):
    """the pattern, loaded; its tables lie on the side of kCarryRowsLds and of 65535 the case is meant for"""
    cp = ctx.load(CC.SCALE_PATTERNS[pname])
    assert not cp.partial
    rows16 = cp.nstates * cp.nclasses * 2
    if pname == "u32":
        assert cp.nstates > 65535 and not CC.rows_in_lds(cp.nstates, cp.nclasses)
    elif pname == "u16_global":
        assert cp.nstates <= 65535 and rows16 > CC.CARRY_ROWS_LDS and not CC.rows_in_lds(cp.nstates, cp.nclasses)
    else:
        assert cp.nstates <= 65535 and rows16 <= CC.CARRY_ROWS_LDS and CC.rows_in_lds(cp.nstates, cp.nclasses)
    return cp


@pytest.mark.parametrize("W,pname", _pairs())
def test_scale_walks_equal_the_model(gpu_ctx, W, pname):
    ctx, pattern = gpu_ctx, CC.SCALE_PATTERNS[pname]
    dfa, rx = CC.Dfa(_load(ctx, pname)), O.Regexp(pattern)
    cus = _num_cus()
    misses = 0
    for case in CC.scale_cases(W, pname):
        pieces = WC.pieces_of(case.data, case.cuts)
        model, info = CC.bounded(pieces, W, dfa, rx.match, num_cus=cus)
        # resident, one-shot bounded and the stream's calls against the oracle and the model; the footprint after
        # every feed; a resident scan right after
        _, stats = TG._check(ctx, "scale/" + case.name, pattern, case.data, pieces, W, model=model)
        walks = info["walks"]
        print(case.name, {k: stats[k] for k in ("folds", "folded_bytes", "max_carry", "chunks", "guess_misses")},
              [w[3:] for w in walks])
        assert stats["folds"] == info["folds"] >= 3, (case.name, stats)
        assert stats["folded_bytes"] == info["folded_bytes"], (case.name, stats)
        assert stats["max_carry"] == info["max_carry"], (case.name, stats, info["max_carry"])
        assert stats["chunks"] == sum(w[4] for w in walks), (case.name, stats, walks)
        assert stats["guess_misses"] == sum(w[5] for w in walks), (case.name, stats, walks)
        misses += stats["guess_misses"]
    # an automaton that converges within the lookback is never walked again
    if pname in ("error", "keywords", "c3", "mod3", "u16_global", "u32"):
        assert misses == 0
    else:
        assert misses > 0
