"""Over-budget patterns whose NFA program has more than 1024 rune-set positions
(up to DGREP_NFA_MAX_POS = 8192, include/dgrep_blob.h). The compiler emits the
same program layout as for narrower ones; here it is interpreted on the CPU
(tests/nfa_runner.py) and must reproduce the oracle's Map output
(grep.go:17-29) bit-exactly, the limit is pinned from both sides and the blob
validator is checked on a wide program."""
import ctypes

import numpy as np
import pytest

import dgrep
import oracle_lib as O
from nfa_runner import NfaProgram, nfa_only, run_partial
from nfa_wide_cases import (E_ACUTE, RULES_POSITIONS, WORD_PATTERN, WORD_POSITIONS, ab_lines, ab_pattern, rule,
                            rule_set)


def _eq(got, want, what):
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g.astype(np.int64), w.astype(np.int64), err_msg=str(what))


def _lines_ab(npos):
    hit, miss = ab_lines(npos)
    if npos == 8192:
        # the interpreter walks every bit of an 8192-bit set per rune: three lines
        return [hit, miss, b"\xffa\xe2\x82b"]
    return [hit, miss, b"ab" * (npos // 2 + 3), b"", E_ACUTE * 40, b"\xffa\xe2\x82b"]


_WORD_T = 1060
CASES = [(ab_pattern(n), n, _lines_ab(n)) for n in (1025, 2048, 2049, 4097, 8192)] + [
    (WORD_PATTERN, WORD_POSITIONS,
     [b"x" + b"a" + b"b" * _WORD_T, b"x" + b"a" + b"b" * (_WORD_T - 1), b"zx" + b"a" + b"b" * _WORD_T,
      b"z xb" + b"ab" * (_WORD_T // 2 + 3), b"", E_ACUTE * 40, b"\xffxa\xe2\x82b"]),
    (rule_set(), RULES_POSITIONS,
     [rule(7), rule(7, 8), b"\xffkw119a\xfftail119b!", b"", E_ACUTE * 40, b"kw000akw001a tail001b", b"tail003b kw003a"]),
]


@pytest.mark.parametrize("pattern,npos,lines", CASES, ids=[str(c[1]) for c in CASES])
def test_wide_program_vs_oracle(pattern, npos, lines):
    cp = dgrep.CompiledPattern(pattern, state_budget=64)
    assert cp.partial, cp.flags
    assert cp.nfa_positions == npos
    prog = NfaProgram(cp.nfa_program())
    assert prog.npos == npos and prog.nw == (npos + 31) // 32
    assert prog.nctx == (4 if pattern == WORD_PATTERN else 1)
    data = b"\n".join(lines)
    want = O.grep_map(pattern, data)
    assert 0 < len(want[0]) < len(lines)
    _eq(run_partial(cp, data), want, pattern[:40])
    _eq(nfa_only(cp, data), want, pattern[:40])


def test_nfa_positions_of_other_blobs():
    assert dgrep.CompiledPattern(b"error").nfa_positions == 0
    cp = dgrep.CompiledPattern(b"[ab]*a[ab]{21}")
    assert cp.partial and cp.nfa_positions == 23 == NfaProgram(cp.nfa_program()).npos


def test_rule_set_compiles_at_the_default_budget():
    """120 `kwNNNa.*tailNNNb` rules: the DFA passes 2^21 states, so the blob is
    the first 65,534 rows + CAND and a 1,800-position program."""
    cp = dgrep.CompiledPattern(rule_set())
    assert cp.partial and cp.nstates == 65535, (cp.flags, cp.nstates)
    assert cp.nfa_positions == RULES_POSITIONS == 1800


def test_upper_limit():
    with pytest.raises(dgrep.DgrepError) as ei:
        dgrep.CompiledPattern(ab_pattern(8193), state_budget=64)
    assert ei.value.code == dgrep.DGREP_E_TOO_LARGE
    assert "8192" in str(ei.value)


def _bad(blob: bytes) -> bool:
    info = dgrep._BlobInfo()
    return dgrep.lib().dgrep_blob_info_get(blob, len(blob), ctypes.byref(info)) == dgrep.DGREP_E_INVALID


def test_blob_info_checks_a_wide_program():
    cp = dgrep.CompiledPattern(ab_pattern(1025), state_budget=64)
    off = 288 + 4 * cp.nstates * cp.nclasses
    prog = np.frombuffer(cp.blob[off:], dtype=np.uint32).copy()
    npos, nw, nrc, nnodes = (int(x) for x in prog[1:5])
    assert (npos, nw) == (1025, 33) and not _bad(cp.blob)

    def with_word(i, v):
        p = prog.copy()
        p[i] = np.uint32(v)
        return cp.blob[:off] + p.tobytes()

    assert _bad(with_word(1, 8193))      # npos above DGREP_NFA_MAX_POS
    assert _bad(with_word(2, nw + 1))    # nw != ceil(npos / 32)
    # npos % 32 == 1: bit 1 of a set's last word is a position beyond npos
    has_last = 8 + nnodes * 256 + nnodes + nrc + nrc * nw - 1
    assert _bad(with_word(has_last, int(prog[has_last]) | 2))
