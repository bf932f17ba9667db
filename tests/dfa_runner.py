"""Test-side interpreter of a compiled DFA blob (include/dgrep_blob.h).

Runs the automaton over a split exactly as the GPU kernel's contract says:
restart at '\\n', a line matches iff the state after its '\\n' is start_m,
the last line (no '\\n') matches iff trans[s][class('\\n')] == start_m.
Used to check the pattern compiler against the oracle on the CPU.
"""
import numpy as np


class _ByteRows:
    """row(s)[b] = next state of s on byte b, as plain lists built when a state
    is first entered (the walk is a Python loop: list indexing is several
    times faster than numpy's, and a large DFA's unvisited rows cost nothing)."""

    def __init__(self, cp):
        bc, tr = cp.tables()
        self.cls = bc.tolist()
        self.tr = tr
        self.rows = [None] * cp.nstates

    def row(self, s):
        r = self.rows[s]
        if r is None:
            t = self.tr[s].tolist()
            r = self.rows[s] = [t[c] for c in self.cls]
        return r


def _byte_rows(cp):
    br = getattr(cp, "_byte_rows", None)
    if br is None:
        br = cp._byte_rows = _ByteRows(cp)
    return br


def run_blob(cp, data: bytes, visited=None):
    """visited: a set that receives every state id the walk enters."""
    br = _byte_rows(cp)
    rows, row = br.rows, br.row
    s = cp.start
    M = cp.start_m
    out_ln, out_st, out_le = [], [], []
    line = 1
    ls = 0
    for i, b in enumerate(data):
        s = (rows[s] or row(s))[b]
        if visited is not None:
            visited.add(s)
        if b == 10:
            if s == M:
                out_ln.append(line)
                out_st.append(ls)
                out_le.append(i - ls)
            line += 1
            ls = i + 1
    if row(s)[10] == M:
        out_ln.append(line)
        out_st.append(ls)
        out_le.append(len(data) - ls)
    return (np.array(out_ln, np.uint64), np.array(out_st, np.uint64), np.array(out_le, np.uint32))


def match_line(cp, line: bytes) -> bool:
    """regexp.Match(pattern, line) through the DFA (line must not contain '\\n')."""
    assert b"\n" not in line
    ln, _, _ = run_blob(cp, line)
    return len(ln) == 1
