"""Patterns whose NFA program has more than 1024 rune-set positions
(include/dgrep_blob.h, DGREP_NFA_MAX_POS = 8192), shared by test_nfa_wide.py
(CPU) and test_gpu_nfa_wide.py (GPU): above 32 position words a candidate line
is decided by one wave (verify_nfa_wave_kernel) instead of one lane."""

E_ACUTE = "é".encode()
CJK = "中".encode()

# \b gives the program four closure contexts (nctx = 4): 1 + 1 + 1 + 1060 positions
WORD_PATTERN = b"\\bx[ab]*a[ab]{1000}[ab]{60}"
WORD_POSITIONS = 1063
# multi-byte rune classes through the decoder trie
LETTER_PATTERN = b"x\\pL{1000}\\pL{40}y"


def ab_pattern(npos: int) -> bytes:
    """[ab]*a[ab]{T} with T + 2 = npos positions, in repeats of at most 1000
    (Go's limit for one repeat count)."""
    t = npos - 2
    assert t >= 1
    pat = b"[ab]*a"
    while t:
        k = min(t, 1000)
        pat += b"[ab]{%d}" % k
        t -= k
    return pat


def ab_lines(npos: int):
    """(the shortest matching line, its non-matching neighbour one byte shorter)"""
    t = npos - 2
    return b"a" + b"b" * t, b"a" + b"b" * (t - 1)


N_RULES = 120
RULES_POSITIONS = N_RULES * 15  # per rule: 6 runes of kwNNNa, the '.', 8 runes of tailNNNb


def rule(i: int, j: int = None) -> bytes:
    """A line holding rule i's prefix and rule j's tail: a match iff i == j."""
    return b"kw%03da zz tail%03db" % (i, i if j is None else j)


def rule_set() -> bytes:
    return b"|".join(b"kw%03da.*tail%03db" % (i, i) for i in range(N_RULES))
