"""Shared by the capacity tests (test_capacity_cases.py on the CPU,
test_gpu_scan_capacity.py on the GPU): the stepper configurations, the split
shapes that send scan_resident down each of its passes, and the oracle's
records for every (configuration, shape), computed once.

A configuration names the stepper the loader must pick for its pattern and a
line (`hit`) that the pattern matches, from which the dense shapes are built.
The capacities of the matrix are relative to the oracle count C (C // 2,
C - 1, C, C + 1), so every shape here holds at least four matching lines:
test_capacity_cases.py checks that, and what each shape is for, without a GPU.
"""
import collections

import oracle_lib as O
from test_gpu_long_lines import _dense_then_long, _long_split
from test_gpu_parity import PATTERNS

C3 = PATTERNS[5]
assert C3.startswith(b"^[0-9]{4}-[0-9]{2}")
AB = b"[ab]*a[ab]{21}"  # beyond the compiler's state budget: a partial blob, candidates decided by its NFA program

# stepper: what scan_stats() must report; budget: dgrep_compile_budget's state
# budget (0 = default); force / rows: dgrep_set_stepper; chunk: the lane chunk
# set for the shapes built around a chunk edge (0 = the u8 table's fixed 2 KiB);
# dense_chunk: the lane chunk of the dense shape (0 = adaptive) -- a lane must
# own more matching lines than its slots and spill area hold (at most 263), and
# 23-byte lines do not at 4 KiB; parks: long lines are parked and resolved
# (not on partial blobs, whose lanes read a long line on).
Config = collections.namedtuple("Config", "name stepper pattern budget force rows hit chunk dense_chunk parks")

CONFIGS = [
    Config("sheng", "sheng", b"error", 0, "auto", 0, b"error", 4096, 0, True),
    Config("pair", "pair", C3, 0, "auto", 0, b"0000-00WARN a", 4096, 0, True),
    Config("table", "table", C3, 0, "table", 0, b"0000-00WARN a", 0, 0, True),
    Config("filter4", "filter", b"error", 0, "filter", 4, b"error", 4096, 0, True),
    Config("partial-error", "filter", b"error", 3, "auto", 0, b"error", 4096, 0, False),
    Config("partial-ab", "filter", AB, 0, "auto", 0, b"a" + b"b" * 21, 8192, 8192, False),
]

EDGES = (4095, 4096, 65535, 65536, 262143, 262144)
LONG = 40000  # every line of the parked shape at least this long is parked (4 KiB, or two chunks, past its chunk)


def _as_hit(cfg, line):
    """A line holding b"error" turned into one that cfg.pattern matches."""
    if cfg.hit == b"error":
        return line
    if cfg.pattern == C3:
        return b"2024-01 " + line.replace(b"error", b"WARN ab")
    return line.replace(b"error", cfg.hit)


def plain(cfg):
    """Log lines, '\\n' forced on both sides of the 4 KiB, 64 KiB and 256 KiB
    edges, and five lines that match, three of them starting right at an edge."""
    import dgrep

    d = bytearray(dgrep.synth_corpus_host(300000, 17, 0))
    for e in EDGES:
        d[e] = 10
    for at in (4097, 65537, 262145, 100000, 200000):
        d[at - 1] = 10
        d[at:at + len(cfg.hit) + 1] = cfg.hit + b"\n"
    return bytes(d)


def dense(cfg):
    """Every line matches, the last one unterminated: every lane overflows."""
    return b"\n".join([cfg.hit] * (400000 // (len(cfg.hit) + 1)))


def parked(cfg):
    """_long_split's lines of 2 B to 2 MiB, some matching, and forty short matching lines."""
    # a partial blob's long candidate lines are each decided by one lane running
    # the NFA program (seconds per scan at 2 MiB): a tenth of the length there
    key = "parked" if cfg.parks else "long"
    if key not in _cache:  # one base for the configurations that share it: _long_split draws every byte
        sizes = [10, 300, 70000, 5, 1 << 20, 40000, 9000, 100, (1 << 21) + 7, 2, 200000, 150000]
        if not cfg.parks:
            sizes = [min(s, 100000 + s // 10) for s in sizes]
        _cache[key] = _long_split(9, sizes) + b"\n" + b"\n".join(b"x error %d" % i for i in range(40))
    return b"\n".join(_as_hit(cfg, l) if b"error" in l else l for l in _cache[key].split(b"\n"))


def dense_long(cfg):
    """_dense_then_long: the lane that owns hundreds of matching lines also owns
    a long line that does not match (one staged record more than the count)."""
    c = cfg.chunk or 2048
    return _dense_then_long(c, 6 * max(c, 4096) + 123, False, dense=cfg.hit)


SHAPES = collections.OrderedDict([("plain", plain), ("dense", dense), ("parked", parked), ("dense_long", dense_long)])

_cache = {}


def case(cfg, shape):
    """(split bytes, the oracle's (line_no, start, len)) of a configuration and
    shape: built once, shared, never changed."""
    key = (cfg.name, shape)
    if key not in _cache:
        data = SHAPES[shape](cfg)
        _cache[key] = (data, O.grep_map(cfg.pattern, data))
    return _cache[key]


def lane_chunk(cfg, shape):
    """The lane chunk the shape needs set (0 = leave it adaptive)."""
    return {"dense": cfg.dense_chunk, "dense_long": cfg.chunk}.get(shape, 0)


def capacities(count):
    """The matrix's calls, in order, on one context: below, at and above the
    count, then a size query followed by an exact call -- and down again: a
    context's staging buffer is as large as the largest capacity it has seen, so
    on the way up it ends where the caller's arrays end and bounds the ordering
    pass by itself; on the way down only the pass's own `dst < capacity` does."""
    return [0, 1, count // 2, count - 1, count, count + 1, 0, count, count - 1, count // 2, 1]
