"""The bounded stream's state machine, before a GPU is involved: the
pure-Python model of carry_cases.bounded() -- the fold rule, the walk of the
carried line's last bytes, the splice, the finish -- run over a compiled
pattern's own tables, gives exactly the oracle's Map of the concatenated
pieces, for every cut, and never holds a window or more as the tail."""
import numpy as np
import pytest

import carry_cases as CC
import oracle_lib as O
import window_cases as WC

_want = {}


def _oracle(pattern, data):
    k = (bytes(pattern), data)
    if k not in _want:
        _want[k] = O.grep_map(pattern, data)
    return _want[k]


def _check(pattern, dfa, rx, name, window, data, cuts):
    pieces = WC.pieces_of(data, cuts)
    calls, info = CC.bounded(pieces, window, dfa, rx.match)
    assert len(calls) == len(pieces) + 1
    got, want = CC.flat(calls), _oracle(pattern, data)
    assert len(got) == len(want[0]), (name, len(got), len(want[0]))
    for k in range(3):
        np.testing.assert_array_equal(np.array([r[k] for r in got], np.uint64), want[k], err_msg=name)
    return got, info


@pytest.mark.parametrize("pattern", CC.PATTERNS, ids=lambda p: p.decode("utf-8") or "empty")
def test_model_equals_oracle_map(pattern):
    import dgrep

    dfa, rx = CC.Dfa(dgrep.CompiledPattern(pattern)), O.Regexp(pattern)
    seen, folds = set(), 0
    for case in WC.CASES:
        got, info = _check(pattern, dfa, rx, case.name, case.window, case.data, case.cuts)
        seen.add(len(got) > 0)
        folds += info["folds"]
        if info["folds"] == 0:  # nothing outgrew the window: the calls are those of the plain windowed model
            assert CC.bounded(WC.pieces_of(case.data, case.cuts), case.window, dfa, rx.match)[0] == \
                WC.windowed(WC.pieces_of(case.data, case.cuts), case.window, rx.match)[0], case.name
    for case in CC.LONG:
        got, info = _check(pattern, dfa, rx, case.name, case.window, case.data, case.cuts)
        assert info["folds"] >= 1 and info["max_carry"] >= case.longest, (case.name, info)
        folds += info["folds"]
        seen.add(len(got) > 0)
    for W in WC.WINDOWS:
        for seed in range(3):
            data, _ = CC.memory_line(W, seed, nwin=5)
            got, _ = _check(pattern, dfa, rx, "memory/%d/w%d" % (seed, W), W, data,
                            WC.random_cuts("memory", len(data), 3))
            seen.add(len(got) > 0)
        got, _ = _check(pattern, dfa, rx, "greek/w%d" % W, W, CC.greek_line(W), [])
        seen.add(len(got) > 0)
    assert folds > 0 and True in seen


def test_long_line_verdicts_follow_the_line():
    """the long cases decide what they were built to decide"""
    import dgrep

    dfa, rx = CC.Dfa(dgrep.CompiledPattern(CC.SHENG8)), O.Regexp(CC.SHENG8)
    lens = {}
    for case in CC.LONG:
        if case.pattern != CC.SHENG8:
            continue
        got, _ = _check(CC.SHENG8, dfa, rx, case.name, case.window, case.data, case.cuts)
        lens[case.name] = [r[2] for r in got]
    for W in WC.WINDOWS:
        assert 7 * W // 2 in lens["hit_first/whole/w%d" % W] and 7 * W // 2 in lens["hit_last/random/w%d" % W]
        assert 13 * W // 2 in lens["hit_middle/whole/w%d" % W]
        assert max(lens["miss_middle/whole/w%d" % W]) < W
        b2b = lens["back_to_back/random/w%d" % W]
        assert 5 * W // 2 + 5 in b2b and 9 * W // 4 + 5 in b2b and 13 * W // 4 not in b2b
        assert lens["ends_exact/whole/w%d" % W] == [2 * W]


def test_even_k_and_greek_decide_by_the_whole_line():
    import dgrep

    for W in WC.WINDOWS:
        dfa, rx = CC.Dfa(dgrep.CompiledPattern(CC.EVEN_K)), O.Regexp(CC.EVEN_K)
        for seed in range(4):
            data, nk = CC.memory_line(W, seed, nwin=5)
            got, info = _check(CC.EVEN_K, dfa, rx, "even", W, data, [])
            assert info["folds"] >= 4
            assert (max(r[2] for r in got) > 5 * W) == (nk % 2 == 0), (seed, nk)
        dfa, rx = CC.Dfa(dgrep.CompiledPattern(CC.GREEK)), O.Regexp(CC.GREEK)
        got, info = _check(CC.GREEK, dfa, rx, "greek", W, CC.greek_line(W), [])
        assert info["folds"] >= 6 and [r[0] for r in got] == [2, 5]


def test_invariant_holds_for_every_feed_pattern():
    """one-byte feeds of a newline-free stream: the tail never reaches a window (bounded() asserts it)"""
    import dgrep

    dfa, rx = CC.Dfa(dgrep.CompiledPattern(b"error")), O.Regexp(b"error")
    data = b"abc " * 2100 + b"error"
    for W in WC.WINDOWS:
        calls, info = CC.bounded([data[i:i + 1] for i in range(len(data))], W, dfa, rx.match)
        assert CC.flat(calls) == [(1, 0, len(data))] and info["folds"] == len(data) // W


# ---- windows past one cut tile and one batch of the fix kernel ----------------------
# (carry_cases.SCALE_WINDOWS; tests/test_gpu_carry_scale.py runs the same splits on the GPU)
_TILE = 16384  # the cut pass's tile (kTile of csrc/kernels/window.hip): one workgroup each
_scale = {}


def _scale_pairs():
    return [(W, p) for W in CC.SCALE_WINDOWS for p in CC.SCALE_PATTERNS if W < (1 << 20) or p in CC.SCALE_1M]


def _scale_rows(W, pname):
    """Every split of (W, pname) through the model for a 256-CU device: the calls equal the oracle's Map, and
    every walk's exit is Dfa.walk's. Returns one dict per walk, for the coverage test. Computed once."""
    import dgrep

    if (W, pname) in _scale:
        return _scale[W, pname]
    pattern = CC.SCALE_PATTERNS[pname]
    cp = dgrep.CompiledPattern(pattern)
    dfa, rx = CC.Dfa(cp), O.Regexp(pattern)
    rows = []
    for case in CC.scale_cases(W, pname):
        detail = []
        pieces = WC.pieces_of(case.data, case.cuts)
        calls, info = CC.bounded(pieces, W, dfa, rx.match, num_cus=256, detail=detail)
        got, want = CC.flat(calls), _oracle(pattern, case.data)
        assert len(got) == len(want[0]), (case.name, len(got), len(want[0]))
        for k in range(3):
            np.testing.assert_array_equal(np.array([r[k] for r in got], np.uint64), want[k], err_msg=case.name)
        assert len(detail) == len(info["walks"]) >= 4, case.name
        longest = max(map(len, case.data.split(b"\n")))
        assert 3 * W <= longest <= 6 * W and info["max_carry"] == longest, (case.name, longest)
        for d, w in zip(detail, info["walks"]):
            assert d["exit"] == dfa.walk(d["entry"], d["data"]), (case.name, w)
            assert w == (d["kind"], len(d["data"]), w[2], w[3], w[4], len(d["miss_chunks"]))
            row = dict(d, case=case.name, pname=pname, W=W, m=w[1], from_=w[2], chunk=w[3], nchunks=w[4], misses=w[5],
                       lds=dfa.rows_in_lds, entry_absorbing=bool(dfa.absorbing[d["entry"]]),
                       matched=longest in [r[2] for r in got])
            if d["kind"] == "head":  # the chain from `start` the head walk follows as well
                dual = {}
                CC.walk_model(dfa, d["data"], dfa.start, True, 256, dual)
                row["dual_absorbed_at"] = dual["absorbed_at"]
            rows.append(row)
    _scale[W, pname] = rows
    return rows


@pytest.mark.parametrize("W,pname", _scale_pairs())
def test_scale_model_equals_oracle_map(W, pname):
    rows = _scale_rows(W, pname)
    assert rows
    by = {r["case"]: r["matched"] for r in rows}
    pairs = [name for name in by if "/hit/" in name and name.replace("/hit/", "/miss/") in by]
    assert pairs or pname.startswith("mod")
    for name in pairs:  # one byte decides the long line
        assert by[name] and not by[name.replace("/hit/", "/miss/")], name
    if pname.startswith("mod"):
        assert {r["matched"] for r in rows} == {True, False}


def _later_tiles_all_hold_a_newline(r):
    first, fill = r["m"] // _TILE + 1, r["fill"]
    return all(b"\n" in fill[t * _TILE:(t + 1) * _TILE] for t in range(first, (len(fill) + _TILE - 1) // _TILE))


def test_scale_cases_reach_what_they_are_built_for():
    """The model shows, for a 256-CU device, every plan shape, batch edge, cut layout and chain event that
    tests/test_gpu_carry_scale.py exists to run on the GPU."""
    rows = [r for W, p in _scale_pairs() for r in _scale_rows(W, p)]
    lds = {(r["chunk"], r["nchunks"]) for r in rows if r["lds"]}
    glob = {p: {(r["chunk"], r["nchunks"]) for r in rows if r["pname"] == p} for p in ("u16_global", "u32")}
    heads = [r for r in rows if r["kind"] == "head"]
    # (a) 256, 257 and 512 chunks of 256 bytes: the fix kernel's batch edge `base + 256 < nchunks`
    assert {(256, 256), (256, 257), (256, 512)} <= lds
    # (b) chunks of 512 bytes (the lookback starts mid-chunk), 257 to 512 of them
    assert {(512, 257), (512, 512)} <= lds and any(n > 512 for c, n in lds if c == 512)
    # (c) chunks of 1024 bytes: exactly 1024, and more
    assert {(1024, 1024), (1024, 1025)} <= lds
    # (d) rows read through the caches: four times the lanes, 513 to 1024 chunks of 256 bytes, u16 and u32
    for p in glob:
        assert {(256, 513), (256, 1024)} <= glob[p] and all(c == 256 for c, _ in glob[p]), (p, glob[p])
    # (e) the last chunk: 1 to 15 bytes, whole, and a range that does not end on a 16-byte load
    last = [r["m"] - (r["nchunks"] - 1) * r["chunk"] for r in rows if r["nchunks"]]
    assert any(1 <= x <= 15 for x in last) and any(r["nchunks"] > 1 and r["m"] % r["chunk"] == 0 for r in rows)
    assert any(r["m"] % 16 for r in rows if r["nchunks"] > 256)
    assert any(0 < r["nchunks"] % 64 < 64 and r["nchunks"] > 256 for r in rows)  # a partial last register group
    # (f) head walks (two chains): beyond one batch, and beyond one register group
    assert any(r["nchunks"] > 256 for r in heads) and any(65 <= r["nchunks"] <= 256 for r in heads)
    # (g) the cut: the first '\n' behind the tail comes from another workgroup than the tail's end ...
    assert any(r["from_"] >= _TILE and r["m"] // _TILE > r["from_"] // _TILE for r in heads)
    # ... and with no tail: at a tile's last byte, a tile's first byte, and in the window's last tile, every
    # later tile holding more '\n' (so the last workgroup's own first '\n' is another one)
    for W in CC.SCALE_WINDOWS[:2]:
        for at in (_TILE - 1, _TILE, None):
            hit = [r for r in heads if r["W"] == W and r["from_"] == 0 and len(r["fill"]) == W and
                   (r["m"] == at if at else r["m"] // _TILE == W // _TILE - 1) and _later_tiles_all_hold_a_newline(r)]
            assert hit and (at is None or len(hit[0]["fill"]) // _TILE - hit[0]["m"] // _TILE >= 3), (W, at)
            assert at is not None or any(b"\n" in r["fill"][r["m"] + 1:] for r in hit)
    # (h) a miss in a later batch; the count-modulo-7 lines miss in every batch of every long walk
    assert any(r["miss_chunks"] and r["miss_chunks"][-1] >= 256 for r in rows)
    for r in rows:
        if r["pname"] == "mod7" and r["nchunks"] >= 64:
            # (a batch of fewer than 64 chunks, such as the 257th chunk alone, may hold none)
            assert {c // 256 for c in r["miss_chunks"]} >= set(range((r["nchunks"] + 192) // 256)), r["case"]
    # (i) the chain turns absorbing in a later batch; a walk enters in an absorbing state
    assert any((r["absorbed_at"] or 0) >= 256 for r in rows)
    assert any(r["absorbed_at"] == -1 and r["entry_absorbing"] and r["nchunks"] > 256 for r in rows)
    # (j) a head whose carried chain has stopped while the chain from `start` runs on through a later batch ...
    assert any(r["entry_absorbing"] and r["dual_absorbed_at"] is None and r["nchunks"] > 256 for r in heads)
    # ... a head that holds the keyword while the carried state never absorbed before it ...
    assert any(r["pname"] == "keywords" and not r["entry_absorbing"] and (r["dual_absorbed_at"] or 0) >= 256
               for r in heads)
    # ... and the chain from `start` stopped in the head's first chunk while the carried one runs on
    assert any(r["dual_absorbed_at"] == 0 and (r["absorbed_at"] is None or r["absorbed_at"] >= 256) and
               r["nchunks"] > 256 for r in heads)
    # a keyword cut by the fold: only the carried chain ever sees it
    assert any(r["pname"] == "keywords" and r["absorbed_at"] == 0 and not r["entry_absorbing"] and
               r["dual_absorbed_at"] is None for r in heads)
    # (k) a finish while carrying, beyond one register group
    assert any(r["kind"] == "finish" and r["nchunks"] > 64 for r in rows)


def test_scale_misses_are_what_the_design_says():
    """DESIGN 3.12's table: an automaton that converges within the lookback never misses. `error`, C3, the
    keywords, the count modulo 3 (one seed per memory class) and a[ab]{k}$ (256 bytes decide the state) miss
    zero times in every walk; the count modulo 7 misses. The Sheng pattern ^[a-j ]*error[a-j ]*$ misses zero times
    until the line has matched: its state behind `error` is neither absorbing nor what a seed reaches, so every
    chunk behind the hit is walked again."""
    for W, pname in _scale_pairs():
        rows = _scale_rows(W, pname)
        total = sum(r["misses"] for r in rows)
        if pname == "mod7":
            assert total > 0
        elif pname == "sheng":
            assert sum(r["misses"] for r in rows if "/miss/" in r["case"]) == 0
            for r in rows:
                if r["misses"]:
                    at = r["data"].index(b"error") if b"error" in r["data"] else -1
                    assert r["miss_chunks"][0] > at // r["chunk"] and "/hit/" in r["case"], r["case"]
            assert total > 0
        else:
            assert total == 0, (W, pname, [(r["case"], r["misses"]) for r in rows if r["misses"]])
