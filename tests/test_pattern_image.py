"""The pattern images (csrc/runtime/pattern_image.h: the stepper choice, the
Sheng, table, pair and filter images, the whole DFA with its absorbing states,
seeds and default-row image) on the CPU, under ASan + UBSan:
tests/pattern_image_c/pattern_image_test is a stand-alone program, linked with
the pattern compiler, that builds the image of every pattern of
tests/golden/pattern_image_patterns.txt under every stepper choice and walks
it with a one-lane restatement of its stepper against the blob's own DFA.

tests/golden/pattern_images.txt holds its `print` output as recorded when the
builders had just moved out of the runtime, unedited, behind a transcription of
the old loader: every scalar and a CRC-32 of every buffer of every image. It
does not change."""
import os
import re
import subprocess

import pytest

import stepper_cells as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "pattern_image_c")
EXE = os.path.join(DIR, "pattern_image_test")
PATTERNS = os.path.join(ROOT, "tests", "golden", "pattern_image_patterns.txt")
GOLDEN = os.path.join(ROOT, "tests", "golden", "pattern_images.txt")
FORCES = ("0:0", "2:0", "3:0", "4:0", "4:3", "4:4", "4:64", "0:3")
KINDS = {0: "table", 1: "sheng", 3: "pair", 4: "filter"}


def _patterns():
    out = []
    with open(PATTERNS, encoding="utf-8") as f:
        for line in f:
            if not line.startswith("#"):
                name, budget, hit, pattern = line.rstrip("\n").split("\t")
                out.append((name, int(budget), hit, pattern))
    return out


@pytest.fixture(scope="module")
def run():
    """one pass of the driver over the patterns: its checks and its print lines"""
    subprocess.run(["make", "-s", "-C", DIR], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([EXE, "check-print"], capture_output=True, timeout=900, env=env)


def test_pattern_images_under_sanitizers(run):
    p = run
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr.decode(errors="replace")[-3000:])
    assert b"AddressSanitizer" not in p.stderr and b"runtime error" not in p.stderr
    last = p.stdout.decode().splitlines()[-1]
    m = re.fullmatch(r"pattern_image OK (\d+) built, (\d+) refused", last)
    assert m, last
    assert int(m.group(1)) + int(m.group(2)) == len(_patterns()) * len(FORCES)


def test_every_image_equals_the_recorded_one(run):
    """line by line: no scalar and no byte of any image differs from the builders as they were in the runtime"""
    got = run.stdout.decode().splitlines()[:-1]
    with open(GOLDEN, encoding="utf-8") as f:
        want = f.read().splitlines()
    assert len(got) == len(want) == len(_patterns()) * len(FORCES)
    for g, w in zip(got, want):
        assert g == w
    tags = [" ".join(w.split(" ")[:2]) for w in want]
    assert tags == ["%s %s" % (p[0], f) for p in _patterns() for f in FORCES]


def test_the_patterns_are_the_cells_the_bench_configs_and_a_partial_build():
    import bench
    import dgrep
    import random_pattern_cases as R

    pats = {name: (budget, hit, pattern) for name, budget, hit, pattern in _patterns()}
    for c in SC.CELLS:
        assert pats["cell:" + c.name] == (0, c.hit.decode(), c.pattern.decode())
    want = {bench.workload_pattern(wl) for wl in bench.WORKLOADS.values()}
    assert len(want) == 6 and {p for n, (_, _, p) in pats.items() if n.startswith("bench:")} == want
    assert pats["partial:budget3"][0] == R.PARTIAL_BUDGET
    for name, (budget, hit, pattern) in pats.items():
        if name.startswith("partial:"):
            assert dgrep.CompiledPattern(pattern.encode(), state_budget=budget).partial, name
    assert sum(1 for n in pats if n.startswith("small:")) >= 30


def test_the_sheng_limit_has_one_default():
    """the runtime names DGREP_SHENG_MAX_STATES with its other knobs; the stand-alone builder takes it from
    pattern_layout.h (the table row stride's two names are tied by a static_assert in scan_dfa.hip)"""
    layout = os.path.join(ROOT, "distributed-grep_amd", "csrc", "kernels", "pattern_layout.h")
    name = "DGREP_SHENG_MAX_STATES"
    assert SC.source_constant(SC.RUNTIME_HIP, name) == SC.source_constant(layout, name) == SC.limits()["sheng_max"]
    assert SC.source_constant(layout, "kTableRow") == SC.limits()["kRow"]


def _fields(line):
    f = dict(kv.split("=", 1) for kv in line.split(" crc ")[0].split(" ")[2:])
    return KINDS[int(f["kind"])], int(f["table"]), int(f["pair"].split(",")[3])


def _check_choice(line, want, S, lim):
    """the driver's stepper, entry width and image size against stepper_cells.choose()'s restatement"""
    stepper, nbytes, w32 = _fields(line)
    assert stepper == want["stepper"], (line, want)
    if stepper == "pair":
        assert ("u32" if w32 else "u16", nbytes) == (want["entry"], want["image"]), (line, want)
    elif stepper == "table":
        assert nbytes == (S * lim["kRow"] + 15) & ~15 and nbytes <= want["rows"] * lim["kRow"], (line, want)
    elif stepper == "sheng":
        assert nbytes == 256 * 8, line


def test_cells_get_the_stepper_the_restated_rule_gives():
    lim = SC.limits()
    with open(GOLDEN, encoding="utf-8") as f:
        lines = {" ".join(l.split(" ")[:2]): l for l in f.read().splitlines()}
    for c in SC.CELLS:
        _check_choice(lines["cell:%s %s" % (c.name, "2:0" if c.force == "table" else "0:0")], c.expected, c.S, lim)
    refused = SC.REFUSED
    assert SC.choose(refused.S, refused.K, refused.S, "table", lim) == refused.expected
    assert lines["cell:filter-257 2:0"].endswith(" refused 2 dgrep_load_dfa: a DFA of 257 states needs the filter stepper")


def test_random_patterns_get_the_stepper_the_restated_rule_gives(tmp_path):
    import random_pattern_cases as R

    sel = R.selected()
    path = tmp_path / "random_patterns.txt"
    with open(path, "wb") as f:
        for c in sel:
            assert b"\t" not in c.pattern and b"\n" not in c.pattern and not c.pattern.startswith(b"#"), c.pattern
            f.write(c.name.encode() + b"\t0\t\t" + c.pattern + b"\n")
    subprocess.run(["make", "-s", "-C", DIR], check=True, capture_output=True)
    p = subprocess.run([EXE, "print-auto", str(path)], capture_output=True, timeout=900)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr.decode(errors="replace")[-3000:])
    got = p.stdout.decode().splitlines()
    assert len(got) == len(sel)
    lim = SC.limits()
    steppers = set()
    for line, c in zip(got, sel):
        assert line.startswith(c.name + " 0:0 kind="), line
        cp = R.compiled(c.pattern)
        want = R.auto_choice(cp)
        _check_choice(line, want, cp.nstates, lim)
        fits = R.pair_fits(cp)
        assert (want["stepper"] == "pair") == (cp.nstates > lim["sheng_max"] and fits is not None), c.name
        steppers.add(want["stepper"])
    assert steppers == {"sheng", "pair", "table", "filter"}
