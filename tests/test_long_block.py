"""The chunked long-value path's host side (csrc/kernels/encode_long.h: the
block assembly clipped to the buffer's bytes, the block's widths and
expansions) under ASan + UBSan: tests/long_block_c/long_block_test is a
stand-alone program that runs a restatement of the two chunk passes over
buffers of exactly n bytes -- every address phase of the value's start and of
the buffer's end with values of 1..48 bytes over the edge alphabet, 16 KiB +- 17
at three phases, 2,000 seeded random values -- and compares the bytes with
json_body<true> (csrc/kernels/encode_common.h). A byte read outside the buffer
is a sanitizer report. Nothing is loaded into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "long_block_c")


def test_long_block_under_sanitizers():
    subprocess.run(["make", "-s", "-C", DIR], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(DIR, "long_block_test")], capture_output=True, timeout=300, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr.decode(errors="replace")[-3000:])
    assert b"AddressSanitizer" not in p.stderr and b"runtime error" not in p.stderr
    m = re.match(rb"OK (\d+) inputs\n", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) == 16 * 2 * 48 * 16 + 3 * 35 + 2000


def test_the_edge_alphabet_is_the_same_in_both_restatements():
    import window_part_cases as PC

    src = open(os.path.join(DIR, "long_block_test.cpp")).read()
    m = re.search(r"kEdge\[\] = \{(.*?)\};", src, re.S)
    assert bytes(int(x, 16) for x in re.findall(r"0x([0-9A-Fa-f]{2})", m.group(1))) == PC.EDGE_BYTES
