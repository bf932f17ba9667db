"""The long-value escaper's host side (csrc/kernels/escape_width.h: the local
width rule) under ASan + UBSan: tests/escape_c/escape_width_test is a
stand-alone program that, for all strings of 1 and 2 bytes, all strings of 3 and
4 bytes over the edge alphabet and 2,000 seeded random strings, compares the sum
of the widths with json_body<false> and the bytes written at the widths' prefix
offsets with json_body<true> (csrc/kernels/encode_common.h). Nothing is loaded
into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "escape_c")


def test_escape_width_under_sanitizers():
    subprocess.run(["make", "-s", "-C", DIR], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(DIR, "escape_width_test")], capture_output=True, timeout=300, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr.decode(errors="replace")[-3000:])
    assert b"AddressSanitizer" not in p.stderr and b"runtime error" not in p.stderr
    m = re.match(rb"OK (\d+) inputs\n", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) == 256 + 256 * 256 + 23 ** 3 + 23 ** 4 + 2000 + 1


def test_the_edge_alphabet_is_the_same_in_both_restatements():
    import window_part_cases as PC

    src = open(os.path.join(DIR, "escape_width_test.cpp")).read()
    m = re.search(r"kEdge\[\] = \{(.*?)\};", src, re.S)
    assert bytes(int(x, 16) for x in re.findall(r"0x([0-9A-Fa-f]{2})", m.group(1))) == PC.EDGE_BYTES
