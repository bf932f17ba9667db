"""The carry walk's host side (csrc/kernels/carry_plan.h: the chunk plan, the
absorbing states, the lookback seeds) under ASan + UBSan:
tests/carry_c/carry_plan_test is a stand-alone program that restates the two
kernels on exact-size heap buffers and compares the guess-and-fix walk of
random DFAs and ranges with the serial walk."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "carry_c")


def test_carry_plan_under_sanitizers():
    subprocess.run(["make", "-s", "-C", DIR], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(DIR, "carry_plan_test")], capture_output=True, timeout=300, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr.decode(errors="replace")[-3000:])
    assert b"AddressSanitizer" not in p.stderr and b"runtime error" not in p.stderr
    assert p.stdout.startswith(b"carry_plan OK"), p.stdout
