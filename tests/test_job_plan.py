"""The windowed job's host arithmetic (csrc/runtime/job_plan.h: the pack
planner, the routes, the arena's offsets, growth and the append kernel's
head / body / tail split) under ASan + UBSan: tests/job_c/job_plan_test is a
stand-alone program that drives the planner as the runtime does, with the pack
buffer, the arena and the segment table as heap buffers of exactly their
planned sizes, and compares them with a plain restatement."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "job_c")


def test_job_plan_under_sanitizers():
    subprocess.run(["make", "-s", "-C", DIR], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(DIR, "job_plan_test")], capture_output=True, timeout=300, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr.decode(errors="replace")[-3000:])
    assert b"AddressSanitizer" not in p.stderr and b"runtime error" not in p.stderr
    assert p.stdout.startswith(b"job_plan OK"), p.stdout
