"""The packing ingest's separator-less mode (pack_piece_segments(..., sep =
false), which lays the batch reduce's inputs back to back) under ASan + UBSan:
tests/pack_nosep_c/pack_nosep_test is a stand-alone program that assembles the
inputs piece by piece (1, 7 and 4096 bytes) into exact-size heap buffers and
compares them with the plain concatenation."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "pack_nosep_c")


def test_pack_pieces_without_separators_under_sanitizers():
    subprocess.run(["make", "-s", "-C", DIR], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(DIR, "pack_nosep_test")], capture_output=True, timeout=300, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr.decode(errors="replace")[-3000:])
    assert b"AddressSanitizer" not in p.stderr and b"runtime error" not in p.stderr
    assert p.stdout.startswith(b"pack_nosep OK"), p.stdout
