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


# ---- the Python restatement (tests/carry_cases.py) against the C++ ------------------
# the inputs of `carry_plan_test print`, written out as they are in carry_plan_test.cpp
PRINT_M = [0, 1, 255, 256, 257, 4095, 4096, 4097, 16383, 16384, 65535, 65536, 65537, 131071, 131072, 131073, 262143,
           262144, 262145, 524289, 1048575, 1048576, 1048577, 2097151, 2097152, 2097153, 268435456, (1 << 32) + 1,
           1 << 40]
PRINT_CUS = [0, 1, 4, 256, 304]
TABLE_A = [[1, 0, 2], [1, 0, 1], [2, 5, 2], [3, 3, 3], [4, 0, 4], [0, 1, 2]]
TABLE_B = [[0, 3], [1, 1], [2, 0], [3, 4], [5, 0], [5, 5], [6, 1], [7, 2], [1, 8]]


def _expected_print():
    import carry_cases as CC

    out = []
    for m in PRINT_M:
        for cus in PRINT_CUS:
            for lds in (1, 0):
                lanes = CC.carry_lanes(m, cus, bool(lds))
                out.append("plan %d %d %d: %d %d %d" % ((m, cus, lds, lanes) + CC.carry_plan(m, lanes)))
    for lanes in (0, 1, 3, 64):
        out.append("lanes %d: %d %d" % ((lanes,) + CC.carry_plan(100000, lanes)))
    for name, table in (("A", TABLE_A), ("B", TABLE_B)):
        S, K = len(table), len(table[0])
        flat = [x for row in table for x in row]
        a = CC.carry_absorbing(flat, S, K, 1)
        out.append("absorbing %s %s" % (name, " ".join(map(str, a))))
        for start in range(S):
            out.append("seeds %s %d: %d %d %d %d" % ((name, start) + tuple(CC.carry_seeds(a, S, start))))
        for n in (1, 2, 3):
            small = [x % n for row in table[:n] for x in row]
            sa = CC.carry_absorbing(small, n, K, 1)
            out.append("small %s %d: %s : %d %d %d %d" % ((name, n, " ".join(map(str, sa))) +
                                                          tuple(CC.carry_seeds(sa, n, n - 1))))
    return out


def test_python_model_equals_carry_plan_h():
    """carry_lanes, carry_plan, carry_absorbing and carry_seeds of tests/carry_cases.py give what the header gives,
    line for line; nothing is loaded into Python"""
    subprocess.run(["make", "-s", "-C", DIR], check=True, capture_output=True)
    p = subprocess.run([os.path.join(DIR, "carry_plan_test"), "print"], capture_output=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr.decode(errors="replace")[-3000:])
    got, want = p.stdout.decode().splitlines(), _expected_print()
    assert len(got) == len(want) == len(PRINT_M) * len(PRINT_CUS) * 2 + 4 + 2 * (1 + 3) + 6 + 9
    for g, w in zip(got, want):
        assert g == w, (g, w)
    # the tables do hold what the seeds must step over: absorbing states, also at a spread id, and a taken one
    import carry_cases as CC
    a = CC.carry_absorbing([x for row in TABLE_B for x in row], 9, 2, 1)
    assert a == [1, 1, 1, 1, 0, 1, 1, 1, 0] and CC.carry_seeds(a, 9, 4) == [4, 8, 4, 4]
    assert CC.carry_absorbing([x for row in TABLE_A for x in row], 6, 3, 1) == [0, 1, 1, 1, 1, 0]


def test_plans_at_the_scale_windows():
    """the plans of a 256-CU device at the sizes the scale cases are built around (tests/carry_cases.py)"""
    import carry_cases as CC

    for lds, m, plan in ((True, 65536, (256, 256)), (True, 65537, (256, 257)), (True, 131072, (256, 512)),
                         (True, 131073, (512, 257)), (True, 262143, (512, 512)), (True, 1048576, (1024, 1024)),
                         (True, 1048577, (1024, 1025)), (True, 2097151, (1024, 2048)), (False, 131073, (256, 513)),
                         (False, 262143, (256, 1024))):
        assert CC.carry_plan(m, CC.carry_lanes(m, 256, lds)) == plan, (lds, m)
    assert CC.rows_in_lds(8, 6) and CC.rows_in_lds(17, 13) and CC.rows_in_lds(4096, 4)
    assert not CC.rows_in_lds(4097, 4) and not CC.rows_in_lds(8193, 4) and not CC.rows_in_lds(131073, 4)
    assert CC.rows_in_lds(65535, 0) and not CC.rows_in_lds(65536, 1) and CC.rows_in_lds(1, 8192)
