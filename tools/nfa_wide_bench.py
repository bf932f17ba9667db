"""Scan rate of an over-budget pattern whose NFA program is wider than one
lane's registers (more than 1024 rune-set positions): 120 `kwNNNa.*tailNNNb`
rules (1,800 positions) at the default state budget, over an HBM-resident
kind-0 synthetic log split with a few hundred matching lines and as many near
misses planted. Candidate lines are decided by verify_nfa_wave_kernel (one wave
per line). Next to it, the oracle on CPU threads over the same
bytes: what a user of this pattern had while the compile was refused. Every
record of the split is compared with the oracle's. Run on the GPU box:

    python tools/nfa_wide_bench.py [--gib 1] [--plants 300] [--threads 16]

Prints one JSON line.
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-grep_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

N_RULES = 120


def rule_set() -> bytes:
    return b"|".join(b"kw%03da.*tail%03db" % (i, i) for i in range(N_RULES))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--plants", type=int, default=300, help="matching lines planted (and as many near misses)")
    ap.add_argument("--seed", type=int, default=12)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16, help="oracle threads")
    args = ap.parse_args()

    import numpy as np
    import torch

    import dgrep
    import oracle_lib as O

    pattern = rule_set()
    t0 = time.perf_counter()
    cp = dgrep.CompiledPattern(pattern)
    compile_s = time.perf_counter() - t0
    assert cp.partial and cp.nfa_positions > 1024, (cp.flags, cp.nfa_positions)
    n = int(args.gib * (1 << 30))
    ctx = dgrep.Context(0)
    ctx.load(cp)
    buf = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    ctx.synth(buf.data_ptr(), n, args.seed, 0)
    # plants: "\n<prefix of rule i> zz <tail of rule j>\n" over the bytes at a
    # random offset (the line there is cut in two); i == j is a match
    rnd = random.Random(args.seed)
    slot = n // (2 * args.plants + 1)
    for k in range(2 * args.plants):
        i = rnd.randrange(N_RULES)
        j = i if k % 2 == 0 else (i + 1 + rnd.randrange(N_RULES - 1)) % N_RULES
        line = b"\nsvc %d kw%03da zz tail%03db end\n" % (k, i, j)
        at = k * slot + rnd.randrange(slot - len(line))
        buf[at:at + len(line)] = torch.frombuffer(bytearray(line), dtype=torch.uint8).cuda()
    cap = 1 << 16
    ln = torch.empty(cap, dtype=torch.int64, device="cuda")
    st = torch.empty(cap, dtype=torch.int64, device="cuda")
    le = torch.empty(cap, dtype=torch.int64, device="cuda")
    runs = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cnt = ctx.scan_device(buf.data_ptr(), n, ln.data_ptr(), st.data_ptr(), le.data_ptr(), cap)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        s = ctx.scan_stats()
        runs.append(dict(wall_ms=round(wall * 1e3, 3), scan_ms=round(s["scan_ms"], 3),
                         verify_ms=round(s["verify_ms"], 3), overflow_ms=round(s["overflow_ms"], 3),
                         candidates=s["candidates"], stepper=s["stepper"]))
    assert cnt <= cap, cnt
    best = min(runs[1:] or runs, key=lambda r: r["wall_ms"])  # the first run warms up
    host = buf[:n].cpu().numpy().tobytes()
    t0 = time.perf_counter()
    oln, ost, ole = O.grep_map(pattern, host, threads=args.threads)
    oracle_s = time.perf_counter() - t0
    same = (cnt == len(oln) and np.array_equal(ln[:cnt].cpu().numpy().astype(np.uint64), oln.astype(np.uint64))
            and np.array_equal(st[:cnt].cpu().numpy().astype(np.uint64), ost.astype(np.uint64))
            and np.array_equal(le[:cnt].cpu().numpy().astype(np.uint64), ole.astype(np.uint64)))
    print(json.dumps({
        "what": "over-budget pattern with a wide NFA program: filter scan + one wave per candidate line",
        "pattern": "%d rules kwNNNa.*tailNNNb" % N_RULES, "nfa_positions": cp.nfa_positions, "dfa_states": cp.nstates,
        "compile_s": round(compile_s, 2), "bytes": n, "planted_matches": args.plants, "records": cnt,
        "scan_gbs": round(n / (best["wall_ms"] * 1e-3) / 1e9, 2), "best": best, "runs": runs,
        "oracle_threads": args.threads, "oracle_s": round(oracle_s, 3),
        "oracle_gbs": round(n / oracle_s / 1e9, 3),
        "checked": "every record bit-exact vs the oracle over the whole split" if same else "MISMATCH",
        "build": dgrep.build_info()}), flush=True)
    ctx.close()
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
