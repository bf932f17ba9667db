"""Bounded windowed scan against the plain windowed one and the resident one, on
a host split that opens with one newline-free line of 1 GiB (corpus kind 3,
dgrep_synth_corpus, seed 3). Not the bench metric (that one is bench.py). Run
on the GPU box:

    python tools/carry_bench.py [--split 4G] [--window 256M] [--reps 3] [--patterns error,c3,c4]
                                [--out profiles/r12/carry/carry_bench.jsonl]

One process, one GPU. Every timing is host wall time around one call, host
bytes in, host records out (end to end: ingest, scan, result copy). Per
pattern the three forms are checked to return equal records, warmed once, and
then timed in turns (resident, windowed, bounded, resident, ...), --reps each:

  resident   dgrep_scan of the whole split; its verify_ms is the existing
             long-line resolution of the same 1 GiB line.
  windowed   dgrep_scan_windowed: the window buffers grow past the 1 GiB line.
  bounded    dgrep_scan_bounded: the line is folded into its DFA state.

data_bytes (the two window buffers, at their largest after a feed or the
finish) and the carry counters come from one more, untimed run of the same
bytes through dgrep_stream_open / _feed(whole) / _finish, which is what the
one-shots do.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-grep_amd"))

UNITS = {"K": 1 << 10, "M": 1 << 20, "G": 1 << 30}
C3 = "^[0-9]{4}-[0-9]{2}.*(WARN|ERROR) [a-z_]+"


def size(s):
    s = s.upper()
    return int(s[:-1]) * UNITS[s[-1]] if s[-1] in UNITS else int(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--split", default="4G")
    ap.add_argument("--window", default="256M")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--patterns", default="error,c3,c4")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import dgrep

    assert torch.cuda.is_available(), "carry_bench.py needs a GPU"
    L = dgrep.lib()
    ctx = dgrep.Context(0)
    n, w = size(args.split), size(args.window)
    patterns = {"error": "error", "c3": C3,
                "c4": "(?i)(" + "|".join(k.decode() for k in dgrep.synth_keywords(4, 1000)) + ")"}

    # the corpus is generated on the device and copied out: the host split is what the calls are given
    dev = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    ctx.synth(dev.data_ptr(), n, 3, 3)
    host = dev.cpu().numpy()
    del dev
    torch.cuda.empty_cache()
    ptr = ctypes.c_void_p(host.ctypes.data)
    first_nl = n
    for o in range(0, n, 1 << 28):  # in pieces: no split-sized temporary
        hit = np.flatnonzero(host[o:o + (1 << 28)] == 0x0A)
        if hit.size:
            first_nl = o + int(hit[0])
            break
    assert (1 << 30) <= first_nl < n, "kind 3 opens with a newline-free GiB"

    def emit(rec):
        rec["build"] = dgrep.build_info()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def one_shot(call, *extra):
        def run():
            res = dgrep._Result()
            t0 = time.perf_counter()
            ctx._check(call(ctx._h, ptr, n, *extra, ctypes.byref(res)))
            dt = time.perf_counter() - t0
            out = [np.ctypeslib.as_array(p, shape=(int(res.count),)).copy() if res.count else np.zeros(0, np.uint64)
                   for p in (res.line_no, res.start, res.len)]
            L.dgrep_result_free(ctypes.byref(res))
            return dt, out, ctx.scan_stats()
        return run

    forms = [("resident", one_shot(L.dgrep_scan)), ("windowed", one_shot(L.dgrep_scan_windowed, w)),
             ("bounded", one_shot(L.dgrep_scan_bounded, w))]

    def stream_stats(bounded):
        with ctx.stream(w, bounded=bounded) as st:
            res = dgrep._StreamResult()
            ctx._check(L.dgrep_stream_feed(st._h, ptr, n, ctypes.byref(res)))
            L.dgrep_stream_result_free(ctypes.byref(res))
            peak = st.stats()["data_bytes"]
            st.finish()
            s = dict(st.stats(), **st.carry_stats())
        s["data_bytes"] = max(peak, s["data_bytes"])
        return s

    for name in args.patterns.split(","):
        ctx.load(patterns[name])
        # equal records first (this is the warm-up too: buffers and the staging ring are allocated)
        want = None
        for form, run in forms:
            _, got, _ = run()
            if want is None:
                want = got
            for g, x in zip(got, want):
                assert np.array_equal(g, x), "%s: %s records differ from resident" % (name, form)
        times = {form: [] for form, _ in forms}
        stats = {}
        for _ in range(args.reps):  # in turns, so that a drift of the box falls on all three
            for form, run in forms:
                dt, _, st = run()
                times[form].append(dt)
                stats[form] = st
        base = statistics.median(times["resident"])
        for form, _ in forms:
            t = statistics.median(times[form])
            rec = {"pattern": name, "form": form, "split": n, "first_line": first_nl, "records": len(want[0]),
                   "s": times[form], "ms": round(t * 1e3, 2), "gbps": round(n / t / 1e9, 3),
                   "vs_resident": round(t / base, 4), "stepper": stats[form]["stepper"],
                   "verify_ms": round(stats[form]["verify_ms"], 3)}
            if form != "resident":
                st = stream_stats(form == "bounded")
                rec.update(window=w, data_bytes=st["data_bytes"], windows=st["windows"], max_carry=st["max_carry"],
                           cut_ms=round(st["cut_ms"], 3), folds=st["folds"], folded_bytes=st["folded_bytes"],
                           chunks=st["chunks"], guess_misses=st["guess_misses"], walk_ms=round(st["walk_ms"], 3))
            else:
                rec["data_bytes"] = n  # the whole split is resident
            emit(rec)
    ctx.close()


if __name__ == "__main__":
    main()
