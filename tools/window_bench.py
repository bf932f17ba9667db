"""Windowed scan against the resident one: a host split too large to want in
HBM whole. Corpus kind 0 (dgrep_synth_corpus, seed 1), pattern `error`. Not
the bench metric (that one is bench.py). Run on the GPU box:

    python tools/window_bench.py [--split 4G] [--windows 64M,256M,1G] [--big 8G@256M] [--reps 3]
                                 [--out profiles/r11/window/window_bench.jsonl]

One process, one GPU. Every figure is host wall time around one call, host
bytes in, host records out (end to end: ingest, scan, result copy):

  resident   dgrep_scan of the whole split, run --reps times TWICE (two series
             in the same process): the run-to-run spread the windowed figures
             are read against.
  windowed   dgrep_scan_windowed at each window size, --reps times.
  big        one larger split at one window, windowed only: the footprint line.

cut_ms (the cut passes' device time, HIP events) and data_bytes (the two
window buffers) come from one more, untimed run of the same bytes through
dgrep_stream_open / _feed(whole) / _finish, which is what dgrep_scan_windowed
does; the windowed records are compared with the resident ones before anything
is timed.
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


def size(s):
    s = s.upper()
    return int(s[:-1]) * UNITS[s[-1]] if s[-1] in UNITS else int(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--split", default="4G")
    ap.add_argument("--windows", default="64M,256M,1G")
    ap.add_argument("--big", default="8G@256M", help="SPLIT@WINDOW of the footprint line ('' to skip)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pattern", default="error")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import dgrep

    assert torch.cuda.is_available(), "window_bench.py needs a GPU"
    L = dgrep.lib()
    ctx = dgrep.Context(0)
    ctx.load(args.pattern)
    n = size(args.split)
    big_n, big_w = (size(x) for x in args.big.split("@")) if args.big else (0, 0)

    # the corpus is generated on the device and copied out: the host split is what the calls are given
    total = max(n, big_n)
    dev = torch.empty(total, dtype=torch.uint8, device="cuda:0")
    ctx.synth(dev.data_ptr(), total, 1, 0)
    host = dev.cpu().numpy()
    del dev
    torch.cuda.empty_cache()
    ptr = ctypes.c_void_p(host.ctypes.data)

    def emit(rec):
        rec["build"] = dgrep.build_info()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def resident(nbytes):
        res = dgrep._Result()
        t0 = time.perf_counter()
        ctx._check(L.dgrep_scan(ctx._h, ptr, nbytes, ctypes.byref(res)))
        dt = time.perf_counter() - t0
        out = [np.ctypeslib.as_array(p, shape=(int(res.count),)).copy() for p in (res.line_no, res.start, res.len)]
        L.dgrep_result_free(ctypes.byref(res))
        return dt, out

    def windowed(nbytes, w):
        res = dgrep._Result()
        t0 = time.perf_counter()
        ctx._check(L.dgrep_scan_windowed(ctx._h, ptr, nbytes, w, ctypes.byref(res)))
        dt = time.perf_counter() - t0
        out = [np.ctypeslib.as_array(p, shape=(int(res.count),)).copy() for p in (res.line_no, res.start, res.len)]
        L.dgrep_result_free(ctypes.byref(res))
        return dt, out

    def stream_stats(nbytes, w):
        with ctx.stream(w) as st:
            res = dgrep._StreamResult()
            ctx._check(L.dgrep_stream_feed(st._h, ptr, nbytes, ctypes.byref(res)))
            L.dgrep_stream_result_free(ctypes.byref(res))
            peak = st.stats()["data_bytes"]
            st.finish()
            s = st.stats()
        s["data_bytes"] = max(peak, s["data_bytes"])
        return s

    def series(fn, *a):
        fn(*a)  # warm-up: buffers and the staging ring are allocated
        return [fn(*a)[0] for _ in range(args.reps)]

    def gbps(nbytes, ts):
        return round(nbytes / statistics.median(ts) / 1e9, 3)

    windows = [size(w) for w in args.windows.split(",")]
    _, want = resident(n)
    for w in windows:
        _, got = windowed(n, w)
        for g, x in zip(got, want):
            assert np.array_equal(g, x), "windowed records differ from resident at window %d" % w

    a = series(resident, n)
    b = series(resident, n)
    ma, mb = statistics.median(a), statistics.median(b)
    spread = abs(ma - mb) / min(ma, mb)
    emit({"form": "resident", "split": n, "records": len(want[0]), "s_a": a, "s_b": b,
          "gbps_a": gbps(n, a), "gbps_b": gbps(n, b), "spread": round(spread, 4),
          "rep_spread": round((max(a + b) - min(a + b)) / statistics.median(a + b), 4)})
    for w in windows:
        t = series(windowed, n, w)
        st = stream_stats(n, w)
        emit({"form": "windowed", "split": n, "window": w, "s": t, "gbps": gbps(n, t),
              "vs_resident": round(statistics.median(t) / min(ma, mb), 4), "cut_ms": round(st["cut_ms"], 3),
              "data_bytes": st["data_bytes"], "windows": st["windows"], "max_carry": st["max_carry"]})
    if big_n:
        t = series(windowed, big_n, big_w)
        st = stream_stats(big_n, big_w)
        emit({"form": "windowed_big", "split": big_n, "window": big_w, "s": t, "gbps": gbps(big_n, t),
              "cut_ms": round(st["cut_ms"], 3), "data_bytes": st["data_bytes"], "windows": st["windows"],
              "max_carry": st["max_carry"]})
    ctx.close()


if __name__ == "__main__":
    main()
