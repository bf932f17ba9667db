"""The windowed partition writer against the resident one, and its long-value
path against the one-lane path. Not the bench metric (that one is bench.py). Run
on the GPU box:

    python tools/window_part_bench.py split [--split 4G] [--windows 64M,256M,1G]
    python tools/window_part_bench.py line  [--line 64M] [--window 256M]
    python tools/window_part_bench.py sweep [--sizes 256,1K,4K,16K,64K,256K,1M,4M,16M]
    python tools/window_part_bench.py many  [--sizes 256,512,1K,2K,4K,8K,16K,64K] [--total 16M]
                                      [--reps 3] [--out profiles/r13/window_part/FILE.jsonl]

One process, one GPU. Every figure is the median of --reps runs after one
warm-up, and the outputs are compared before anything is timed.

  split  a kind-0 host split (dgrep_synth_corpus, seed 1), `error`, nreduce 10:
         dgrep_map_partitions (resident) against dgrep_map_partitions_windowed
         at each window. End to end host wall time (host bytes in, host bytes
         out), the encoder's device time (dgrep_last_encode_ms: for the windowed
         form the sum over the windows) and the device bytes of the window
         buffers and of the encoded-bytes buffer.
  line   one line of --line bytes with a '"' every 8 bytes, between short lines,
         pattern `` (every line): the resident writer's encode (one lane measures
         the line, one lane writes it) against the windowed writer's (the line
         cut into chunks, a workgroup each) at --window.
  sweep  one escaped value ('"' every 8 bytes) per size, forced onto each path
         of the WINDOW encoder with dgrep_set_long_value (256: the chunked path;
         2^30: the one-lane path). The crossover is the smallest size from
         which the chunked path is faster.
  many   the same, with --total bytes of such values in one window instead of
         one value alone: the one-lane path then runs a lane per value side by
         side, which is what the default of dgrep_set_long_value has to beat.

The windowed encode times come from a partition stream that is fed the same
bytes again and again: the first feed sizes the stream's buffers (and encodes
twice to do so), the timed ones encode once, as the steady state of a long
stream does.
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
FILENAME = b"pg-big.txt"
R = 10


def size(s):
    s = s.upper()
    return int(s[:-1]) * UNITS[s[-1]] if s[-1] in UNITS else int(s)


def window_for(n):
    return max(4096, (n + 8192 + 4095) // 4096 * 4096)


def escaped_value(n):
    return (b'abcdefg"' * (n // 8 + 1))[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["split", "line", "sweep", "many"])
    ap.add_argument("--split", default="4G")
    ap.add_argument("--windows", default="64M,256M,1G")
    ap.add_argument("--line", default="64M")
    ap.add_argument("--window", default="256M")
    ap.add_argument("--sizes", default="", help="default: 256 .. 16M (sweep), 256 .. 64K (many)")
    ap.add_argument("--total", default="16M")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import dgrep

    assert torch.cuda.is_available(), "window_part_bench.py needs a GPU"
    L = dgrep.lib()
    ctx = dgrep.Context(0)

    def emit(rec):
        rec["lib"] = os.path.basename(dgrep.LIB_PATH)  # DGREP_LIB: a build with another DGREP_LONG_CHUNK
        rec["build"] = dgrep.build_info()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def med(xs):
        return round(statistics.median(xs), 4)

    def resident(ptr, n):
        """(seconds end to end, encode ms, the partitions)"""
        res = dgrep._Partitions()
        t0 = time.perf_counter()
        ctx._check(L.dgrep_map_partitions(ctx._h, ptr, n, FILENAME, len(FILENAME), R, ctypes.byref(res)))
        dt = time.perf_counter() - t0
        raw = ctypes.string_at(res.bytes, res.total) if res.total else b""
        parts = [raw[res.begin[p]:res.end[p]] for p in range(R)]
        L.dgrep_partitions_free(ctypes.byref(res))
        return dt, ctx.last_encode_ms(), parts

    def windowed(ptr, n, w):
        res = dgrep._BatchPartitions()
        t0 = time.perf_counter()
        ctx._check(L.dgrep_map_partitions_windowed(ctx._h, ptr, n, w, FILENAME, len(FILENAME), R, ctypes.byref(res)))
        dt = time.perf_counter() - t0
        enc = ctx.last_encode_ms()
        rows = dgrep._take_rows(L, res)
        return dt, enc, [b"".join(r[p] for r in rows) for p in range(R)]

    def stream_encode(ptr, n, w, want=None):
        """the per-feed encode ms of a stream fed the same bytes 1 + reps times (they end in '\\n'); its stats"""
        ms = []
        with ctx.partition_stream(w, FILENAME, R) as st:
            for k in range(args.reps + 1):
                res = dgrep._BatchPartitions()
                ctx._check(L.dgrep_stream_feed_partitions(st._h, ptr, n, ctypes.byref(res)))
                if k:
                    ms.append(ctx.last_encode_ms())
                elif want is not None:
                    rows = dgrep._take_rows(L, res)
                    res = None
                    got = [b"".join(r[p] for r in rows) for p in range(R)]
                    assert got == want, "the windowed bytes differ from the resident ones"
                if res is not None:
                    L.dgrep_batch_partitions_free(ctypes.byref(res))
            stats = st.stats()
        return ms, stats

    if args.mode == "split":
        ctx.load("error")
        n = size(args.split)
        dev = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        ctx.synth(dev.data_ptr(), n, 1, 0)
        host = dev.cpu().numpy()
        del dev
        torch.cuda.empty_cache()
        ptr = ctypes.c_void_p(host.ctypes.data)
        windows = [size(w) for w in args.windows.split(",")]
        _, _, want = resident(ptr, n)
        for w in windows:
            assert windowed(ptr, n, w)[2] == want, "windowed bytes differ from resident at window %d" % w
        runs = [resident(ptr, n)[:2] for _ in range(args.reps + 1)][1:]
        base = statistics.median(r[0] for r in runs)
        emit({"mode": "split", "form": "resident", "split": n, "out_bytes": sum(map(len, want)),
              "s": [round(r[0], 4) for r in runs], "gbps": round(n / base / 1e9, 3),
              "encode_ms": med([r[1] for r in runs]), "device_bytes": n})
        for w in windows:
            runs = [windowed(ptr, n, w)[:2] for _ in range(args.reps + 1)][1:]
            with ctx.partition_stream(w, FILENAME, R) as st:
                res = dgrep._BatchPartitions()
                ctx._check(L.dgrep_stream_feed_partitions(st._h, ptr, n, ctypes.byref(res)))
                L.dgrep_batch_partitions_free(ctypes.byref(res))
                stats = st.stats()
            t = statistics.median(r[0] for r in runs)
            emit({"mode": "split", "form": "windowed", "split": n, "window": w, "s": [round(r[0], 4) for r in runs],
                  "gbps": round(n / t / 1e9, 3), "vs_resident": round(t / base, 4),
                  "encode_ms_sum": med([r[1] for r in runs]), "rows": stats["rows"], "windows": stats["windows"],
                  "data_bytes": stats["data_bytes"], "enc_device_bytes": stats["enc_device_bytes"],
                  "cut_ms": round(stats["cut_ms"], 3)})
    elif args.mode == "line":
        ctx.load("")
        n, w = size(args.line), size(args.window)
        data = b"a short line\n" * 100 + escaped_value(n) + b"\n" + b"another short line\n" * 100
        host = np.frombuffer(data, dtype=np.uint8)
        ptr = ctypes.c_void_p(host.ctypes.data)
        _, _, want = resident(ptr, len(data) - 1)  # a feed completes the lines up to the last '\n'; the empty one behind it is the finish's
        res_ms = [resident(ptr, len(data))[1] for _ in range(args.reps)]
        win_ms, stats = stream_encode(ptr, len(data), w, want)
        assert stats["long_values"] == args.reps + 1, stats
        emit({"mode": "line", "line": n, "window": w, "resident_encode_ms": med(res_ms), "resident_ms": res_ms,
              "windowed_encode_ms": med(win_ms), "windowed_ms": win_ms,
              "factor": round(statistics.median(res_ms) / statistics.median(win_ms), 2),
              "enc_device_bytes": stats["enc_device_bytes"]})
    else:
        ctx.load("")
        sizes = args.sizes or ("256,1K,4K,16K,64K,256K,1M,4M,16M" if args.mode == "sweep" else
                               "256,512,1K,2K,4K,8K,16K,64K")
        for n in (size(x) for x in sizes.split(",")):
            copies = max(1, size(args.total) // (n + 1)) if args.mode == "many" else 1
            data = b"a short line\n" + (escaped_value(n) + b"\n") * copies
            host = np.frombuffer(data, dtype=np.uint8)
            ptr = ctypes.c_void_p(host.ctypes.data)
            w = window_for(len(data))
            _, _, want = resident(ptr, len(data) - 1)  # without the empty last line, which is the finish's
            rec = {"mode": args.mode, "value": n, "values": copies, "window": w}
            for name, lv in (("chunked", 256), ("one_lane", 1 << 30)):
                ctx.set_long_value(lv)
                ms, stats = stream_encode(ptr, len(data), w, want)
                assert stats["long_values"] == ((args.reps + 1) * copies if lv == 256 else 0), stats
                rec[name + "_ms"] = med(ms)
                rec[name + "_all"] = [round(x, 4) for x in ms]
            ctx.set_long_value(0)
            rec["chunked_over_one_lane"] = round(rec["chunked_ms"] / rec["one_lane_ms"], 3)
            emit(rec)
    ctx.close()


if __name__ == "__main__":
    main()
