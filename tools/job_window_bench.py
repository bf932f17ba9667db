"""The windowed whole job against the resident one. Not the bench metric (that
one is bench.py). Run on the GPU box:

    python tools/job_window_bench.py [--total 4G] [--windows 64M,256M,1G] [--shapes one,64,small]
                                     [--small 256K] [--reps 3] [--out profiles/r15/job_window/FILE.jsonl]

One process, one GPU. A kind-0 host corpus (dgrep_synth_corpus, seed 1) of
--total bytes, pattern `error`, nreduce 10, cut into files three ways:

  one    1 file
  64     64 files of total / 64 bytes
  small  files of --small bytes (256 KiB: 16,384 of them in 4 GiB)

For each shape the forms are the resident dgrep_grep_job and the windowed job
(dgrep_job_open / dgrep_job_add per file / dgrep_job_finish) at each window. The
outputs of every form are compared with the resident job's before anything is
timed. Then the forms are run alternately, --reps + 1 rounds; the first round
is the warm-up and every figure is the median of the others. Times are host
wall time end to end: host bytes in, every mr-out-<r> on the host out. The
windowed lines carry dgrep_job_stats_get's legs (device ms of scan, encode,
append and reduce), its counts and the device bytes of the arena and the
window buffers.

Shape `small` also gets one partition stream per file
(dgrep_map_partitions_windowed, window = the smallest of --windows) over every
64th file, which is what a caller without the pack route would do; its time
times 64 is what the pack route has to beat.
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
R = 10


def size(s):
    s = s.upper()
    return int(s[:-1]) * UNITS[s[-1]] if s[-1] in UNITS else int(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--total", default="4G")
    ap.add_argument("--windows", default="64M,256M,1G")
    ap.add_argument("--shapes", default="one,64,small")
    ap.add_argument("--small", default="256K")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch

    import dgrep

    assert torch.cuda.is_available(), "job_window_bench.py needs a GPU"
    L = dgrep.lib()
    ctx = dgrep.Context(0)

    def emit(rec):
        rec["build"] = dgrep.build_info()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    n = size(args.total)
    windows = [size(w) for w in args.windows.split(",")]
    ctx.load("error")
    dev = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    ctx.synth(dev.data_ptr(), n, 1, 0)
    host = dev.cpu().numpy()
    del dev
    torch.cuda.empty_cache()
    base = host.ctypes.data

    def files_of(piece):
        """(offsets, lengths, names) of the corpus cut every `piece` bytes"""
        offs = list(range(0, n, piece))
        lens = [min(piece, n - o) for o in offs]
        names = [b"in/pg-%06d.txt" % i for i in range(len(offs))]
        return offs, lens, names

    def take(res):
        raw = ctypes.string_at(res.bytes, res.total) if res.total else b""
        off = [res.part_off[p] for p in range(R + 1)]
        lines = [res.lines_in[p] for p in range(R)]
        L.dgrep_reduce_batch_free(ctypes.byref(res))
        return [raw[off[p]:off[p + 1]] for p in range(R)], lines

    def arrays(offs, lens, names):
        k = len(offs)
        return ((ctypes.c_void_p * k)(*[base + o for o in offs]), (ctypes.c_size_t * k)(*lens),
                (ctypes.c_char_p * k)(*names), (ctypes.c_size_t * k)(*[len(f) for f in names]))

    def resident(arr, k):
        """(seconds, legs, outputs)"""
        res = dgrep._ReduceBatchOut()
        t0 = time.perf_counter()
        ctx._check(L.dgrep_grep_job(ctx._h, arr[0], arr[1], arr[2], arr[3], k, R, ctypes.byref(res)))
        dt = time.perf_counter() - t0
        legs = {"scan_ms": round(ctx.last_kernel_ms(), 3), "encode_ms": round(ctx.last_encode_ms(), 3),
                "reduce_ms": round(ctx.last_reduce_ms(), 3)}
        return dt, legs, take(res)

    def windowed(offs, lens, names, w):
        """(seconds, dgrep_job_stats_get, outputs)"""
        res = dgrep._ReduceBatchOut()
        st = dgrep._JobStats()
        j = ctypes.c_void_p()
        t0 = time.perf_counter()
        ctx._check(L.dgrep_job_open(ctx._h, w, R, ctypes.byref(j)))
        try:
            for o, m, f in zip(offs, lens, names):
                ctx._check(L.dgrep_job_add(j, ctypes.c_void_p(base + o), m, f, len(f)))
            ctx._check(L.dgrep_job_finish(j, ctypes.byref(res)))
            dt = time.perf_counter() - t0
            ctx._check(L.dgrep_job_stats_get(j, ctypes.byref(st), ctypes.sizeof(st)))
        finally:
            L.dgrep_job_close(j)
        stats = {f: (round(getattr(st, f), 3) if f.endswith("_ms") else getattr(st, f)) for f, _ in st._fields_}
        return dt, stats, take(res)

    def streams(offs, lens, names, w):
        """one partition stream per file: seconds for all of them"""
        t0 = time.perf_counter()
        for o, m, f in zip(offs, lens, names):
            res = dgrep._BatchPartitions()
            ctx._check(L.dgrep_map_partitions_windowed(ctx._h, ctypes.c_void_p(base + o), m, w, f, len(f), R,
                                                       ctypes.byref(res)))
            L.dgrep_batch_partitions_free(ctypes.byref(res))
        return time.perf_counter() - t0

    pieces = {"one": n, "64": (n + 63) // 64, "small": size(args.small)}
    for shape in args.shapes.split(","):
        offs, lens, names = files_of(pieces[shape])
        k = len(offs)
        arr = arrays(offs, lens, names)
        _, _, want = resident(arr, k)
        for w in windows:
            assert windowed(offs, lens, names, w)[2] == want, "windowed job differs from resident at window %d" % w
        runs = {"resident": []}
        runs.update({w: [] for w in windows})
        for rep in range(args.reps + 1):  # the forms alternate; round 0 is the warm-up
            dt, legs, _ = resident(arr, k)
            runs["resident"].append((dt, legs))
            for w in windows:
                dt, stats, _ = windowed(offs, lens, names, w)
                runs[w].append((dt, stats))
        med = lambda rs: statistics.median(r[0] for r in rs[1:])
        t_res = med(runs["resident"])
        common = {"shape": shape, "files": k, "total": n, "out_bytes": sum(map(len, want[0])), "lines": sum(want[1])}
        emit(dict(common, form="resident", s=[round(r[0], 4) for r in runs["resident"][1:]],
                  gbps=round(n / t_res / 1e9, 3), legs=runs["resident"][-1][1]))
        for w in windows:
            t = med(runs[w])
            emit(dict(common, form="windowed", window=w, s=[round(r[0], 4) for r in runs[w][1:]],
                      gbps=round(n / t / 1e9, 3), vs_resident=round(t / t_res, 4), stats=runs[w][-1][1]))
        if shape == "small":
            w = min(windows)
            sample = (offs[::64], lens[::64], names[::64])
            ts = [streams(*sample, w) for _ in range(args.reps + 1)][1:]
            t = statistics.median(ts)
            emit(dict(common, form="stream_per_file", window=w, sample_files=len(sample[0]),
                      s=[round(x, 4) for x in ts], s_per_file=round(t / len(sample[0]), 6),
                      s_times_64=round(t * 64, 3)))
    ctx.close()


if __name__ == "__main__":
    main()
