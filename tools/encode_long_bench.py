"""Long escaped values through the resident and the batch partition writer: the
chunked path (encode_long.h) against the one-lane path, and what the chunked
path's launches cost an encode without any long value. Not the bench metric
(that one is bench.py). Run on the GPU box:

    python tools/encode_long_bench.py cliff [--line 64M] [--one-lane-lines 1M,4M]
    python tools/encode_long_bench.py sweep [--sizes 256,1K,4K,16K,64K,1M,16M]
    python tools/encode_long_bench.py many  [--sizes 256,512,1K,4K,16K,64K] [--total 16M]
    python tools/encode_long_bench.py plain
                                      [--reps 3] [--out profiles/r17/encode_long/FILE.jsonl]

One process, one GPU. Every figure is the device time of the encode
(dgrep_last_encode_ms; for the job the pack's encode), the median of --reps runs
after one warm-up, and the outputs are compared before anything is timed.

  cliff  one line of --line bytes with a '"' every 8 bytes, between short lines,
         pattern `` (every line), through dgrep_map_partitions,
         dgrep_map_partitions_batch (one file) and the pack route of a windowed
         job, at long_value 0 (the chunked path). The one-lane path
         (dgrep_set_long_value(2^30)) is timed on the smaller lines of
         --one-lane-lines only: a lane escapes 2.6 MB/s.
  sweep  one escaped value per size, forced onto each path of the resident and of
         the batch writer. The crossover is the smallest size from which the
         chunked path is faster. Sizes above --one-lane-max take the chunked
         path only.
  many   the same with --total bytes of such values in one split, where the
         one-lane path runs a lane per value side by side.
  plain  the encode of ONE plain record: the floor of the pipeline's launches.
         Run on two builds, the difference is what the chunked path's launches
         (the scan of the counts, two chunk kernels with nothing to do, the fix
         kernel) add to every encode.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-grep_amd"))

UNITS = {"K": 1 << 10, "M": 1 << 20, "G": 1 << 30}
FILENAME = b"pg-big.txt"
R = 10
ONE_LANE = 1 << 30


def size(s):
    s = s.upper()
    return int(s[:-1]) * UNITS[s[-1]] if s[-1] in UNITS else int(s)


def escaped_value(n):
    return (b'abcdefg"' * (n // 8 + 1))[:n]


def window_for(n):
    return max(4096, (n + 8192 + 4095) // 4096 * 4096)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["cliff", "sweep", "many", "plain"])
    ap.add_argument("--line", default="64M")
    ap.add_argument("--one-lane-lines", default="1M,4M")
    ap.add_argument("--sizes", default="", help="default: 256 .. 16M (sweep), 256 .. 64K (many)")
    ap.add_argument("--total", default="16M")
    ap.add_argument("--one-lane-max", default="1M", help="sweep: no one-lane leg above this size (2.6 MB/s a lane)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch

    import dgrep

    assert torch.cuda.is_available(), "encode_long_bench.py needs a GPU"
    ctx = dgrep.Context(0)
    has_stats = hasattr(ctx, "encode_stats")  # a build from before dgrep_last_encode_stats: `plain` still runs

    def emit(rec):
        rec["lib"] = os.path.basename(dgrep.LIB_PATH)
        rec["build"] = dgrep.build_info()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def med(xs):
        return round(statistics.median(xs), 4)

    def long_values():
        return ctx.encode_stats()["long_values"] if has_stats else None

    def resident(data):
        parts = ctx.map_partitions(FILENAME, data, R)
        return parts, ctx.last_encode_ms(), long_values()

    def batch(data):
        parts = ctx.map_partitions_batch([(FILENAME, data)], R)[0]
        return parts, ctx.last_encode_ms(), long_values()

    def job_pack(data):
        """the pack route's encode: a second file that does not fit beside the
        first flushes the first pack; the job is closed without its reduce"""
        with ctx.job(window_for(len(data)), R) as job:
            job.add(FILENAME, data)
            job.add(FILENAME, data)
            stats = job.stats()
        assert stats["packs"] == 1 and stats["files_windowed"] == 0, stats
        return None, stats["encode_ms"], long_values()

    def timed(form, data):
        return [form(data)[1] for _ in range(args.reps + 1)][1:]

    if args.mode == "plain":
        ctx.load("")
        data = b"one plain record"
        want = resident(data)[0]
        assert batch(data)[0] == want and sum(map(len, want)) == len(b'{"Key":"pg-big.txt (line number #1)","Value":""}\n' + data)
        reps = max(args.reps, 30)
        rec = {"mode": "plain", "reps": reps}
        for name, form in (("resident", resident), ("batch", batch)):
            ms = [form(data)[1] for _ in range(reps + 5)][5:]
            rec[name + "_ms"] = med(ms)
            rec[name + "_min"] = round(min(ms), 4)
            rec[name + "_max"] = round(max(ms), 4)
        emit(rec)
    elif args.mode == "cliff":
        ctx.load("")

        def split_of(n):
            return b"a short line\n" * 100 + escaped_value(n) + b"\n" + b"another short line\n" * 100

        # the two paths against each other where the one-lane path is affordable, and against the value built here
        for n in [size(x) for x in args.one_lane_lines.split(",")]:
            data = split_of(n)
            ctx.set_long_value(0)
            want, _, lv = resident(data)
            assert lv == 1 and batch(data)[0] == want
            needle = b'","Value":"' + escaped_value(n).replace(b'"', b'\\"') + b'"}\n'
            assert sum(p.count(needle) for p in want) == 1, "the long line's encoded value is not in the output"
            rec = {"mode": "cliff", "line": n, "path": "one_lane"}
            ctx.set_long_value(ONE_LANE)
            for name, form in (("resident", resident), ("batch", batch)):
                got, _, lv = form(data)
                assert got == want and lv == 0, "the one-lane bytes differ from the chunked ones"
                ms = timed(form, data)
                rec[name + "_ms"], rec[name + "_all"] = med(ms), [round(x, 4) for x in ms]
            ctx.set_long_value(0)
            for name, form in (("resident", resident), ("batch", batch), ("job_pack", job_pack)):
                ms = timed(form, data)
                rec["chunked_" + name + "_ms"] = med(ms)
            emit(rec)
        n = size(args.line)
        data = split_of(n)
        ctx.set_long_value(0)
        want, _, lv = resident(data)
        assert lv == 1 and batch(data)[0] == want
        needle = b'","Value":"' + escaped_value(n).replace(b'"', b'\\"') + b'"}\n'
        assert sum(p.count(needle) for p in want) == 1, "the long line's encoded value is not in the output"
        rec = {"mode": "cliff", "line": n, "path": "chunked", "out_bytes": sum(map(len, want))}
        for name, form in (("resident", resident), ("batch", batch), ("job_pack", job_pack)):
            ms = timed(form, data)
            assert long_values() == 1
            rec[name + "_ms"], rec[name + "_all"] = med(ms), [round(x, 4) for x in ms]
        emit(rec)
    else:
        ctx.load("")
        sizes = args.sizes or ("256,1K,4K,16K,64K,1M,16M" if args.mode == "sweep" else "256,512,1K,4K,16K,64K")
        for n in (size(x) for x in sizes.split(",")):
            copies = max(1, size(args.total) // (n + 1)) if args.mode == "many" else 1
            data = b"a short line\n" + b"\n".join([escaped_value(n)] * copies)
            rec = {"mode": args.mode, "value": n, "values": copies}
            ctx.set_long_value(256)
            want = resident(data)[0]
            for name, form in (("resident", resident), ("batch", batch)):
                for path, lv in (("chunked", 256), ("one_lane", ONE_LANE)):
                    if lv == ONE_LANE and n > size(args.one_lane_max):
                        continue
                    ctx.set_long_value(lv)
                    got, _, took = form(data)
                    assert got == want and took == (copies if lv == 256 else 0), (name, path, took)
                    ms = timed(form, data)
                    rec["%s_%s_ms" % (name, path)] = med(ms)
                    rec["%s_%s_all" % (name, path)] = [round(x, 4) for x in ms]
            ctx.set_long_value(0)
            emit(rec)
    ctx.close()


if __name__ == "__main__":
    main()
