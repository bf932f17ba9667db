"""Whole map tasks over many small splits: what one batched scan + one batched
encode buy over one scan + one encode per split. Device-resident data
(dgrep_synth_corpus kind 0, seed 1), pattern `error`, nreduce 10, filenames
split-%05d.log; the shapes and protocol of tools/batch_bench.py. Not the bench
metric (that one is bench.py). Run on the GPU box:

    python tools/encode_batch_bench.py [--shapes 256x64M,4096x4M,65536x256K] [--reps 10] [--warmup 3]
                                       [--out profiles/r09/encode_batch/encode_batch_bench.jsonl]

For each shape k x S it prints one JSON line with three forms, taken in one
process on one GPU, alternated repetition by repetition:

  (a) per_split   k x (dgrep_scan_device + dgrep_encode_device), one pair per
                  split with its own filename: what a caller has without the
                  batch forms. From 65,536 splits on it runs --big-warmup +
                  --big-reps times only (a repetition takes most of a minute);
                  the line says how many.
  (b) packed      one dgrep_scan_device + one dgrep_encode_device over the same
                  bytes packed with '\\n' separators, one filename: the floor
                  (same records, almost the same output volume, nreduce cells
                  instead of k x nreduce)
  (c) batch       dgrep_scan_batch_device + dgrep_encode_batch_device

Each figure is host wall time around calls that end in a device
synchronisation (median and best), split into its scan and encode legs;
encode_dev_ms is the encode's device time (HIP events, dgrep_last_encode_ms;
summed over the splits for (a)). The three forms must report the same record
count, and on the smallest shape (c)'s cells must equal (a)'s partitions byte
for byte before anything is timed.
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


def parse_shape(s):
    k, size = s.lower().split("x")
    size = size.upper()
    return int(k), int(size[:-1]) * UNITS[size[-1]] if size[-1] in UNITS else int(size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x64M,4096x4M,65536x256K")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--big-reps", type=int, default=2, help="(a)'s timed repetitions from 65,536 splits on")
    ap.add_argument("--big-warmup", type=int, default=1)
    ap.add_argument("--pattern", default="error")
    ap.add_argument("--nreduce", type=int, default=10)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import dgrep

    assert torch.cuda.is_available(), "encode_batch_bench.py needs a GPU"
    L = dgrep.lib()
    ctx = dgrep.Context(0)
    ctx.load(args.pattern)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    R = args.nreduce
    shapes = [parse_shape(s) for s in args.shapes.split(",")]
    smallest = min(k for k, _ in shapes)

    for k, S in shapes:
        n = k * S
        n_packed = n + k - 1
        assert S % 16 == 0, "split i of the unpacked buffer starts at i * S: S must keep it 16-byte aligned"
        flat = torch.empty(n, dtype=torch.uint8, device="cuda")
        ctx.synth(flat.data_ptr(), n, 1, 0)
        packed = torch.empty(k * (S + 1), dtype=torch.uint8, device="cuda")
        packed.view(k, S + 1)[:, :S] = flat.view(k, S)
        packed.view(k, S + 1)[:, S] = 10
        cap = n // 96 + 1024
        ln, st, le = (torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(3))
        sp = torch.empty(cap, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        lens = np.full(k, S, np.uint64)
        names = [b"split-%05d.log" % i for i in range(k)]
        fptrs = (ctypes.c_char_p * k)(*names)
        flens = (ctypes.c_size_t * k)(*[len(f) for f in names])
        cnt, tot, ms = u64(), u64(), ctypes.c_float()
        pb, pe = (u64 * R)(), (u64 * R)()
        cell_off = np.zeros(k * R + 1, np.uint64)
        res = [vp(ln.data_ptr()), vp(st.data_ptr()), vp(le.data_ptr())]
        base = flat.data_ptr()
        split_ptrs = [vp(base + i * S) for i in range(k)]

        # output sizes: (c)'s total from a capacity-0 call, (b)'s likewise
        count_c = ctx.scan_batch_device(packed.data_ptr(), n_packed, lens, ln.data_ptr(), st.data_ptr(),
                                        le.data_ptr(), sp.data_ptr(), 0, cap)
        assert count_c <= cap
        _, total_c = ctx.encode_batch_device(packed.data_ptr(), n_packed, lens, ln.data_ptr(), st.data_ptr(),
                                             le.data_ptr(), sp.data_ptr(), count_c, names, R, 0, 0)
        out_cap = total_c + total_c // 8 + 4096  # (b)'s line numbers are P's: a few more digits
        out = torch.empty(out_cap, dtype=torch.uint8, device="cuda")
        out_a = torch.empty(out_cap if k == smallest else (out_cap // k) * 4 + 65536, dtype=torch.uint8, device="cuda")

        def enc_ms():
            L.dgrep_last_encode_ms(ctx._h, ctypes.byref(ms))
            return ms.value

        def per_split():
            total, t_scan, t_enc, dev = 0, 0.0, 0.0, 0.0
            o, ocap = vp(out_a.data_ptr()), out_a.numel()
            for i in range(k):
                t0 = time.perf_counter()
                rc = L.dgrep_scan_device(ctx._h, split_ptrs[i], S, res[0], res[1], res[2], cap, ctypes.byref(cnt))
                t1 = time.perf_counter()
                rc = rc or L.dgrep_encode_device(ctx._h, split_ptrs[i], S, res[0], res[1], res[2], cnt.value, names[i],
                                                 len(names[i]), R, o, ocap, pb, pe, ctypes.byref(tot))
                t2 = time.perf_counter()
                if rc:
                    ctx._check(rc)
                assert tot.value <= ocap
                total += cnt.value
                t_scan += t1 - t0
                t_enc += t2 - t1
                dev += enc_ms()
            return total, t_scan, t_enc, dev

        def one_packed():
            t0 = time.perf_counter()
            ctx._check(L.dgrep_scan_device(ctx._h, vp(packed.data_ptr()), n_packed, res[0], res[1], res[2], cap,
                                           ctypes.byref(cnt)))
            t1 = time.perf_counter()
            ctx._check(L.dgrep_encode_device(ctx._h, vp(packed.data_ptr()), n_packed, res[0], res[1], res[2], cnt.value,
                                             names[0], len(names[0]), R, vp(out.data_ptr()), out_cap, pb, pe,
                                             ctypes.byref(tot)))
            t2 = time.perf_counter()
            assert tot.value <= out_cap
            return cnt.value, t1 - t0, t2 - t1, enc_ms()

        def batch():
            t0 = time.perf_counter()
            c = ctx.scan_batch_device(packed.data_ptr(), n_packed, lens, ln.data_ptr(), st.data_ptr(), le.data_ptr(),
                                      sp.data_ptr(), 0, cap)
            t1 = time.perf_counter()
            ctx._check(L.dgrep_encode_batch_device(ctx._h, vp(packed.data_ptr()), n_packed, vp(lens.ctypes.data), k,
                                                   res[0], res[1], res[2], vp(sp.data_ptr()), c, fptrs, flens, R,
                                                   vp(out.data_ptr()), out_cap, vp(cell_off.ctypes.data),
                                                   ctypes.byref(tot)))
            t2 = time.perf_counter()
            assert tot.value == total_c
            return c, t1 - t0, t2 - t1, enc_ms()

        checked = None
        if k == smallest:
            # (c)'s cells against (a)'s partitions, every split, compared on the device
            batch()
            cells = out[:total_c].clone()
            off = cell_off.astype(np.int64).tolist()
            for i in range(k):
                c_i = ctx.scan_device(base + i * S, S, ln.data_ptr(), st.data_ptr(), le.data_ptr(), cap)
                b, e, t_i = ctx.encode_device(base + i * S, S, ln.data_ptr(), st.data_ptr(), le.data_ptr(), c_i,
                                              names[i], R, out_a.data_ptr(), out_a.numel())
                assert t_i <= out_a.numel() and t_i == off[(i + 1) * R] - off[i * R], (i, t_i)
                for p in range(R):
                    assert e[p] - b[p] == off[i * R + p + 1] - off[i * R + p], (i, p)
                    assert torch.equal(out_a[b[p]:e[p]], cells[off[i * R + p]:off[i * R + p + 1]]), (i, p)
            del cells
            checked = "every cell of (c) equals (a)'s partition, %d splits x %d" % (k, R)

        big = k >= 65536
        a_warm, a_reps = (args.big_warmup, args.big_reps) if big else (args.warmup, args.reps)
        forms = (("per_split", per_split), ("packed", one_packed), ("batch", batch))
        times = {name: [] for name, _ in forms}
        counts = {}
        for rep in range(args.warmup + args.reps):
            for name, fn in forms:
                if name == "per_split" and rep >= a_warm + a_reps:
                    continue
                t0 = time.perf_counter()
                c, t_scan, t_enc, dev = fn()
                dt = time.perf_counter() - t0
                assert c <= cap, (name, c, cap)
                assert counts.setdefault(name, c) == c
                warm = a_warm if name == "per_split" else args.warmup
                if rep >= warm:
                    times[name].append((dt * 1e3, t_scan * 1e3, t_enc * 1e3, dev))
        assert counts["per_split"] == counts["packed"] == counts["batch"] == count_c, counts

        rec = {"shape": "%dx%d" % (k, S), "splits": k, "split_bytes": S, "bytes": n, "pattern": args.pattern,
               "nreduce": R, "records": count_c, "output_bytes": total_c, "cells": k * R, "reps": args.reps,
               "warmup": args.warmup, "per_split_reps": a_reps, "per_split_warmup": a_warm}
        for name, _ in forms:
            col = lambda j: [t[j] for t in times[name]]
            rec[name] = {"wall_ms_median": round(statistics.median(col(0)), 3), "wall_ms_best": round(min(col(0)), 3),
                         "scan_wall_ms": round(statistics.median(col(1)), 3),
                         "encode_wall_ms": round(statistics.median(col(2)), 3),
                         "encode_dev_ms": round(statistics.median(col(3)), 3)}
        a, b, c = rec["per_split"], rec["packed"], rec["batch"]
        rec["per_split_over_batch"] = round(a["wall_ms_median"] / c["wall_ms_median"], 2)
        rec["batch_over_packed"] = round(c["wall_ms_median"] / b["wall_ms_median"], 3)
        rec["encode_per_split_over_batch"] = round(a["encode_wall_ms"] / c["encode_wall_ms"], 2)
        rec["encode_batch_over_packed"] = round(c["encode_wall_ms"] / b["encode_wall_ms"], 3)
        rec["encode_dev_batch_over_packed"] = round(c["encode_dev_ms"] / b["encode_dev_ms"], 3)
        if checked:
            rec["checked"] = checked
        rec["build"] = dgrep.build_info()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del flat, packed, ln, st, le, sp, out, out_a
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
