"""The reduce side of a worker that has just produced k x nreduce cells on the
GPU: what one batch reduce over the cells where they lie buys over copying them
out and reducing partition by partition. Device-resident data
(dgrep_synth_corpus kind 0, seed 1), pattern `error`, filenames split-%05d.log:
the shapes and protocol of tools/encode_batch_bench.py. Not the bench metric
(that one is bench.py). Run on the GPU box:

    python tools/reduce_batch_bench.py [--runs 256x64M:10,4096x4M:10,65536x256K:10,4096x4M:1000]
                                       [--reps 10] [--warmup 3]
                                       [--out profiles/r10/reduce_batch/reduce_batch_bench.jsonl]

For each run k x S : nreduce the cells come from one dgrep_scan_batch_device +
one dgrep_encode_batch_device and stay in HBM. One JSON line with three forms,
taken in one process on one GPU, alternated repetition by repetition:

  (a) per_partition  what a worker does today from device cells: a D2H copy of
                     all cells, a host concatenation of cells (0,p), (1,p), ...
                     per partition (numpy, empty cells skipped), and nreduce
                     dgrep_reduce calls; the three legs are also given apart
  (b) single         one dgrep_reduce over all cell bytes (already on the host)
                     as a single partition: the floor of the launch train. Its
                     output differs (keys merge across partitions), so it is
                     timed only
  (c) batch          dgrep_reduce_batch_device over the cells, seg_off = cell_off

Each figure is host wall time around calls that end in a device
synchronisation (median and best). reduce_dev_ms is the device time of the
reduce's launch train (HIP events): dgrep_last_kernel_ms for dgrep_reduce
(summed over the partitions for (a)), dgrep_last_reduce_ms for (c). Before
anything is timed every partition of (c) must equal (a)'s byte for byte.
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


def parse_run(s):
    shape, _, r = s.partition(":")
    k, size = shape.lower().split("x")
    size = size.upper()
    return int(k), int(size[:-1]) * UNITS[size[-1]] if size[-1] in UNITS else int(size), int(r or 10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="256x64M:10,4096x4M:10,65536x256K:10,4096x4M:1000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pattern", default="error")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import dgrep

    assert torch.cuda.is_available(), "reduce_batch_bench.py needs a GPU"
    L = dgrep.lib()
    ctx = dgrep.Context(0)
    ctx.load(args.pattern)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64

    for k, S, R in [parse_run(s) for s in args.runs.split(",")]:
        n = k * S
        n_packed = n + k - 1
        flat = torch.empty(n, dtype=torch.uint8, device="cuda")
        ctx.synth(flat.data_ptr(), n, 1, 0)
        packed = torch.empty(k * (S + 1), dtype=torch.uint8, device="cuda")
        packed.view(k, S + 1)[:, :S] = flat.view(k, S)
        packed.view(k, S + 1)[:, S] = 10
        del flat
        cap = n // 96 + 1024
        ln, st, le = (torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(3))
        sp = torch.empty(cap, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        lens = np.full(k, S, np.uint64)
        names = [b"split-%05d.log" % i for i in range(k)]
        count = ctx.scan_batch_device(packed.data_ptr(), n_packed, lens, ln.data_ptr(), st.data_ptr(), le.data_ptr(),
                                      sp.data_ptr(), 0, cap)
        assert count <= cap
        _, cells_total = ctx.encode_batch_device(packed.data_ptr(), n_packed, lens, ln.data_ptr(), st.data_ptr(),
                                                 le.data_ptr(), sp.data_ptr(), count, names, R, 0, 0)
        cells = torch.empty(cells_total + 16, dtype=torch.uint8, device="cuda")
        cell_off, t2 = ctx.encode_batch_device(packed.data_ptr(), n_packed, lens, ln.data_ptr(), st.data_ptr(),
                                               le.data_ptr(), sp.data_ptr(), count, names, R, cells.data_ptr(),
                                               cells_total)
        assert t2 == cells_total
        del packed, ln, st, le, sp
        torch.cuda.empty_cache()
        seg = np.asarray(cell_off, np.uint64)
        seg_i = seg.astype(np.int64)
        host = torch.empty(cells_total, dtype=torch.uint8).pin_memory()
        host_np = host.numpy()
        ms = ctypes.c_float()
        res = dgrep._ReduceOut()
        part_off = np.zeros(R + 1, np.uint64)
        lines_in = np.zeros(R, np.uint64)
        tot = u64()

        def reduce_host(buf, keep):
            """one dgrep_reduce over a host array: (device ms, output bytes or None)"""
            ctx._check(L.dgrep_reduce(ctx._h, vp(buf.ctypes.data if len(buf) else None), len(buf), ctypes.byref(res)))
            L.dgrep_last_kernel_ms(ctx._h, ctypes.byref(ms))
            out = ctypes.string_at(res.bytes, res.total) if keep and res.total else b""
            total = res.total
            L.dgrep_reduce_free(ctypes.byref(res))
            return (ms.value if len(buf) else 0.0), total, out

        def per_partition(keep=False):
            t0 = time.perf_counter()
            host.copy_(cells[:cells_total])  # (synchronous: pinned destination, default stream)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            inputs = []
            for p in range(R):
                a, b = seg_i[p:-1:R], seg_i[p + 1::R]
                nz = np.flatnonzero(b > a)
                inputs.append(np.concatenate([host_np[a[i]:b[i]] for i in nz.tolist()]) if len(nz)
                              else np.zeros(0, np.uint8))
            t2 = time.perf_counter()
            dev, total, outs = 0.0, 0, []
            for buf in inputs:
                d, t, o = reduce_host(buf, keep)
                dev += d
                total += t
                outs.append(o)
            t3 = time.perf_counter()
            return total, dev, (t1 - t0, t2 - t1, t3 - t2), outs

        def single():
            d, t, _ = reduce_host(host_np, False)
            return t, d, (0.0, 0.0, 0.0), None

        out_cap_box = [0]
        out = None

        def batch():
            ctx._check(L.dgrep_reduce_batch_device(ctx._h, vp(cells.data_ptr()), cells_total, vp(seg.ctypes.data),
                                                   len(seg) - 1, R, vp(out.data_ptr()) if out is not None else None,
                                                   out_cap_box[0], vp(part_off.ctypes.data), vp(lines_in.ctypes.data),
                                                   ctypes.byref(tot)))
            L.dgrep_last_reduce_ms(ctx._h, ctypes.byref(ms))
            return tot.value, ms.value, (0.0, 0.0, 0.0), None

        # (c) against (a), every partition, before anything is timed
        total_a, _, _, outs_a = per_partition(keep=True)
        total_c = batch()[0]
        assert total_c == total_a, (total_c, total_a)
        out = torch.empty(total_c + 16, dtype=torch.uint8, device="cuda")
        out_cap_box[0] = total_c
        assert batch()[0] == total_c
        got = out[:total_c].cpu().numpy().tobytes()
        off = part_off.astype(np.int64).tolist()
        for p in range(R):
            assert got[off[p]:off[p + 1]] == outs_a[p], p
        assert int(lines_in.sum()) == count
        checked = "every partition of (c) equals (a)'s, %d partitions" % R
        del got, outs_a

        forms = (("per_partition", per_partition), ("single", single), ("batch", batch))
        times = {name: [] for name, _ in forms}
        totals = {}
        for rep in range(args.warmup + args.reps):
            for name, fn in forms:
                t0 = time.perf_counter()
                total, dev, legs, _ = fn()
                dt = time.perf_counter() - t0
                assert totals.setdefault(name, total) == total
                if rep >= args.warmup:
                    times[name].append((dt * 1e3, dev) + tuple(x * 1e3 for x in legs))
        assert totals["per_partition"] == totals["batch"] == total_c, totals

        rec = {"shape": "%dx%d" % (k, S), "splits": k, "split_bytes": S, "bytes": n, "pattern": args.pattern,
               "nreduce": R, "records": count, "cells": k * R, "cell_bytes": cells_total, "output_bytes": total_c,
               "single_output_bytes": totals["single"], "reps": args.reps, "warmup": args.warmup}
        for name, _ in forms:
            col = lambda j: [t[j] for t in times[name]]
            rec[name] = {"wall_ms_median": round(statistics.median(col(0)), 3), "wall_ms_best": round(min(col(0)), 3),
                         "reduce_dev_ms": round(statistics.median(col(1)), 3)}
        rec["per_partition"].update(d2h_ms=round(statistics.median([t[2] for t in times["per_partition"]]), 3),
                                    concat_ms=round(statistics.median([t[3] for t in times["per_partition"]]), 3),
                                    reduce_calls_ms=round(statistics.median([t[4] for t in times["per_partition"]]), 3))
        a, b, c = rec["per_partition"], rec["single"], rec["batch"]
        rec["per_partition_over_batch"] = round(a["wall_ms_median"] / c["wall_ms_median"], 2)
        rec["batch_over_single"] = round(c["wall_ms_median"] / b["wall_ms_median"], 3)
        rec["dev_batch_over_single"] = round(c["reduce_dev_ms"] / b["reduce_dev_ms"], 3)
        rec["dev_per_partition_over_batch"] = round(a["reduce_dev_ms"] / c["reduce_dev_ms"], 3)
        rec["checked"] = checked
        rec["gpu"] = torch.cuda.get_device_name(0)
        rec["build"] = dgrep.build_info()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del cells, out, host
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
