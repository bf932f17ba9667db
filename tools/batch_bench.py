"""Many small splits: what one batched scan buys over one scan per split.
Device-resident data (dgrep_synth_corpus kind 0, seed 1), pattern `error`;
not the bench metric (that one is bench.py). Run on the GPU box:

    python tools/batch_bench.py [--shapes 256x64M,4096x4M,65536x256K] [--reps 10] [--warmup 3]

For each shape k x S (k splits of S bytes) it prints one JSON line with three
figures, taken in one process on one GPU, alternated repetition by repetition:

  (a) per_split   k consecutive dgrep_scan_device calls, one per split: what a
                  caller has without the batch form
  (b) packed      one dgrep_scan_device over the same bytes packed with '\\n'
                  separators: the floor (its line numbers and starts are the
                  packed buffer's, not the splits')
  (c) batch       dgrep_scan_batch_device over that packed buffer

Each figure is host wall time around calls that end in a device
synchronisation (median and best of --reps after --warmup), and GB/s of the
k x S split bytes over the median; newline_ms / rebase_ms are the batch form's
own kernels (HIP events, dgrep_last_batch_ms). The three forms must agree on
the number of matching lines, and (c)'s records of the first and last split
must equal (a)'s.
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
    ap.add_argument("--pattern", default="error")
    args = ap.parse_args()

    import numpy as np
    import torch

    import dgrep

    assert torch.cuda.is_available(), "batch_bench.py needs a GPU"
    L = dgrep.lib()
    ctx = dgrep.Context(0)
    ctx.load(args.pattern)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64

    for shape in args.shapes.split(","):
        k, S = parse_shape(shape)
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
        sb = torch.empty(k + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        lens = np.full(k, S, np.uint64)
        cnt = u64()
        res = [vp(ln.data_ptr()), vp(st.data_ptr()), vp(le.data_ptr())]
        base = flat.data_ptr()
        split_ptrs = [vp(base + i * S) for i in range(k)]

        def per_split():
            total = 0
            for p in split_ptrs:
                rc = L.dgrep_scan_device(ctx._h, p, S, res[0], res[1], res[2], cap, ctypes.byref(cnt))
                if rc:
                    ctx._check(rc)
                total += cnt.value
            return total

        def one_packed():
            ctx._check(L.dgrep_scan_device(ctx._h, vp(packed.data_ptr()), n_packed, res[0], res[1], res[2], cap,
                                           ctypes.byref(cnt)))
            return cnt.value

        def batch():
            return ctx.scan_batch_device(packed.data_ptr(), n_packed, lens, ln.data_ptr(), st.data_ptr(),
                                         le.data_ptr(), sp.data_ptr(), sb.data_ptr(), cap)

        forms = (("per_split", per_split), ("packed", one_packed), ("batch", batch))
        times = {name: [] for name, _ in forms}
        counts, batch_ms = {}, []
        for rep in range(args.warmup + args.reps):
            for name, fn in forms:
                t0 = time.perf_counter()
                c = fn()
                dt = time.perf_counter() - t0
                assert c <= cap, (name, c, cap)
                assert counts.setdefault(name, c) == c
                if rep >= args.warmup:
                    times[name].append(dt * 1e3)
                    if name == "batch":
                        batch_ms.append(ctx.last_batch_ms())
        assert counts["per_split"] == counts["packed"] == counts["batch"], counts

        # (c) against (a) on the first and the last split (the arrays hold (c)'s records now)
        total = counts["batch"]
        got = [t[:total].cpu().numpy() for t in (ln, st, le, sp)]
        ranges = sb.cpu().numpy()
        assert ranges[0] == 0 and ranges[k] == total and (np.diff(ranges) >= 0).all()
        for i in (0, k - 1):
            a, b = int(ranges[i]), int(ranges[i + 1])
            want_n = ctx.scan_device(base + i * S, S, ln.data_ptr(), st.data_ptr(), le.data_ptr(), cap)
            assert want_n == b - a, (i, want_n, a, b)
            for j, t in enumerate((ln, st, le)):
                np.testing.assert_array_equal(got[j][a:b], t[:want_n].cpu().numpy())
            assert (got[3][a:b] == i).all()

        out = {"shape": "%dx%d" % (k, S), "splits": k, "split_bytes": S, "bytes": n, "pattern": args.pattern,
               "matching_lines": total, "reps": args.reps, "warmup": args.warmup}
        for name, _ in forms:
            med = statistics.median(times[name])
            out[name] = {"wall_ms_median": round(med, 3), "wall_ms_best": round(min(times[name]), 3),
                         "gbs": round(n / med / 1e6, 1)}
        out["batch"]["newline_ms"] = round(statistics.median(m[0] for m in batch_ms), 3)
        out["batch"]["rebase_ms"] = round(statistics.median(m[1] for m in batch_ms), 3)
        out["batch"]["newline_gbs"] = round(n_packed / out["batch"]["newline_ms"] / 1e6, 1)
        out["batch_over_per_split"] = round(out["per_split"]["wall_ms_median"] / out["batch"]["wall_ms_median"], 2)
        out["batch_over_packed"] = round(out["batch"]["wall_ms_median"] / out["packed"]["wall_ms_median"], 3)
        out["build"] = dgrep.build_info()
        print(json.dumps(out), flush=True)
        del flat, packed, ln, st, le, sp, sb
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
