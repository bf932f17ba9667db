"""bench.py's rank launch contract on a machine without GPUs: `--gpus N`
(N > 1) without a launcher must start N rank processes or fail fast -- never
print an N=1 line -- and `--gpus` must agree with WORLD_SIZE under a launcher."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True,
                          text=True, timeout=120)


def test_gpus_without_devices_fails_fast():
    import torch

    if torch.cuda.device_count() >= 2:
        pytest.skip("GPUs visible: the launch path would really start ranks")
    p = _run(["--gpus", "2", "--steps", "2"])
    assert p.returncode == 2, (p.returncode, p.stderr[-2000:])
    assert p.stdout.strip() == "", "no JSON line may be printed"
    assert "GPU(s) visible" in p.stderr


def test_gpus_disagrees_with_world_size():
    p = _run(["--gpus", "4", "--steps", "2"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode == 2, (p.returncode, p.stderr[-2000:])
    assert p.stdout.strip() == ""
    assert "disagrees with WORLD_SIZE" in p.stderr


def test_dry_run_world2_line():
    """`bench.py --gpus 2 --dry-run --full` (CPU, gloo, the oracle standing in
    for the scan): the N > 1 line carries the node-wide CPU comparators and
    prices the roofline with the SLOWEST rank's kernel time, per GPU and for the
    node."""
    import json

    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run", "--full",
                        "--split-gib", "0.01", "--steps", "2", "--warmup", "0", "--cpu-seconds", "1"],
                       env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")},
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] is None and "dry_run" in d
    r = d["roofline"]
    per = r["per_rank_kernel_ms_avg"]
    assert len(per) == 2 and r["kernel_ms_avg"] == max(per) and r["slowest_rank"] == per.index(max(per))
    assert r["aggregate"]["peak"] == 2 * r["peak"] and r["aggregate"]["achieved"] >= r["achieved"]
    assert d["cpu_baseline_mt"] and d["cpu_baseline_mt"]["cores"] >= 1 and d["cpu_baseline_mt"]["value"] > 0
    w = d["cpu_baseline_workers"]
    assert w and w["cores"] == 2 and w["workers"] == 2 and w["value"] > 0
    assert len(d["config"]["matching_lines_per_split"]) == 2
    # the exchange: rank 0's gathered records checked against every rank's own
    assert d["exchange"].startswith("torch") and d["gather_verified"] is True
    g = d["gather"]
    assert g["per_rank_counts"] == d["config"]["matching_lines_per_split"] and g["checksums_match"]


def test_plain_dry_run_dumps_the_last_steps_records(tmp_path):
    """A plain run (no --full) times --steps steps, leaves the checks and CPU
    baselines out of the line, and --dump-outputs writes the last step's
    records: here (dry run) the oracle's own over the seeded split."""
    import json

    import numpy as np

    import dgrep
    import oracle_lib as O

    out = tmp_path / "dump"
    p = _run(["--gpus", "1", "--dry-run", "--split-gib", "0.002", "--steps", "3", "--warmup", "1",
              "--dump-outputs", str(out)])
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["full"] is False
    assert d["cpu_baseline"] is None and d["cpu_baseline_mt"] is None and "gather" not in d
    assert d["unit"] == "GB/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    n = int(0.002 * (1 << 30))
    n -= n % 64
    want = O.grep_map(b"error", dgrep.synth_corpus_host(n, 2, 0))
    assert len(want[0]) > 0 and d["config"]["matching_lines_per_split"] == len(want[0])
    got = {k: np.load(out / (k + ".npy")) for k in ("line", "start", "len", "index", "totals")}
    assert all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["index"], np.arange(len(want[0])))
    for k, w in zip(("line", "start", "len"), want):
        np.testing.assert_array_equal(got[k], w.astype(np.float64))
    np.testing.assert_array_equal(got["totals"], [len(want[0])] + [float(int(w.sum())) for w in want])


def test_dump_outputs_samples_a_large_output(tmp_path, monkeypatch):
    """Past DUMP_SAMPLE records the dump is a fixed seeded sample (the same
    indices for the same count) and totals.npy still covers every record."""
    import numpy as np
    import torch

    import bench

    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    count = 1000
    line = torch.arange(1, count + 25, dtype=torch.int64) * 3  # capacity beyond count is not output
    start, ln = line * 1000 + (1 << 40), line % 97
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), line, start, ln, count, 1, 0)
    a = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in ("line", "start", "len", "index", "totals")}
    for k, v in a.items():
        np.testing.assert_array_equal(v, np.load(tmp_path / "b" / (k + ".npy")))
    idx = a["index"].astype(np.int64)
    assert 50 < len(idx) <= 100 and (np.diff(idx) > 0).all() and idx[-1] < count
    for k, t in (("line", line), ("start", start), ("len", ln)):
        np.testing.assert_array_equal(a[k], t.numpy()[idx].astype(np.float64))
    np.testing.assert_array_equal(a["totals"], [count] + [float(int(t[:count].sum())) for t in (line, start, ln)])
