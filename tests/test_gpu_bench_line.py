"""The driver's contract with bench.py, end to end on the GPU: `python bench.py --gpus 1 --steps K --warmup W` prints ONE JSON line
whose metric is BASELINE.json's and whose value is the whole-solve throughput at 1280x720; with --full the line also carries the
roofline record of the dominant kernel (priced with counters that belong to the kernel sources in the tree) and the CPU baseline timed
on the host.  --dump-outputs writes what the last timed solve returned, the same from run to run."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_bench_line_has_the_contracts_fields():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2", "--no-side-records", "--full"], capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert base["metric"].startswith(d["metric"].split(",")[0])  # "Mpixels/sec RS depth+pose solve, 1280x720 pair ..."
    assert d["unit"] == "Mpixels/s" and d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f64" and d["data"].startswith("synthetic")
    assert "1280x720" in d["config"]["workload"] and "model" not in d["config"]
    assert d["value"] > 50.0  # north_star's target; the measured value is ~20x that
    assert abs(d["value"] - 1280 * 720 / (d["ms_per_step"] * 1e-3) / 1e6) <= 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] in ("fp64-valu", "hbm", "mfma") and r["peak"] > 0 and r["unit"]
    if r["counters_stale"]:  # the kernel sources changed since profiles/counters.json was collected: the line must say so and price nothing
        assert r["counters_stale_files"] and r["frac"] is None and r["achieved"] is None
    else:
        assert 0.3 < r["frac"] < 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
        assert r["traffic"] is None or r["traffic"] > 0.5 * r["alg_bytes_per_launch"]
    assert r["avg_launch_ms"] > 0
    assert 0.0 < r["hbm"]["frac"] < 1.0
    c = d["cpu_baseline"]
    assert c["value"] > 0 and c["unit"] == "Mpixels/s" and c["cores"] >= 1 and c["kind"] in ("port", "reference") and c["sample"]


def _plain_run(out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_solve(tmp_path):
    """a plain run: set-up, warm-up, the timed steps, the outputs of the last one, the line -- none of the --full sub-records"""
    import numpy as np

    d = _plain_run(tmp_path / "a")
    assert d["steps"] == 5 and d["warmup"] == 2 and d["unit"] == "Mpixels/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert abs(d["value"] - 1280 * 720 / (d["ms_per_step"] * 1e-3) / 1e6) <= 1e-6 * d["value"]
    assert not {"roofline", "refine_pass", "cpu_baseline", "regimes", "full_solve_batched", "tiled_full"} & set(d)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(n + ".npy" for n in ("depth_map", "pose_table_R", "pose_table_t", "pose", "ransac_pose", "counts", "refine_summary"))
    out = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype == np.float64 for a in out.values()) and sum(a.nbytes for a in out.values()) <= 64 << 20
    assert out["depth_map"].shape == (1280, 720) and out["pose_table_R"].shape == (720, 9) and out["pose_table_t"].shape == (720, 3)
    n, m = out["counts"][:2]
    assert n == 1280 * 720 and 0 < m <= n and np.count_nonzero(out["depth_map"]) <= m
    assert np.all(np.isfinite(out["pose"])) and out["refine_summary"][0] >= 1
    # the same arguments: the same inputs, the same outputs
    _plain_run(tmp_path / "b")
    for f in files:
        assert np.array_equal(np.load(tmp_path / "b" / f), out[f[:-4]]), f
