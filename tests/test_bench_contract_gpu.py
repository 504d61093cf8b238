"""GPU: `bench.py` prints exactly ONE JSON line on stdout carrying the contract's fields (a small configuration)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", *extra],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines          # RCCL banners and warnings must not reach stdout
    return json.loads(lines[0])


def test_plain_line_is_the_headline_alone():
    """no --full: set-up, warm-up, the timed steps and the line -- no other configuration, CPU baseline or per-kernel pass"""
    d = _run("--n", "300000", "--extent", "10")
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "survivors_rank0", "threshold"):
        assert key in d, key
    for key in ("cpu_baseline", "configs", "grid", "value_resident"):
        assert key not in d, key
    assert list(d["kernel_ms_per_step"]) == ["knn"]      # the HIP events inside the timed region; no separate pass
    assert d["metric"] == "Msplats/sec SOR k=16" and d["dtype"] == "f32 select / f64 finalize" and d["higher_is_better"] is True
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "Msplats/s"
    assert abs(d["value"] - 300000 / (d["ms_per_step"] * 1e-3) / 1e6) < 0.02 * d["value"]
    assert d["roofline"]["kernel"] == "knn_brick_kernel" and d["roofline"]["kernel_ms"] > 0


def test_sor_line_has_the_contract_fields():
    d = _run("--n", "300000", "--extent", "10", "--full", "--no-secondary")
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "Msplats/s" and d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"] and "300000" in d["config"]["workload"]
    assert abs(d["value"] - 300000 / (d["ms_per_step"] * 1e-3) / 1e6) < 0.02 * d["value"]
    r = d["roofline"]
    assert r["kernel"] == "knn_brick_kernel" and r["kernel_ms"] > 0 and r["bound"] in ("hbm", "valu")
    hbm = r["hbm"] if "hbm" in r else r
    for key in ("achieved", "peak", "unit", "frac", "traffic"):
        assert key in hbm, key
    assert hbm["unit"] == "GB/s" and hbm["peak"] == 8000.0 and abs(hbm["frac"] - hbm["achieved"] / hbm["peak"]) < 1e-4
    c = d["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in c, key
    assert c["kind"] == "port" and c["cores"] >= 1 and c["mask_identical_to_gpu"] is True


def test_slab_pipeline_line_one_rank():
    d = _run("--n", "300000", "--extent", "10", "--no-secondary", "--no-cpu-baseline", "--exchange", "slab")
    assert "slab" in d["config"]["parallelism"] and d["survivors_rank0"] > 0


def test_dump_outputs_are_the_timed_steps_results(tmp_path):
    """--dump-outputs DIR: the last timed step's mask, mean distances and statistics == the oracle on the same cloud"""
    sys.path.insert(0, ROOT)
    import bench
    from oracle import sor as osor
    d = _run("--n", "300000", "--extent", "10", "--no-secondary", "--no-cpu-baseline", "--dump-outputs", str(tmp_path))
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and sorted(d["dump_outputs"]["files"]) == ["index", "mask", "mean_dists", "stats", "survivors"]
    ref = osor.sor(bench.synth_uniform(300000, 10.0, 0), 16, 1.0)
    assert np.array_equal(np.load(tmp_path / "index.npy"), np.arange(300000))
    assert np.array_equal(np.load(tmp_path / "mask.npy"), ref["mask"].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "mean_dists.npy").view(np.uint32), ref["mean_dists"].view(np.uint32))
    assert np.float32(np.load(tmp_path / "stats.npy")[2]) == np.float32(ref["threshold"])
    assert np.load(tmp_path / "survivors.npy")[0] == d["survivors_rank0"] == ref["mask"].sum()
