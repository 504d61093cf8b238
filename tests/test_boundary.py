"""-m "not gpu": the drop-in boundary -- the C-ABI library loads and exports every symbol the header
declares, the ctypes table matches the header, the product never touches oracle/ or the reference,
and the host-side mirror of the reference API behaves like the reference without a GPU."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "3dgsconverter_amd")


def _header_functions():
    text = open(os.path.join(ROOT, "include", "gsx_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gsx_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(gsx):
    lib_path = gsx._lib.LIB_PATH
    assert os.path.exists(lib_path), "run python 3dgsconverter_amd/build.py"
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    exported = set(re.findall(r"\bT (gsx_[a-z0-9_]+)", syms))
    declared = _header_functions()
    assert declared, "header parse failed"
    missing = [f for f in declared if f not in exported]
    assert not missing, missing
    lib = gsx._lib.load()  # binds all of them through ctypes
    assert lib.gsx_version().startswith(b"gsx-hip")


def test_ctypes_table_matches_header(gsx):
    assert sorted(gsx._lib.SIGNATURES) == _header_functions()


def test_header_cites_reference_lines():
    text = open(os.path.join(ROOT, "include", "gsx_hip.h")).read()
    for needle in ("data_processor.py:156-173", "data_processor.py:176-178", "gpu_ops.py:193-263",
                   "data_processor.py:38-52", "data_processor.py:111-114", "gpu_ops.py:178-191", "sog.py:408-419"):
        assert needle in text, needle


def test_product_never_imports_oracle_or_reference():
    bad = []
    for dirpath, _, files in os.walk(PKG):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) or "/root/reference" in src:
                    bad.append(os.path.join(dirpath, f))
    assert not bad, bad


def test_only_test_infrastructure_touches_the_oracle():
    """outside tests/ and oracle/ the oracle is imported in exactly three places: smoke(), bench.py's cpu_baseline leg and
    the cpu_baseline leg of its K-Means workload (tools/bench_kmeans.py)"""
    root = os.path.dirname(PKG)
    allowed = {"__graft_entry__.py", "bench.py", os.path.join("tools", "bench_kmeans.py")}
    hits = set()
    for dirpath, dirs, files in os.walk(root):
        rel = os.path.relpath(dirpath, root)
        if rel.split(os.sep)[0] in ("tests", "oracle", ".git", "gpurun_out", "profiles"):
            dirs[:] = []
            continue
        for f in files:
            if f.endswith((".py", ".sh")):
                src = open(os.path.join(dirpath, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M):
                    hits.add(os.path.normpath(os.path.join(rel, f)))
    assert hits <= allowed, hits - allowed
    for f in ("bench.py", os.path.join("tools", "bench_kmeans.py")):   # ... and there only inside a cpu_baseline leg
        src = open(os.path.join(root, f)).read()
        for m in re.finditer(r"^\s*(from|import)\s+oracle\b", src, flags=re.M):
            before = src[:m.start()]
            assert "cpu_baseline" in before[-700:], (f, m.group(0))


def test_no_gpu_means_loud_failure_not_fallback(gsx):
    if gsx.has_hip():
        pytest.skip("a GPU is present")
    arr = np.zeros(100, dtype=[("x", "f4"), ("y", "f4"), ("z", "f4")])
    arr["x"] = np.arange(100)
    with pytest.raises(gsx.GsxError):
        gsx.DataProcessor(arr).remove_flyers(8, 1.0)
    with pytest.raises(gsx.GsxError):
        gsx.DataProcessor(arr).apply_density_filter(sensitivity=0.5)
    with pytest.raises(gsx.GsxError):
        gsx.gpu_ops.kmeans(np.zeros((100, 3), np.float32), 4)
    with pytest.raises(gsx.GsxError):
        gsx.gpu_ops.filter_sor_gpu(np.zeros((100, 3), np.float32), 8, 1.0)
    assert gsx.gpu_ops.HAS_TAICHI is False and gsx.gpu_ops.HAS_HIP is False


def test_api_shape_and_errors_without_gpu(gsx):
    dp = gsx.DataProcessor([1, 2, 3])
    with pytest.raises(TypeError, match="numpy structured array"):
        dp.remove_flyers()
    with pytest.raises(TypeError, match="numpy structured array"):
        dp.apply_density_filter()
    with pytest.raises(ValueError, match="Requires 3D data"):
        gsx.gpu_ops.filter_sor_gpu(np.zeros((5, 2), np.float32))
    data = np.random.default_rng(0).standard_normal((10, 3)).astype(np.float32)
    c, l = gsx.gpu_ops.kmeans(data, 10)  # k >= N shortcut never touches the GPU (gpu_ops.py:30-31)
    np.testing.assert_array_equal(c, data)
    np.testing.assert_array_equal(l, np.arange(10, dtype=np.int32))
    empty = np.zeros(0, dtype=[("x", "f4"), ("y", "f4"), ("z", "f4")])
    assert len(gsx.DataProcessor(empty).remove_flyers(8, 1.0)) == 0
    import inspect
    sig = inspect.signature(gsx.DataProcessor.remove_flyers)
    assert list(sig.parameters)[1:] == ["k", "threshold_factor", "chunk_size", "intensity"]
    assert sig.parameters["k"].default == 25 and sig.parameters["threshold_factor"].default == 10.5
    sig = inspect.signature(gsx.DataProcessor.apply_density_filter)
    assert list(sig.parameters)[1:] == ["voxel_size", "threshold_percentage", "sensitivity", "keep_multicluster"]
    sig = inspect.signature(gsx.gpu_ops.kmeans)
    assert list(sig.parameters)[:6] == ["data", "k", "max_iter", "tolerance", "use_gpu", "verbose"]


def test_param_maps_match_oracle(gsx):
    from oracle import density as oden, sor as osor
    dpm = gsx.processing.data_processor
    for i in (1, 2.5, 5, 7, 10):
        assert dpm.sor_params_from_intensity(i) == osor.params_from_intensity(i)
    for s in (0.0, 0.1, 0.5, 0.9, 1.0, 1.5):
        assert dpm.density_params_from_sensitivity(s) == oden.params_from_sensitivity(s)


def test_cluster_selection_matches_oracle(gsx):
    """host BFS + keep rule (clusters.py) == oracle restatement of data_processor.py:57-106, ties included"""
    from oracle import density as oden
    clusters = gsx.processing.clusters
    rng = np.random.default_rng(4)
    for trial in range(40):
        pts = np.unique(rng.integers(-4, 5, size=(rng.integers(1, 60), 3)), axis=0)  # lexicographic like np.unique
        for multi in (False, True):
            want, want_kept, want_max = oden.cluster_dense_voxels(pts, multi)
            comps = clusters.connected_clusters(map(tuple, pts.tolist()))
            got, got_kept, got_max = clusters.select_clusters(comps, multi)
            assert got == want and got_kept == want_kept and got_max == want_max
    # two equal clusters: the first met in set-iteration order wins, same as the reference
    pts = np.array([[0, 0, 0], [0, 0, 1], [5, 5, 5], [5, 5, 6]])
    want, _, _ = oden.cluster_dense_voxels(pts, False)
    got, _, _ = clusters.select_clusters(clusters.connected_clusters(map(tuple, pts.tolist())), False)
    assert got == want


_STANDIN = {   # the module layout install() rebinds, with the names the orchestrator resolves at call time (no reference code)
    "gsconverter/__init__.py": "",
    "gsconverter/processing/__init__.py": "from . import gpu_ops\nfrom .data_processor import DataProcessor\n",
    "gsconverter/processing/gpu_ops.py": "HAS_TAICHI = False\n",
    "gsconverter/processing/data_processor.py":
        "class DataProcessor:\n"
        "    def __init__(self, data):\n        self.data = data\n"
        "    def later_method(self, n):\n        return ('forwarded', len(self.data), n)\n",
    "gsconverter/converter.py": "from .processing import DataProcessor\n",
    "gsconverter/formats/__init__.py": "",
    "gsconverter/formats/sog.py": "from ..processing import gpu_ops\n\nclass SogFormat:\n    def write(self, data, path, **kw):\n        return 'own'\n",
    "gsconverter/formats/compressed_ply.py": "class CompressedPlyFormat:\n    def write(self, data, path, **kw):\n        return 'own'\n",
}


def test_install_patches_reference_when_present(gsx, tmp_path, monkeypatch):
    """install() on a stand-in ``gsconverter`` package with the reference's module layout: every name the orchestrator and
    the writers resolve is rebound, a method this package does not implement is forwarded to the package's own class, and
    uninstall() puts everything back"""
    for rel, src in _STANDIN.items():
        (tmp_path / rel).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / rel).write_text(src)
    saved = {m: sys.modules.pop(m) for m in list(sys.modules) if m == "gsconverter" or m.startswith("gsconverter.")}
    mine = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    monkeypatch.setattr(mine, "_REFERENCE_CLASS", None)
    monkeypatch.syspath_prepend(str(tmp_path))
    try:
        import gsconverter.converter as rconv
        import gsconverter.formats.compressed_ply as rcply
        import gsconverter.formats.sog as rsog
        import gsconverter.processing as rp
        import gsconverter.processing.data_processor as rdp
        orig, own_gpu_ops, own_sog_write, own_cply_write = rdp.DataProcessor, rp.gpu_ops, rsog.SogFormat.write, rcply.CompressedPlyFormat.write
        try:
            gsx.install()
            assert issubclass(rp.DataProcessor, gsx.DataProcessor) and issubclass(rdp.DataProcessor, gsx.DataProcessor)
            assert rp.gpu_ops is gsx.gpu_ops and rsog.gpu_ops is gsx.gpu_ops and sys.modules["gsconverter.processing.gpu_ops"] is gsx.gpu_ops
            assert rconv.DataProcessor is mine.ChainedDataProcessor
            assert rsog.SogFormat.write is not own_sog_write and rcply.CompressedPlyFormat.write is not own_cply_write
            arr = np.zeros(5, dtype=[("x", "f4"), ("y", "f4"), ("z", "f4")])
            arr["x"] = np.arange(5)
            out = gsx.DataProcessor(arr).crop_by_bbox(1, -1, -1, 3, 1, 1)
            assert len(out) == 3
            # a method of the reference class this package does not implement is forwarded to it
            assert gsx.DataProcessor(arr).later_method(7) == ("forwarded", 5, 7)
        finally:
            gsx.uninstall()
        assert rdp.DataProcessor is orig and rp.DataProcessor is orig and rp.gpu_ops is own_gpu_ops and rsog.gpu_ops is own_gpu_ops
        assert rsog.SogFormat.write is own_sog_write and rcply.CompressedPlyFormat.write is own_cply_write
        assert sys.modules["gsconverter.processing.gpu_ops"] is own_gpu_ops
    finally:
        for m in [m for m in sys.modules if m == "gsconverter" or m.startswith("gsconverter.")]:
            del sys.modules[m]
        sys.modules.update(saved)


def test_info_struct_layout_matches_the_header(gsx, tmp_path):
    """the ctypes mirror of gsx_sor_info must have the C compiler's size and field offsets"""
    import ctypes as C
    import subprocess
    src = tmp_path / "layout.c"
    fields = [f[0] for f in gsx._lib.SorInfo._fields_]
    body = "".join('printf("%%s %%zu\\n", "%s", offsetof(gsx_sor_info, %s));' % (f, f) for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsx_hip.h"\nint main(void){printf("size %zu\\n", sizeof(gsx_sor_info));'
                   + body + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(gsx._lib.SorInfo)
    for f in fields:
        assert int(out[f]) == getattr(gsx._lib.SorInfo, f).offset, f


def test_sor_k_range_is_checked_at_the_python_boundary(gsx):
    """the reference's cKDTree path takes any k (its Taichi kernel caps K at 50): here 1..2047 (65 and above on the exact
    list-free kernel); anything else is refused with a clear message before it reaches the device"""
    arr = np.zeros(100, dtype=[("x", "f4"), ("y", "f4"), ("z", "f4")])
    arr["x"] = np.arange(100)
    with pytest.raises(ValueError, match="1..2047"):
        gsx.DataProcessor(arr).remove_flyers(2048, 1.0)
    with pytest.raises(ValueError, match="1..2047"):
        gsx.gpu_ops.filter_sor_gpu(np.zeros((100, 3), np.float32), k=0)
    # every --sor_intensity maps inside the range (data_processor.py:125-134)
    from importlib import import_module
    dp = import_module("3dgsconverter_amd.processing.data_processor")
    assert [dp.sor_params_from_intensity(i)[0] for i in (1, 5, 10)] == [10, 27, 50]
