"""-m "not gpu": the .splat writer's host side -- the numpy restatement against the reference's files (tests/golden/splat_ref.npz),
the tie rule, the reference's errors before any device work and without a file, empty tables, and the install() binding."""
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import splat_numpy  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "splat_ref.npz")
ERRORS = {"ValueError": ValueError}


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return g, json.loads(bytes(g["spec"]).decode())


@pytest.fixture(scope="module")
def writer():
    return importlib.import_module("3dgsconverter_amd.formats.splat_writer")


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgsconverter_amd._lib")


def _table(g, spec, name):
    return g["edges__table"] if spec[name]["kind"] == "edges" else splat_numpy.case_table(spec[name])


def _same(got: bytes, g, name):
    if name + "__sha256" in g:
        return hashlib.sha256(got).digest() == g[name + "__sha256"].tobytes()
    return got == g[name].tobytes()


def test_edge_rows_are_the_recorded_ones(gold):
    g, _ = gold
    t = splat_numpy.edge_table()
    assert t.tobytes() == g["edges__table"].tobytes()
    assert len(t) % 16 != 0


def test_restatement_equals_every_golden_file(gold):
    g, spec = gold
    assert len(spec) >= 30
    checked = 0
    for name, rec in spec.items():
        if "error" in rec:
            continue
        got = splat_numpy.file_bytes(_table(g, spec, name))
        assert len(got) == rec["bytes"] and _same(got, g, name), name
        checked += 1
    assert checked >= 25
    assert sum(rec.get("ties", False) for rec in spec.values()) >= 5          # tie-heavy cases, stable order
    assert sum(rec.get("ties") is False for rec in spec.values()) >= 20       # tie-free cases, the unpatched reference's files


def test_edge_rows_reach_nan_casts_in_the_vector_body_and_the_remainder(gold):
    """in the reference's arrays (sorted order), NaN reaches the u8 casts of colour, alpha and rotation at positions inside
    16-element blocks and in the last partial block (the golden file then pins numpy's result, 0)"""
    g, spec = gold
    t = g["edges__table"][splat_numpy.order(g["edges__table"])]
    n = len(t)
    with np.errstate(all="ignore"):
        colour = np.isnan((np.float32(0.5) + splat_numpy.SH_C0 * t["f_dc_0"]) * np.float32(255))
        alpha = np.isnan(np.float32(1) / (np.float32(1) + np.exp(-t["opacity"])))
        q = [t[f"rot_{a}"] for a in range(4)]
        rot = np.isnan(q[0] / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]))
    tail = n // 16 * 16
    for m in (colour, alpha, rot):
        idx = np.nonzero(m)[0]
        assert (idx < tail).any() and (idx >= tail).any(), idx
    rec = np.frombuffer(g["edges"].tobytes(), splat_numpy.RECORD)
    assert (rec["rot"][rot, 0] == 0).all() and (rec["color"][alpha, 3] == 0).all() and (rec["color"][colour, 0] == 0).all()


def test_ties_keep_input_order():
    t = splat_numpy.ties_table(300, 9, "all")
    assert np.array_equal(splat_numpy.order(t), np.arange(300))
    m = np.array([1.0, -0.0, np.nan, 0.0, 2.0, np.nan, 1.0, -np.nan], np.float32)
    # -metric ascending, equal keys by index: -2 | -1 -1 | -0 +0 (equal) | NaN NaN NaN
    assert np.argsort(-m, kind="stable").tolist() == [4, 0, 6, 1, 3, 2, 5, 7]


def test_errors_come_before_any_device_work(writer, gold, lib, tmp_path, monkeypatch):
    """the reference's exception types and messages for a missing field, TypeError for a float field that is not little-endian
    float32 or colour bytes that are not u1 -- raised with the device path made unreachable, and no file created"""
    def boom(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(lib, "splat_pack_table", boom)
    monkeypatch.setattr(lib, "require_hip", boom)
    g, spec = gold
    path = tmp_path / "x.splat"
    n_err = 0
    for name, rec in spec.items():
        if "error" not in rec:
            continue
        with pytest.raises(ERRORS[rec["error"][0]]) as e:
            writer.write_splat(_table(g, spec, name), str(path))
        assert str(e.value) == rec["error"][1], name
        assert not path.exists(), name
        n_err += 1
    assert n_err >= 6
    t = splat_numpy.random_table(10, 1)
    for f, dt in (("opacity", "<f8"), ("rot_1", ">f4"), ("scale_2", "<f2"), ("x", "<i4"), ("f_dc_2", "<f8")):
        bad = np.zeros(10, [(n, dt if n == f else t.dtype[n]) for n in t.dtype.names])
        with pytest.raises(TypeError, match=f):
            writer.write_splat(bad, str(path))
    r = splat_numpy.rgb_table(10, 2)
    for f, dt in (("green", "<u2"), ("red", "<f4"), ("blue", "i1")):
        bad = np.zeros(10, [(n, dt if n == f else r.dtype[n]) for n in r.dtype.names])
        with pytest.raises(TypeError, match=f):
            writer.write_splat(bad, str(path))
    assert not path.exists()


def test_empty_table_writes_an_empty_file_without_the_device(writer, gold, lib, tmp_path, monkeypatch):
    g, spec = gold
    monkeypatch.setattr(lib, "splat_pack_table", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device touched")))
    writer.write_splat(_table(g, spec, "n0"), str(tmp_path / "e.splat"))
    assert (tmp_path / "e.splat").read_bytes() == b"" == g["n0"].tobytes()


def test_host_metric_is_the_restatements(lib, gold):
    g, _ = gold
    t = g["edges__table"]
    assert lib.splat_metric_host(t).tobytes() == splat_numpy.metric(t).tobytes()


_STANDIN = {
    "gsconverter/__init__.py": "",
    "gsconverter/processing/__init__.py": "from . import gpu_ops\nfrom .data_processor import DataProcessor\n",
    "gsconverter/processing/gpu_ops.py": "HAS_TAICHI = False\n",
    "gsconverter/processing/data_processor.py": "class DataProcessor:\n    def __init__(self, data):\n        self.data = data\n",
    "gsconverter/converter.py": "from .processing import DataProcessor\n",
    "gsconverter/formats/__init__.py": "",
    "gsconverter/formats/splat.py": "class SplatFormat:\n    def write(self, data, path, **kw):\n        return 'own'\n",
}


def test_install_rebinds_splat_write_on_a_stand_in_and_uninstall_restores_it(gsx, tmp_path, monkeypatch):
    for rel, src in _STANDIN.items():
        (tmp_path / rel).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / rel).write_text(src)
    saved = {m: sys.modules.pop(m) for m in list(sys.modules) if m == "gsconverter" or m.startswith("gsconverter.")}
    mine = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    monkeypatch.setattr(mine, "_REFERENCE_CLASS", None)
    monkeypatch.syspath_prepend(str(tmp_path))
    writer = importlib.import_module("3dgsconverter_amd.formats.splat_writer")
    try:
        import gsconverter.formats.splat as rsp
        own = rsp.SplatFormat.write
        calls = []
        monkeypatch.setattr(writer, "write_splat", lambda data, path, **kw: calls.append((len(data), path, kw)) or "mine")
        try:
            gsx.install(splat_writer=False)
            assert rsp.SplatFormat.write is own
            gsx.uninstall()
            assert rsp.SplatFormat.write is own
            gsx.install()
            assert rsp.SplatFormat.write is not own
            assert rsp.SplatFormat().write(np.zeros(3), "a.splat") == "mine"
            assert rsp.SplatFormat().write(np.zeros(2), "b.splat", extra=1) == "mine"
            assert calls == [(3, "a.splat", {}), (2, "b.splat", {"extra": 1})]
        finally:
            gsx.uninstall()
        assert rsp.SplatFormat.write is own
    finally:
        for m in [m for m in sys.modules if m == "gsconverter" or m.startswith("gsconverter.")]:
            del sys.modules[m]
        sys.modules.update(saved)
