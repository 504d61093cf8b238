"""-m "not gpu": the .ksplat writer's host side -- the numpy restatement against the reference's files
(tests/golden/ksplat_ref.npz, and a live run when the reference is mounted), the reference's errors before any device work,
the host twin of numpy's exp and the runtime probe, the host patch of the rows and buckets the device lists, and the install()
binding."""
import hashlib
import importlib
import json
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ksplat_numpy  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ksplat_ref.npz")
ERRORS = {"ZeroDivisionError": ZeroDivisionError, "error": struct.error, "ValueError": ValueError}


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return g, json.loads(bytes(g["spec"]).decode())


@pytest.fixture(scope="module")
def writer():
    return importlib.import_module("3dgsconverter_amd.formats.ksplat_writer")


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgsconverter_amd._lib")


def _table(g, spec, name):
    return g["edges__table"] if spec[name]["kind"] == "edges" else ksplat_numpy.case_table(spec[name])


def _same(got: bytes, g, name):
    if name + "__sha256" in g:
        return hashlib.sha256(got).digest() == g[name + "__sha256"].tobytes()
    return got == g[name].tobytes()


def test_edge_rows_are_the_recorded_ones(gold):
    g, _ = gold
    assert ksplat_numpy.edge_table().tobytes() == g["edges__table"].tobytes()


def test_restatement_equals_every_golden_file(gold):
    g, spec = gold
    assert len(spec) >= 60
    for name, rec in spec.items():
        t = _table(g, spec, name)
        if "error" in rec:
            with pytest.raises(ERRORS[rec["error"][0]]) as e:
                ksplat_numpy.file_bytes(t, rec["level"], **rec.get("kw", {}))
            assert str(e.value) == rec["error"][1], name
            continue
        got = ksplat_numpy.file_bytes(t, rec["level"], **rec.get("kw", {}))
        assert len(got) == rec["bytes"] and _same(got, g, name), name


@pytest.mark.skipif(not os.path.isdir("/root/reference/gsconverter"), reason="reference checkout not present")
def test_restatement_equals_a_live_reference_run(tmp_path):
    sys.path.insert(0, ROOT)
    from oracle import refload
    refload.load()
    from gsconverter.formats.ksplat import KSplatFormat
    for seed, level, kw, tkw in ((41, 0, {}, {}), (42, 1, dict(bucket_size=13), dict(rgb=True)), (43, 2, dict(block_size=0.5), {}),
                                 (44, 1, dict(bucket_size=100000), dict(sh_upto=24)), (45, 5, dict(sh_level=1, bucket_size=3), {})):
        t = ksplat_numpy.random_table(3001, seed, **tkw)
        t["x"][::97] = np.nan
        t["rot_2"][5::89] = np.nan
        t["opacity"][3::71] = np.nan
        with np.errstate(all="ignore"):
            KSplatFormat().write(t, str(tmp_path / "r.ksplat"), compression_level=level, **kw)
        assert (tmp_path / "r.ksplat").read_bytes() == ksplat_numpy.file_bytes(t, level, **kw), seed


def test_plan_decides_degree_from_names_or_defers_to_the_device(writer):
    t = ksplat_numpy.random_table(10, 0)
    assert writer.plan(t)["degree"] is None and writer.plan(t)["scan"] == list(range(24))
    assert writer.plan(t, sh_level=1)["scan"] == list(range(9))
    assert writer.plan(t, sh_level=0)["degree"] == 0
    assert writer.plan(ksplat_numpy.random_table(10, 0, n_rest=0))["degree"] == 0
    assert [writer.degree_from_mask(m, s) for m, s in ((0, None), (1, None), (1 << 9, None), (3 | 1 << 23, None), (1 | 1 << 9, 1))] \
        == [0, 1, 0, 2, 1]


def test_errors_come_before_any_device_work(writer, gold, lib, tmp_path, monkeypatch):
    """the reference's exception types and messages for every error case, and TypeError for a field that is not little-endian
    float32 -- raised with the device path made unreachable, and no file created"""
    def boom(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(lib, "ksplat_pack_table", boom)
    monkeypatch.setattr(lib, "require_hip", boom)
    g, spec = gold
    path = tmp_path / "x.ksplat"
    n_err = 0
    for name, rec in spec.items():
        if "error" not in rec:
            continue
        with pytest.raises(ERRORS[rec["error"][0]]) as e:
            writer.write_ksplat(_table(g, spec, name), str(path), rec["level"], **rec.get("kw", {}))
        assert str(e.value) == rec["error"][1], name
        assert not path.exists(), name
        n_err += 1
    assert n_err >= 11
    t = ksplat_numpy.random_table(10, 1)
    for f, dt in (("opacity", "<f8"), ("rot_1", ">f4"), ("f_rest_3", "<f2"), ("x", "<i4")):
        bad = np.zeros(10, [(n, dt if n == f else t.dtype[n]) for n in t.dtype.names])
        with pytest.raises(TypeError, match=f):
            writer.write_ksplat(bad, str(path))
    assert not path.exists()


def test_empty_tables_need_no_device(writer, gold, lib, tmp_path, monkeypatch):
    g, spec = gold
    monkeypatch.setattr(lib, "ksplat_pack_table", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device touched")))
    for lv in (0, 1, 2):
        name = f"n0_l{lv}"
        writer.write_ksplat(_table(g, spec, name), str(tmp_path / "e.ksplat"), lv)
        assert (tmp_path / "e.ksplat").read_bytes() == g[name].tobytes()
        assert len(g[name]) == 5120


def test_host_exp_twin_equals_numpy(lib):
    """csrc/np_exp.h compiled for the host: 2^22 strided bit patterns + the probe vector, bit for bit"""
    x = (np.arange(1 << 22, dtype=np.uint64) * 1023 + 7).astype(np.uint32).view(np.float32)
    x = np.concatenate([x, lib.np_exp_probe_vector(), np.random.default_rng(3).uniform(-104, 89, 1 << 20).astype(np.float32)])
    with np.errstate(all="ignore"):
        want = np.exp(x).view(np.uint32)
    got = lib.np_exp_host(x).view(np.uint32)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert lib.np_exp_probe() is True


def test_failed_probe_warns_or_raises(lib, monkeypatch):
    monkeypatch.setattr(lib, "_np_exp_checked", None)
    def off_by_one_ulp(x):
        with np.errstate(all="ignore"):
            return np.nextafter(np.exp(x), np.float32(np.inf))
    monkeypatch.setattr(lib, "np_exp_host", off_by_one_ulp)
    monkeypatch.setenv("GSX_STRICT_NUMPY", "1")
    with pytest.raises(lib.GsxError, match="exp"):
        lib.np_exp_probe()
    monkeypatch.delenv("GSX_STRICT_NUMPY")
    with pytest.warns(RuntimeWarning, match="exp"):
        assert lib.np_exp_probe() is False
    monkeypatch.setattr(lib, "_np_exp_checked", None)


@pytest.mark.parametrize("level", [0, 1, 2])
def test_host_patch_of_listed_rows_and_buckets_is_the_restatement(lib, level):
    """numpy's own expressions for the rows (NaN casts) and buckets (NaN or mixed-zero centres) the device lists"""
    t = ksplat_numpy.edge_table()
    for bs in (7, 256):
        want = ksplat_numpy.file_bytes(t, level, bucket_size=bs)
        n = len(t)
        sc = 24
        nb = -(-n // bs)
        head = 5120 + (4 if n % bs else 0)
        cen_want = np.frombuffer(want[head:head + 12 * nb], "<f4").reshape(nb, 3) if level else None
        base = head + (12 * nb if level else 0)
        dt = lib.ksplat_row_dtype(level, sc)
        rows_want = np.frombuffer(want[base:], dt)
        if level:
            cen = lib.ksplat_centres_host(t, bs)
            assert cen.tobytes() == cen_want.tobytes()
        pick = np.arange(0, n, 3)
        got = lib.ksplat_rows_host(t, pick, level, sc, cen_want, bs, 32767 / (5.0 / 2.0))
        assert got.tobytes() == rows_want[pick].tobytes(), (level, bs)


def test_zero_sign_of_an_all_zero_bucket_is_numpys(lib):
    """the device sends such buckets to the host, whose numpy reduction decides the centre's sign (pinned here)"""
    for v in ([0.0, -0.0], [-0.0, 0.0], [0.0] * 300, [-0.0] * 300, [0.0, -0.0] * 200):
        t = np.zeros(len(v), ksplat_numpy.dtype_3dgs())
        t["x"] = np.array(v, np.float32)
        c = lib.ksplat_centres_host(t, 1000)[0, 0]
        s = np.minimum.reduceat(t["x"], [0]) + np.maximum.reduceat(t["x"], [0])
        assert np.float32(c).tobytes() == np.float32(s[0] / 2.0).tobytes()


_STANDIN = {
    "gsconverter/__init__.py": "",
    "gsconverter/processing/__init__.py": "from . import gpu_ops\nfrom .data_processor import DataProcessor\n",
    "gsconverter/processing/gpu_ops.py": "HAS_TAICHI = False\n",
    "gsconverter/processing/data_processor.py": "class DataProcessor:\n    def __init__(self, data):\n        self.data = data\n",
    "gsconverter/converter.py": "from .processing import DataProcessor\n",
    "gsconverter/formats/__init__.py": "",
    "gsconverter/formats/ksplat.py": ("class KSplatFormat:\n    def write(self, data, path, compression_level=0, **kw):\n"
                                      "        return 'own'\n"),
}


def test_install_rebinds_ksplat_write_on_a_stand_in_and_uninstall_restores_it(gsx, tmp_path, monkeypatch):
    for rel, src in _STANDIN.items():
        (tmp_path / rel).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / rel).write_text(src)
    saved = {m: sys.modules.pop(m) for m in list(sys.modules) if m == "gsconverter" or m.startswith("gsconverter.")}
    mine = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    monkeypatch.setattr(mine, "_REFERENCE_CLASS", None)
    monkeypatch.syspath_prepend(str(tmp_path))
    writer = importlib.import_module("3dgsconverter_amd.formats.ksplat_writer")
    try:
        import gsconverter.formats.ksplat as rks
        own = rks.KSplatFormat.write
        calls = []
        monkeypatch.setattr(writer, "write_ksplat", lambda data, path, level=0, **kw: calls.append((len(data), path, level, kw)) or "mine")
        try:
            gsx.install(ksplat_writer=False)
            assert rks.KSplatFormat.write is own
            gsx.uninstall()
            gsx.install()
            assert rks.KSplatFormat.write is not own
            assert rks.KSplatFormat().write(np.zeros(3), "a.ksplat", compression_level=2, bucket_size=7) == "mine"
            assert rks.KSplatFormat().write(np.zeros(2), "b.ksplat", 1) == "mine"
            assert calls == [(3, "a.ksplat", 2, {"bucket_size": 7}), (2, "b.ksplat", 1, {})]
        finally:
            gsx.uninstall()
        assert rks.KSplatFormat.write is own
    finally:
        for m in [m for m in sys.modules if m == "gsconverter" or m.startswith("gsconverter.")]:
            del sys.modules[m]
        sys.modules.update(saved)
