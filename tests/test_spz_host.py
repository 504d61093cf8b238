"""-m "not gpu": the SPZ writer's host side -- the numpy restatement against the reference's payloads
(tests/golden/spz_ref.npz, and a live run when the reference is mounted), the host's checks and errors before any device
work, the host patch of the rotation words the device lists, and the install() binding."""
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spz_numpy  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "spz_ref.npz")


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return g, json.loads(bytes(g["spec"]).decode())


@pytest.fixture(scope="module")
def writer():
    return importlib.import_module("3dgsconverter_amd.formats.spz_writer")


def _table(g, spec, name):
    return g["edges__table"] if name == "edges" else spz_numpy.case_table(spec[name])


def test_edge_rows_are_the_recorded_ones(gold):
    g, _ = gold
    assert spz_numpy.edge_table().tobytes() == g["edges__table"].tobytes()


def test_restatement_equals_every_golden_payload(gold):
    g, spec = gold
    assert len(spec) >= 16
    for name, rec in spec.items():
        t = _table(g, spec, name)
        if "error" in rec:
            with pytest.raises(ValueError) as e:
                spz_numpy.payload(t)
            assert str(e.value) == rec["error"], name
            continue
        got = spz_numpy.payload(t)
        assert got[12] == rec["degree"], name
        if name + "__sha256" in g:
            assert hashlib.sha256(got).digest() == g[name + "__sha256"].tobytes(), name
        else:
            assert got == g[name].tobytes(), name


@pytest.mark.skipif(not os.path.isdir("/root/reference/gsconverter"), reason="reference checkout not present")
def test_restatement_equals_a_live_reference_run(tmp_path):
    import gzip
    sys.path.insert(0, ROOT)
    from oracle import refload
    refload.load()
    from gsconverter.formats.spz import SpzFormat
    for seed, kw in ((21, {}), (22, dict(rgb=True)), (23, dict(sh_upto=24)), (24, dict(opacity=False, n_rest=45))):
        t = spz_numpy.random_table(3001, seed, **kw)
        t["x"][::97] = np.nan
        t["rot_2"][5::89] = np.nan
        with np.errstate(all="ignore"):
            SpzFormat().write(t, str(tmp_path / "r.spz"), compression_level=1)
        assert gzip.decompress((tmp_path / "r.spz").read_bytes()) == spz_numpy.payload(t), seed


def test_plan_decides_degree_or_defers_to_the_device(writer):
    t = spz_numpy.random_table(10, 0)
    assert writer.plan(t) == (None, list(range(44, -1, -1)))
    assert writer.plan(spz_numpy.random_table(10, 0, n_rest=0)) == (0, [])
    assert writer.plan(spz_numpy.random_table(10, 0, n_rest=9, sh_scale=0.0)) == (0, [])
    assert writer.plan(spz_numpy.random_table(10, 0, n_rest=24, sh_scale=0.0)) == (0, [])
    assert [writer.degree_from_last_index(i) for i in (-1, 0, 8, 9, 23, 24, 44)] == [0, 1, 1, 2, 2, 3, 3]


def test_errors_come_before_any_device_work(writer, gold, tmp_path, monkeypatch):
    """TypeError for a field that is not little-endian float32, numpy's ValueError for the tables the reference refuses --
    raised with the device path made unreachable, and no file created"""
    lib = importlib.import_module("3dgsconverter_amd._lib")

    def boom(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(lib, "spz_pack_table", boom)
    monkeypatch.setattr(lib, "require_hip", boom)
    g, spec = gold
    path = tmp_path / "x.spz"
    for name in ("c9_nonzero", "c24_nonzero", "c24_low"):
        with pytest.raises(ValueError) as e:
            writer.write_spz(_table(g, spec, name), str(path))
        assert str(e.value) == spec[name]["error"]
        assert not path.exists()
    t = spz_numpy.random_table(10, 1)
    for f, dt in (("opacity", "<f8"), ("rot_1", ">f4"), ("f_rest_30", "<f2"), ("x", "<i4")):
        bad = np.zeros(10, [(n, dt if n == f else t.dtype[n]) for n in t.dtype.names])
        with pytest.raises(TypeError, match=f):
            writer.write_spz(bad, str(path))
    no_x = np.zeros(3, [(n, t.dtype[n]) for n in t.dtype.names if n != "x"])
    with pytest.raises(ValueError, match="no field of name x"):
        writer.write_spz(no_x, str(path))
    no_dc1 = np.zeros(3, [(n, t.dtype[n]) for n in t.dtype.names if n != "f_dc_1"])
    with pytest.raises(ValueError, match="f_dc_1"):
        writer.write_spz(no_dc1, str(path))
    assert not path.exists()


def test_empty_table_and_zero_coefficient_tables_need_no_device(writer, gold, tmp_path, monkeypatch):
    import gzip
    g, spec = gold
    lib = importlib.import_module("3dgsconverter_amd._lib")
    monkeypatch.setattr(lib, "spz_pack_table", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device touched")))
    writer.write_spz(spz_numpy.case_table(spec["n0"]), str(tmp_path / "e.spz"), compression_level=0)
    assert gzip.decompress((tmp_path / "e.spz").read_bytes()) == g["n0"].tobytes()


def test_host_patch_of_listed_rotation_words_is_the_restatement(gold):
    """the rows with a NaN non-largest component: the device leaves their words to the host, which must find numpy's cast
    of a NaN at the position the reference's per-component array holds it"""
    lib = importlib.import_module("3dgsconverter_amd._lib")
    g, spec = gold
    for t in (g["edges__table"], spz_numpy.edge_table()[:7], spz_numpy.edge_table()[:300]):
        n = len(t)
        want = np.frombuffer(spz_numpy.payload(t), np.uint8)[16:]
        rot_want = want[16 * n:20 * n].view("<u4")
        q = np.stack([t[f"rot_{c}"] for c in range(4)], axis=1)
        with np.errstate(all="ignore"):
            norm = np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2 + q[:, 2] ** 2 + q[:, 3] ** 2 + np.float32(1e-9))
            r = np.stack([q[:, 1], q[:, 2], q[:, 3], q[:, 0]], axis=1) / norm[:, None]
        big = np.argmax(np.abs(r), axis=1)
        nan_other = np.array([np.isnan(np.delete(r[i], big[i])).any() for i in range(n)])
        rows = np.nonzero(nan_other)[0]
        assert len(rows) > 0
        rot = rot_want.copy()
        rot[rows] = 0x12345678          # what the device leaves there does not matter
        lib.spz_patch_rotations(rot, rows[::-1].copy(), q[rows[::-1]])
        assert np.array_equal(rot, rot_want)


def test_host_alpha_bytes_are_the_restatement():
    lib = importlib.import_module("3dgsconverter_amd._lib")
    t = spz_numpy.edge_table()
    want = np.frombuffer(spz_numpy.payload(t), np.uint8)[16 + 9 * len(t):16 + 10 * len(t)]
    assert np.array_equal(lib.spz_alpha_bytes(t["opacity"].copy()), want)


_STANDIN = {
    "gsconverter/__init__.py": "",
    "gsconverter/processing/__init__.py": "from . import gpu_ops\nfrom .data_processor import DataProcessor\n",
    "gsconverter/processing/gpu_ops.py": "HAS_TAICHI = False\n",
    "gsconverter/processing/data_processor.py": "class DataProcessor:\n    def __init__(self, data):\n        self.data = data\n",
    "gsconverter/converter.py": "from .processing import DataProcessor\n",
    "gsconverter/formats/__init__.py": "",
    "gsconverter/formats/spz.py": "class SpzFormat:\n    def write(self, data, path, **kw):\n        return 'own'\n",
}


def test_install_rebinds_spz_write_on_a_stand_in_and_uninstall_restores_it(gsx, tmp_path, monkeypatch):
    for rel, src in _STANDIN.items():
        (tmp_path / rel).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / rel).write_text(src)
    saved = {m: sys.modules.pop(m) for m in list(sys.modules) if m == "gsconverter" or m.startswith("gsconverter.")}
    mine = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    monkeypatch.setattr(mine, "_REFERENCE_CLASS", None)
    monkeypatch.syspath_prepend(str(tmp_path))
    writer = importlib.import_module("3dgsconverter_amd.formats.spz_writer")
    try:
        import gsconverter.formats.spz as rspz
        own = rspz.SpzFormat.write
        calls = []
        monkeypatch.setattr(writer, "write_spz", lambda data, path, **kw: calls.append((len(data), path, kw)) or "mine")
        try:
            gsx.install(spz_writer=False)
            assert rspz.SpzFormat.write is own
            gsx.uninstall()
            gsx.install()
            assert rspz.SpzFormat.write is not own
            assert rspz.SpzFormat().write(np.zeros(3), "a.spz", compression_level=4) == "mine"
            assert calls == [(3, "a.spz", {"compression_level": 4})]
        finally:
            gsx.uninstall()
        assert rspz.SpzFormat.write is own
    finally:
        for m in [m for m in sys.modules if m == "gsconverter" or m.startswith("gsconverter.")]:
            del sys.modules[m]
        sys.modules.update(saved)
