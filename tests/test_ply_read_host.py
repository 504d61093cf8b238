"""-m "not gpu": the 3DGS / CloudCompare PLY readers on the host -- the plan (output dtype, descriptors, identity, refusals)
against the golden file the reference's own readers made, the numpy restatement against the same file, the kernel's conversion
code run on the host (gsx_ply_unpack_host) against numpy, the exceptions raised before any device work
and the install() binding of both classes' `read`."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ply_read_numpy as pn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ply_read_ref.npz")
WANTED_CASES = {"canonical_deg3", "deg0", "deg1", "deg2", "cc_layout", "prefix_scal", "prefix_scalar_scal", "prefix_scalar_scal_nested",
                "opacity_and_scalar_opacity", "red_without_green", "missing_rot_3", "camera_before_vertex", "no_vertex", "zero_vertices",
                "shuffled", "every_source_type", "big_endian", "extras_of_every_type", "cc_extra_collides"}


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return g, json.loads(bytes(g["spec"]).decode())


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgsconverter_amd._lib")


@pytest.fixture(scope="module")
def reader():
    return importlib.import_module("3dgsconverter_amd.formats.ply_reader")


def _file(g, name, tmp_path):
    p = tmp_path / (name + ".ply")
    p.write_bytes(g[name + "__file"].tobytes())
    return str(p)


def _runs(spec):
    return [(name, dialect, r) for name, rec in spec.items() for dialect, r in rec["readers"].items()]


def _no_device(monkeypatch, lib):
    def refuse(*a, **k):
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(lib, "require_hip", refuse)
    monkeypatch.setattr(lib, "ply_unpack_table", refuse)


def _model_device(monkeypatch, lib, calls=None):
    """ply_unpack_table without a device: the same file bytes through the kernel's own field code on the host"""
    def model(path, body_offset, n, layout, dtype, stage_ms=None, device=0):
        if calls is not None:
            calls.append((path, n))
        with open(path, "rb") as f:
            f.seek(body_offset)
            body = np.empty(n * layout.in_stride, np.uint8)
            lib.read_exact(f, body, path, " in element 'vertex'")
        return lib.ply_unpack_host(body, n, layout, dtype)
    monkeypatch.setattr(lib, "ply_unpack_table", model)


def _read(reader, dialect):
    return reader.read_ply_3dgs if dialect == "3dgs" else reader.read_ply_cc


def test_golden_spec_covers_the_cases_the_feature_names(gold):
    g, spec = gold
    assert set(spec) == WANTED_CASES
    assert os.path.getsize(GOLD) < 1_000_000
    for name, dialect, r in _runs(spec):
        if "error" not in r:
            assert r["rows"] <= 300 and len(g["%s__%s__rows" % (name, dialect)]) == r["rows"] * r["itemsize"], name
    # the two readers differ where the feature says they do
    cc = spec["cc_layout"]["readers"]
    assert cc["3dgs"]["names"][-2:] == ["scalar_confidence", "scalar_label"] and cc["cc"]["names"][-2:] == ["confidence", "label"]
    assert cc["cc"]["dtype"][-2:] == ["<f4", "<i4"]
    assert spec["prefix_scal"]["readers"]["3dgs"]["itemsize"] == 248 < spec["prefix_scal"]["readers"]["cc"]["itemsize"]
    assert "green" in spec["red_without_green"]["readers"]["3dgs"]["names"]
    assert spec["cc_extra_collides"]["readers"]["cc"]["names"].count("opacity") == 1


def test_plan_dtype_equals_the_references_for_every_case(gold, reader, lib, tmp_path, monkeypatch):
    g, spec = gold
    _no_device(monkeypatch, lib)
    for name, dialect, r in _runs(spec):
        h = reader.parse_header(_file(g, name, tmp_path))
        if "error" in r:
            with pytest.raises(ValueError) as e:
                reader.plan(h, dialect)
            assert type(e.value).__name__ == r["error"]["type"] and str(e.value) == r["error"]["message"], name
            continue
        p = reader.plan(h, dialect)
        assert p.refusal is None, (name, dialect, p.refusal)
        assert list(p.dtype.names) == r["names"] and [p.dtype[f].str for f in p.dtype.names] == r["dtype"], (name, dialect)
        assert p.dtype.itemsize == r["itemsize"] == p.out_stride and p.count == r["rows"], (name, dialect)
        d = p.descriptors()
        assert len(d) == len(r["names"]) and sum(x[3] for x in d) == r["itemsize"]
        assert [x[2] for x in d] == [p.dtype.fields[f][1] for f in p.dtype.names]


def test_restatement_equals_every_golden_case(gold, tmp_path):
    g, spec = gold
    for name, dialect, r in _runs(spec):
        path = _file(g, name, tmp_path)
        if "error" in r:
            with pytest.raises(ValueError, match=r["error"]["message"]):
                pn.read(path, dialect)
            continue
        rows, others = pn.read(path, dialect)
        assert list(rows.dtype.names) == r["names"] and rows.tobytes() == g["%s__%s__rows" % (name, dialect)].tobytes(), (name, dialect)
        assert [n for n, _ in others] == r["extra_elements"]


def test_readers_through_the_kernels_field_code_on_the_host_equal_every_golden_case(gold, reader, lib, tmp_path, monkeypatch):
    g, spec = gold
    calls = []
    _model_device(monkeypatch, lib, calls)
    for name, dialect, r in _runs(spec):
        path = _file(g, name, tmp_path)
        if "error" in r:
            with pytest.raises(ValueError, match=r["error"]["message"]):
                _read(reader, dialect)(path)
            continue
        st = {}
        rows, extras = _read(reader, dialect)(path, stage_ms=st)
        assert list(rows.dtype.names) == r["names"] and [rows.dtype[f].str for f in rows.dtype.names] == r["dtype"], (name, dialect)
        assert rows.tobytes() == g["%s__%s__rows" % (name, dialect)].tobytes(), (name, dialect)
        assert [e.name for e in extras] == r["extra_elements"] and "parse" in st
        want_extras = dict(pn.read(path, dialect)[1])
        for e in extras:
            assert e.data.dtype == want_extras[e.name].dtype and e.data.tobytes() == want_extras[e.name].tobytes(), (name, e.name)
    # the canonical file (identity) and the empty one never reach the device
    assert not any("canonical_deg3" in p or "zero_vertices" in p for p, _ in calls) and all(n > 0 for _, n in calls)
    assert len(calls) == len([1 for n, d, r in _runs(spec) if "error" not in r and n not in ("canonical_deg3", "zero_vertices")])


def test_identity_plan_is_the_canonical_file_and_no_other(gold, reader, lib, tmp_path, monkeypatch):
    g, spec = gold
    _no_device(monkeypatch, lib)
    for name, dialect, r in _runs(spec):
        if "error" in r:
            continue
        p = reader.plan(reader.parse_header(_file(g, name, tmp_path)), dialect)
        assert p.identity == (name == "canonical_deg3"), (name, dialect)
    st = {}
    rows, extras = reader.read_ply_3dgs(_file(g, "canonical_deg3", tmp_path), stage_ms=st)      # no device: _no_device would raise
    assert rows.tobytes() == g["canonical_deg3__3dgs__rows"].tobytes() and extras == []
    assert "file_read" in st and not {"upload", "kernel", "download"} & set(st)
    rows, extras = reader.read_ply_cc(_file(g, "zero_vertices", tmp_path))
    assert len(rows) == 0 and rows.dtype.itemsize == 259 and [e.name for e in extras] == ["camera"] and len(extras[0].data) == 3


def _raw_file(tmp_path, name, header_lines, body=b""):
    p = tmp_path / name
    p.write_bytes(("\n".join(header_lines) + "\n").encode("ascii") + body)
    return str(p)


def _refusal_files(tmp_path):
    """-> [(path, a word of the reason)]"""
    rng = np.random.default_rng(5)
    std = ["property float %s" % f for f in pn.FLOAT_FIELDS]
    head = ["ply", "format binary_little_endian 1.0", "element vertex 2"]
    out = [(_raw_file(tmp_path, "ascii.ply", ["ply", "format ascii 1.0", "element vertex 1"] + std + ["end_header"],
                      (" ".join(["0"] * 59) + "\n").encode()), "ascii"),
           (_raw_file(tmp_path, "list.ply", head + std + ["property list uchar int idx", "end_header"], bytes(2 * 237)), "list property 'idx'"),
           (_raw_file(tmp_path, "list_elsewhere.ply", head + std + ["element face 1", "property list uchar int vertex_indices", "end_header"],
                      bytes(2 * 236 + 1)), "list property 'vertex_indices' of element 'face'"),
           (_raw_file(tmp_path, "twice.ply", head + std + ["property float opacity", "end_header"], bytes(2 * 240)), "'opacity' appears twice")]
    can = pn.canonical_fields(3)
    for c in pn.COLOURS:
        cols = [(k, "f4" if k == c else "u1") for k in pn.COLOURS]
        out.append((pn.write_ply(str(tmp_path / ("float_%s.ply" % c)), [("vertex", pn.build(3, can + cols, rng))]), "uchar colours"))
    out.append((pn.write_ply(str(tmp_path / "be_extra.ply"), [("vertex", pn.build(3, can + [("extra", "f4")], rng))], "binary_big_endian"),
                "big-endian body with extra fields (extra)"))
    wide_in = [(f, "f8") for f in pn.FLOAT_FIELDS] + [("red", "u1")] + [("e%d" % i, "f8") for i in range(2)]          # 496 + 1 + 16 = 513
    out.append((pn.write_ply(str(tmp_path / "in513.ply"), [("vertex", pn.build(3, [(f, t) for f, t in wide_in if f != "red"] + [("red", "u1")], rng))]),
                "rows of 513 bytes"))
    wide_out = pn.canonical_fields(0) + [("e%d" % i, "f8") for i in range(33)] + [("b", "u1")]                    # out: 248 + 264 + 1
    out.append((pn.write_ply(str(tmp_path / "out513.ply"), [("vertex", pn.build(3, wide_out, rng))]), "and 513 in the table"))
    many = pn.canonical_fields(3) + [("e%d" % i, "u1") for i in range(67)]                                            # 62 + 67 = 129 fields
    out.append((pn.write_ply(str(tmp_path / "fields129.ply"), [("vertex", pn.build(3, many, rng))]), "129 output fields"))
    return out


def test_every_refusal_raises_with_its_reason_or_goes_to_the_fallback(reader, lib, tmp_path, monkeypatch):
    _no_device(monkeypatch, lib)
    files = _refusal_files(tmp_path)
    assert len(files) == 11
    for path, reason in files:
        for read in (reader.read_ply_3dgs, reader.read_ply_cc):
            with pytest.raises(reader.UnsupportedPlyError) as e:
                read(path)
            assert reason in str(e.value) and path in str(e.value), (path, str(e.value))
            assert read(path, fallback=lambda p: ("the reference's", p)) == ("the reference's", path)
        p = reader.plan(reader.parse_header(path), "cc")
        assert p.refusal is not None and reason in p.refusal and not p.identity
    # what is NOT refused at the caps: 512-byte rows in and out, 128 fields (the device tests read them)
    rng = np.random.default_rng(6)
    ok = [[(f, "f8") for f in pn.FLOAT_FIELDS] + [("e%d" % i, "f8") for i in range(2)],
          pn.canonical_fields(0) + [("e%d" % i, "f8") for i in range(33)],
          pn.canonical_fields(3) + [("e%d" % i, "u1") for i in range(66)]]
    for k, fields in enumerate(ok):
        p = reader.plan(reader.parse_header(pn.write_ply(str(tmp_path / ("ok%d.ply" % k)), [("vertex", pn.build(3, fields, rng))])), "3dgs")
        assert p.refusal is None, p.refusal
        assert (p.in_stride, p.out_stride, len(p.fields))[k] == (512, 512, 128)[k]


def test_missing_vertex_non_ply_and_truncated_files_raise(gold, reader, lib, tmp_path, monkeypatch):
    g, spec = gold
    _model_device(monkeypatch, lib)
    for read in (reader.read_ply_3dgs, reader.read_ply_cc):
        with pytest.raises(ValueError) as e:
            read(_file(g, "no_vertex", tmp_path), fallback=lambda p: "never asked")
        assert str(e.value) == "PLY file does not contain 'vertex' element" and type(e.value) is ValueError
        not_ply = tmp_path / "not.ply"
        not_ply.write_bytes(b"solid cube\nfacet normal 0 0 1\n")
        with pytest.raises(reader.PlyHeaderError):
            read(str(not_ply))
        with pytest.raises(FileNotFoundError):
            read(str(tmp_path / "missing.ply"))
        for name in ("deg1", "canonical_deg3", "camera_before_vertex"):        # device path, identity path, an element before
            data = g[name + "__file"].tobytes()
            for cut in (1, 300):
                short = tmp_path / "short.ply"
                short.write_bytes(data[:-cut])
                with pytest.raises(ValueError, match="early end of file in element 'vertex'"):
                    read(str(short))
    data = g["zero_vertices__file"].tobytes()                                   # the camera element behind an empty vertex element
    (tmp_path / "short2.ply").write_bytes(data[:-5])
    with pytest.raises(ValueError, match="early end of file in element 'camera'"):
        reader.read_ply_cc(str(tmp_path / "short2.ply"))


def test_kernel_field_code_on_the_host_equals_numpy_for_every_source_type_and_byte_order(reader, lib, tmp_path, monkeypatch):
    _model_device(monkeypatch, lib)
    for typ in pn.SOURCE_TYPES:
        table = pn.type_matrix_table(typ)
        for fmt in ("binary_little_endian", "binary_big_endian"):
            path = pn.write_ply(str(tmp_path / "m.ply"), [("vertex", table)], fmt)
            for dialect in ("3dgs", "cc"):
                rows, _ = _read(reader, dialect)(path)
                want, _ = pn.read(path, dialect)
                assert rows.dtype == want.dtype and rows.tobytes() == want.tobytes(), (typ, fmt, dialect)
    # the cases the feature spells out, by their bits: what numpy gives here is what the device tests hold the kernel to
    bits = {0x7ff0000000000001: 0x7fc00000, 0xfff4000000000000: 0xffe00000, 0x47effffff0000000: 0x7f800000, 0x47efffffefffffff: 0x7f7fffff,
            0x3690000000000000: 0, 0x3690000000000001: 1, 0xb680000000000000: 0x80000000, 0x36a0000000000000: 1, 0x3810000000000000: 0x00800000}
    ev = pn.edge_values("f8")
    assert set(bits) <= set(int(b) for b in ev.view(np.uint64))                 # ... and the type matrix holds every one of them
    with np.errstate(all="ignore"):
        got = np.array(list(bits), np.uint64).view(np.float64).astype(np.float32).view(np.uint32)
    assert [int(x) for x in got] == list(bits.values())


def test_random_layouts_through_the_kernels_field_code_on_the_host(reader, lib, tmp_path, monkeypatch):
    _model_device(monkeypatch, lib)
    for seed in range(20):
        table, dialect = pn.random_layout(seed, 100)
        path = pn.write_ply(str(tmp_path / "r.ply"), [("vertex", table)], body_mod16=seed % 16)
        rows, _ = _read(reader, dialect)(path)
        want, _ = pn.read(path, dialect)
        assert rows.dtype == want.dtype and rows.tobytes() == want.tobytes(), seed


_STANDIN = {
    "gsconverter/__init__.py": "",
    "gsconverter/processing/__init__.py": "from . import gpu_ops\nfrom .data_processor import DataProcessor\n",
    "gsconverter/processing/gpu_ops.py": "HAS_TAICHI = False\n",
    "gsconverter/processing/data_processor.py": "class DataProcessor:\n    def __init__(self, data):\n        self.data = data\n",
    "gsconverter/converter.py": "from .processing import DataProcessor\n",
    "gsconverter/formats/__init__.py": "",
    "gsconverter/formats/ply_3dgs.py": "class Ply3DGSFormat:\n    def read(self, path, **kw):\n        return ('own 3dgs', path, kw)\n",
    "gsconverter/formats/ply_cc.py": "class PlyCCFormat:\n    def read(self, path, **kw):\n        return ('own cc', path, kw)\n",
}


def test_install_binds_both_reads_on_a_stand_in_and_uninstall_restores_them(gsx, gold, reader, lib, tmp_path, monkeypatch):
    g, spec = gold
    for rel, src in _STANDIN.items():
        (tmp_path / rel).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / rel).write_text(src)
    saved = {m: sys.modules.pop(m) for m in list(sys.modules) if m == "gsconverter" or m.startswith("gsconverter.")}
    mine = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    monkeypatch.setattr(mine, "_REFERENCE_CLASS", None)
    monkeypatch.syspath_prepend(str(tmp_path))
    _model_device(monkeypatch, lib)
    monkeypatch.setattr(reader, "plyfile_available", lambda: False)
    try:
        import gsconverter.formats.ply_3dgs as r3
        import gsconverter.formats.ply_cc as rcc
        own3, owncc = r3.Ply3DGSFormat.read, rcc.PlyCCFormat.read
        try:
            gsx.install(ply_reader=False)
            assert r3.Ply3DGSFormat.read is own3 and rcc.PlyCCFormat.read is owncc
            gsx.uninstall()
            gsx.install()
            assert r3.Ply3DGSFormat.read is not own3 and rcc.PlyCCFormat.read is not owncc
            assert r3.Ply3DGSFormat.read.__wrapped__ is own3 and rcc.PlyCCFormat.read.__wrapped__ is owncc
            for cls, dialect in ((r3.Ply3DGSFormat, "3dgs"), (rcc.PlyCCFormat, "cc")):
                fmt = cls()
                rows = fmt.read(_file(g, "cc_layout", tmp_path), anything=1)
                assert rows.tobytes() == g["cc_layout__%s__rows" % dialect].tobytes() and fmt.extra_elements == []
                fmt = cls()
                rows = fmt.read(_file(g, "camera_before_vertex", tmp_path))
                assert [(e.name, len(e.data)) for e in fmt.extra_elements] == [("camera", 3)]
                with pytest.raises(reader.UnsupportedPlyError):                # no plyfile: nothing to hand a refused file to
                    cls().read(_refusal_files(tmp_path)[0][0])
            monkeypatch.setattr(reader, "plyfile_available", lambda: True)     # with plyfile a refused file goes to the reference's read
            monkeypatch.setitem(sys.modules, "plyfile", type(sys)("plyfile"))
            assert r3.Ply3DGSFormat().read(_refusal_files(tmp_path)[0][0], k=2)[0] == "own 3dgs"
        finally:
            gsx.uninstall()
        assert r3.Ply3DGSFormat.read is own3 and rcc.PlyCCFormat.read is owncc
    finally:
        for m in [m for m in sys.modules if m == "gsconverter" or m.startswith("gsconverter.")]:
            del sys.modules[m]
        sys.modules.update(saved)


def test_golden_file_regenerates_identically_when_the_reference_is_there(tmp_path):
    from oracle import refload
    if not refload.available():
        pytest.skip("the reference is not mounted")
    env = dict(os.environ, PYTHONWARNINGS="ignore")
    code = ("import sys, runpy; sys.path.insert(0, %r); m = runpy.run_path(%r); m['main'].__globals__['OUT'] = %r; m['main']()"
            % (ROOT, os.path.join(ROOT, "tests", "devtools", "make_golden_ply_read.py"), str(tmp_path / "again.npz")))
    subprocess.run([sys.executable, "-c", code], check=True, env=env, capture_output=True, cwd=ROOT)
    a, b = np.load(GOLD), np.load(str(tmp_path / "again.npz"))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
