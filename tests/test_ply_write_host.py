"""-m "not gpu": the 3DGS / CloudCompare PLY writers on the host -- the numpy restatement against the golden files the reference's
own writers made, the plan (property list, runs, identity, refusals) against the same files, the kernel's run code on the host
(gsx_ply_pack_host) against their rows, both writers end to end with that code in the device's place, the refusals with their
reasons, the paths that must not ask for a device, and the install() binding of both classes' `write`."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ply_read_numpy as pn  # noqa: E402
import ply_write_numpy as pw  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ply_write_ref.npz")
BOTH = ("3dgs", "cc")
WANTED_CASES = {"canonical_deg3", "canonical_rgb", "rgb_no_normals", "rgb_crop_8", "deg0", "deg1", "deg2", "deg0_crop", "deg1_crop", "deg2_crop",
                "no_normals", "holes", "shuffled", "noncontiguous", "extras", "extras_crop", "red_without_green", "green_without_red",
                "no_opacity", "f8_rest_3", "f8_rest_3_crop", "zero_rows", "zero_rows_crop", "extra_elements", "extra_elements_zero_rows",
                "crop_last_m1", "crop_last_0", "crop_last_5", "crop_last_8", "crop_last_9", "crop_last_23", "crop_last_24", "crop_last_44"}
# the table's rows are the file's rows already (after the crop scan where there is one): nothing is packed
IDENTITY = {"canonical_deg3", "canonical_rgb", "deg0_crop", "deg1_crop", "deg2_crop", "crop_last_44", "extra_elements_zero_rows"}
EMPTY = {"zero_rows", "zero_rows_crop", "extra_elements_zero_rows"}
WANTED_ROWS = {1, 63, 64, 65, 127, 128, 129, 300}
WANTED_LAST_IDX = {-1, 0, 5, 8, 9, 23, 24, 44}


@pytest.fixture(scope="module")
def cases():
    return pw.load_cases(GOLD)


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgsconverter_amd._lib")


@pytest.fixture(scope="module")
def writer():
    return importlib.import_module("3dgsconverter_amd.formats.ply_writer")


def _write(writer, dialect):
    return writer.write_ply_3dgs if dialect == "3dgs" else writer.write_ply_cc


def _plan(writer, case, dialect):
    return writer.plan_write(case.table.dtype, dialect, case.crop_sh, case.writers[dialect].get("last_idx"))


def _no_device(monkeypatch, lib):
    def refuse(*a, **k):
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(lib, "require_hip", refuse)
    monkeypatch.setattr(lib, "ply_pack_table", refuse)


def _model_device(monkeypatch, lib, calls=None):
    """ply_pack_table without a device: the scan's meaning in numpy, the rows through the kernel's own run code on the host"""
    def model(data, plan_of, scan=None, stage_ms=None, device=0):
        assert data.flags.c_contiguous and len(data) >= 1
        last = None
        if scan is not None:
            offsets, present = scan
            raw = data.view(np.uint8).reshape(len(data), -1)
            hit = [i for i in range(45) if (present >> i) & 1
                   and np.any(np.ascontiguousarray(raw[:, offsets[i]:offsets[i] + 4]).view("<u4") & 0x7fffffff)]
            last = max(hit) if hit else -1
        plan = plan_of(last)
        if calls is not None:
            calls.append((len(data), scan is not None, plan.identity))
        if plan.refusal is not None or plan.identity:
            return plan, None
        if stage_ms is not None:
            stage_ms["pack"] = 0.0
        return plan, lib.ply_pack_host(data, plan.layout())
    monkeypatch.setattr(lib, "ply_pack_table", model)


def test_golden_spec_covers_the_cases_the_feature_names(cases):
    assert set(cases) == WANTED_CASES
    assert os.path.getsize(GOLD) < 1_000_000
    assert {len(c.table) for c in cases.values()} - {0} == WANTED_ROWS
    assert {w["last_idx"] for c in cases.values() for w in c.writers.values() if "last_idx" in w} >= WANTED_LAST_IDX
    for c in cases.values():
        assert set(c.writers) == set(BOTH) and len(c.table) <= 300, c.name
    names = lambda case, d: [p[1] for p in cases[case].writers[d]["properties"]]   # noqa: E731
    types = lambda case, d: dict((p[1], p[0]) for p in cases[case].writers[d]["properties"])   # noqa: E731
    # the points of the contract, each where its case shows it
    assert cases["canonical_rgb"].table.dtype.itemsize == 251 and not cases["noncontiguous"].table.flags.c_contiguous
    assert cases["holes"].table.dtype.itemsize > sum(cases["holes"].table.dtype[f].itemsize for f in cases["holes"].table.dtype.names)
    assert names("no_normals", "3dgs")[:7] == ["x", "y", "z", "nx", "ny", "nz", "f_dc_0"]
    assert "f_rest_44" in names("deg0", "3dgs") and "scalar_f_rest_44" in names("deg0", "cc")                # padded, and prefixed
    assert not any("f_rest" in n for n in names("deg0_crop", "3dgs")) and names("deg1_crop", "cc")[-9] == "scalar_f_rest_8"
    assert names("crop_last_5", "3dgs")[9:16] == ["f_rest_%d" % i for i in range(6)] + ["opacity"]           # a cut by index: six coefficients
    assert "green" not in names("red_without_green", "3dgs") and names("red_without_green", "cc")[-2:] == ["red", "blue"]
    assert "green" not in names("green_without_red", "3dgs") and "scalar_green" not in names("green_without_red", "cc")
    assert "opacity" not in names("no_opacity", "3dgs") and "scalar_opacity" not in names("no_opacity", "cc")
    assert types("f8_rest_3", "3dgs")["f_rest_3"] == "double" and types("f8_rest_3_crop", "cc")["scalar_f_rest_3"] == "double"
    assert [types("extras", "3dgs")["e_" + t] for t in pn.SOURCE_TYPES] == [pn.NAMES[t] for t in pn.SOURCE_TYPES]
    assert names("extras", "cc")[-8:] == ["scalar_e_" + t for t in pn.SOURCE_TYPES]
    assert [e.data.dtype[1].str[0] for e in cases["extra_elements"].extras] == [">", "<"] and len(cases["extra_elements"].extras[1].data) == 0
    # the deciding values of the crop scan, in the forms the feature names
    rest = lambda case, i: cases[case].table["f_rest_%d" % i]   # noqa: E731
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)   # noqa: E731
    assert np.count_nonzero(bits(rest("crop_last_0", 0))) == 1 and rest("crop_last_0", 0)[0] != 0
    assert np.count_nonzero(bits(rest("crop_last_5", 5))) == 1 and rest("crop_last_5", 5)[299] != 0 and 299 % 128 != 127
    assert np.isnan(rest("crop_last_9", 9)).sum() == 1 and np.count_nonzero(bits(rest("crop_last_9", 9))) == 1
    assert sorted(set(bits(rest("crop_last_23", 23)).tolist())) == [0, 1]
    assert set(bits(rest("crop_last_8", 9)).tolist()) == {0x80000000} and set(bits(rest("crop_last_m1", 0)).tolist()) == {0x80000000}


def test_restatement_equals_every_golden_file(cases):
    for c in cases.values():
        for d in BOTH:
            dtype, rows, blob, last_idx = pw.write(c.table, d, c.crop_sh, c.extras)
            w = c.writers[d]
            assert blob == c.files[d] and rows == c.vertex_rows(d), (c.name, d)
            assert pw.properties(dtype) == w["properties"] and dtype.itemsize == w["itemsize"] and last_idx == w.get("last_idx"), (c.name, d)


def test_plan_gives_the_references_property_list_for_every_case(cases, writer, lib, monkeypatch):
    _no_device(monkeypatch, lib)
    for c in cases.values():
        for d in BOTH:
            p = _plan(writer, c, d)
            w = c.writers[d]
            assert p.refusal is None, (c.name, d, p.refusal)
            assert [list(x) for x in p.properties] == w["properties"] and p.out_stride == w["itemsize"] == p.dtype.itemsize, (c.name, d)
            assert p.in_stride == c.table.dtype.itemsize and p.dtype.isnative and not p.dtype.hasobject
            assert [f.dst_offset for f in p.fields] == [p.dtype.fields[n][1] for n in p.dtype.names]
            assert p.identity == (c.name in IDENTITY), (c.name, d)
    # the canonical tables are a few runs a row, not 62 fields
    for name, runs in (("canonical_deg3", 1), ("deg0", 3), ("no_normals", 3), ("rgb_no_normals", 3), ("crop_last_5", 2), ("rgb_crop_8", 2), ("holes", 4)):
        assert len(_plan(writer, cases[name], "3dgs").runs) == runs, name
    with pytest.raises(ValueError, match="crop_sh needs last_idx"):
        writer.plan_write(cases["deg1"].table.dtype, "3dgs", True)
    with pytest.raises(ValueError, match="dialect"):
        writer.plan_write(cases["deg1"].table.dtype, "ply")


def test_runs_cover_every_output_byte_exactly_once(cases, writer):
    for c in cases.values():
        for d in BOTH:
            p = _plan(writer, c, d)
            covered = np.zeros(p.out_stride, np.int64)
            taken = np.zeros(p.in_stride, np.int64)
            for so, do, nb in p.runs:
                assert nb >= 1 and 0 <= do and do + nb <= p.out_stride and (so is None or (0 <= so and so + nb <= p.in_stride)), (c.name, d)
                covered[do:do + nb] += 1
                if so is not None:
                    taken[so:so + nb] += 1
            assert covered.tolist() == [1] * p.out_stride and taken.max(initial=0) <= 1, (c.name, d)
            assert sum(nb for _, _, nb in p.runs) == sum(f.nbytes for f in p.fields) == p.out_stride
            assert writer.merge_runs(p.entries()) == p.runs and len(p.runs) <= lib_runs(writer)
            lay = p.layout()
            assert (lay.in_stride, lay.out_stride, lay.n_runs) == (p.in_stride, p.out_stride, len(p.runs))
            assert [(lay.src_offset[k], lay.dst_offset[k], lay.bytes[k]) for k in range(lay.n_runs)] == [(-1 if s is None else s, t, b) for s, t, b in p.runs]


def lib_runs(writer):
    return writer.MAX_RUNS


def test_kernels_run_code_on_the_host_gives_the_golden_rows(cases, writer, lib):
    assert lib.PLY_WRITE_MAX_RUNS >= 128
    for c in cases.values():
        if c.name in EMPTY:
            continue
        table = np.ascontiguousarray(c.table)
        for d in BOTH:
            p = _plan(writer, c, d)
            got = lib.ply_pack_host(table, p.layout())
            assert got.tobytes() == c.vertex_rows(d), (c.name, d)


def test_run_code_on_the_host_at_every_alignment_and_both_tile_shapes(writer, lib):
    """synthetic tables against the restatement: runs that start and end at every byte phase on both sides, rows of 1 byte and
    of 512, more rows than a tile of 128 (strides up to 256) and of 64 (above)"""
    rng = np.random.default_rng(7)
    layouts = [[("e", "u1")],
               [("a", "u1"), ("x", "f4"), ("b", "u2"), ("y", "f4"), ("c", "u1"), ("z", "f8"), ("opacity", "f4"), ("d", "u1")],
               [("k%d" % i, "u1") for i in range(3)] + pn.canonical_fields(3) + [("t%d" % i, "f8") for i in range(30)] + [("w", "u1")],
               [("t0", "f8")] + pn.canonical_fields(3) + [("t%d" % i, "f8") for i in range(1, 33)]]
    for fields in layouts:
        for n in (1, 65, 130):
            t = pn.build(n, fields, rng)
            for d in BOTH:
                for crop in (False, True):
                    dtype, rows, _, last = pw.write(t, d, crop)
                    p = writer.plan_write(t.dtype, d, crop, last)
                    assert p.refusal is None and p.dtype == dtype, (fields[0], d, crop, p.refusal)
                    assert lib.ply_pack_host(t, p.layout()).tobytes() == rows, (fields[0], n, d, crop)
    assert pn.build(1, layouts[3], rng).dtype.itemsize == 512


def test_both_writers_end_to_end_with_the_run_code_in_the_devices_place(cases, writer, lib, tmp_path, monkeypatch):
    calls = []
    _model_device(monkeypatch, lib, calls)
    for c in cases.values():
        for d in BOTH:
            calls.clear()
            st = {}
            path = str(tmp_path / ("%s_%s.ply" % (c.name, d)))
            plan = _write(writer, d)(c.table, path, stage_ms=st, **c.kwargs)
            with open(path, "rb") as f:
                assert f.read() == c.files[d], (c.name, d)
            assert plan.last_idx == c.writers[d].get("last_idx"), (c.name, d)
            packed = c.name not in IDENTITY and c.name not in EMPTY
            assert ("pack" in st) == packed and "file_write" in st, (c.name, d, st)
            scans = c.crop_sh and len(c.table) > 0 and any(f.startswith("f_rest_") for f in c.table.dtype.names) and "f8" not in c.name
            assert len(calls) == (1 if packed or scans else 0) and all(call[1] == scans for call in calls), (c.name, d, calls)


def test_identity_and_empty_tables_ask_for_no_device(cases, writer, lib, tmp_path, monkeypatch):
    _no_device(monkeypatch, lib)
    for name in ("canonical_deg3", "canonical_rgb", "deg0_crop", "zero_rows", "zero_rows_crop", "extra_elements_zero_rows"):
        c = cases[name]
        for d in BOTH:
            st = {}
            path = str(tmp_path / ("%s_%s.ply" % (name, d)))
            _write(writer, d)(c.table, path, stage_ms=st, **c.kwargs)
            with open(path, "rb") as f:
                assert f.read() == c.files[d], (name, d)
            assert not {"upload", "pack", "download"} & set(st) and {"plan", "file_write"} <= set(st), (name, d, st)


def test_messages_are_the_references(cases, writer, lib, tmp_path, monkeypatch, capsys):
    _model_device(monkeypatch, lib)
    said = []
    monkeypatch.setattr(writer, "status_print", lambda *a, **k: said.append(("status", a[0])))
    monkeypatch.setattr(writer, "debug_print", lambda *a, **k: said.append(("debug", a[0])))
    c = cases["extra_elements"]
    writer.write_ply_3dgs(c.table, str(tmp_path / "a.ply"), **c.kwargs)
    assert ("status", "Maintained 2 extra PLY elements.") in said and said[-1] == ("status", "3DGS PLY write completed. 1 points.")
    assert capsys.readouterr().out == ""
    said.clear()
    writer.write_ply_cc(c.table, str(tmp_path / "b.ply"), **c.kwargs)
    assert capsys.readouterr().out == "Maintained 2 extra PLY elements.\n"                          # ply_cc.py:129: plain print
    assert said[-1] == ("debug", "CloudCompare PLY write completed. 1 points.") and not [s for s in said if s[0] == "status"]
    said.clear()
    writer.write_ply_3dgs(cases["crop_last_9"].table, str(tmp_path / "c.ply"), crop_sh=True)
    assert ("debug", "[DEBUG] crop_sh=True. Detected last active SH index: 9") in said


def _refusals():
    """-> [(case name, table, crop_sh, the words its refusal must hold)]"""
    base = pn.canonical_fields(0)
    out = [("half_extra", np.zeros(4, [(f, "<f4") for f, _ in base] + [("h", "<f2")]), False, "field 'h' is float16"),
           ("int64_extra", np.zeros(4, [(f, "<f4") for f, _ in base] + [("id", "<i8")]), False, "field 'id' is int64"),
           ("bool_extra", np.zeros(4, [(f, "<f4") for f, _ in base] + [("keep", "?")]), False, "field 'keep' is bool"),
           ("subarray_extra", np.zeros(4, [(f, "<f4") for f, _ in base] + [("v", "<f4", (3,))]), False, "field 'v' is"),
           ("big_endian_x", np.zeros(4, [(f, ">f4" if f == "x" else "<f4") for f, _ in base]), False, "field 'x' is big-endian"),
           ("wide_table", np.zeros(4, pn.canonical_fields(3) + [("t%d" % i, "<f8") for i in range(34)]), False, "rows of 520 bytes in the table and 520 in the file"),
           ("wide_file", np.zeros(4, [f for f in pn.canonical_fields(3) if f[0] not in ("nx", "ny", "nz")] + [("t%d" % i, "<f8") for i in range(34)]), False,
            "rows of 508 bytes in the table and 520 in the file"),
           ("many_runs", np.zeros(4, np.dtype({"names": ["x"] + ["e%d" % i for i in range(200)], "formats": ["<f4"] + ["u1"] * 200,
                                               "offsets": [0] + [4 + 2 * i for i in range(200)], "itemsize": 404})), False, "202 runs a row"),
           # a field that crop_sh drops is never written: its type does not matter
           ]
    return out


def test_refusals_raise_their_reasons(writer, lib, tmp_path, monkeypatch):
    _no_device(monkeypatch, lib)
    monkeypatch.setattr(writer, "plyfile_available", lambda: False)
    for name, table, crop, words in _refusals():
        for d in BOTH:
            p = writer.plan_write(table.dtype, d, crop, -1 if crop else None)
            assert p.refusal is not None and words in p.refusal and not p.identity, (name, d, p.refusal)
            path = str(tmp_path / (name + ".ply"))
            with pytest.raises(writer.UnsupportedPlyError, match=words.split("(")[0]):
                _write(writer, d)(table, path, crop_sh=crop)
            assert not os.path.exists(path)
            taken = []
            assert _write(writer, d)(table, path, fallback=lambda: taken.append(name) or "reference", crop_sh=crop) == "reference" and taken == [name]
    # a dropped field is never written, whatever its type: no refusal
    base = [(f, "<f4") for f, _ in pn.canonical_fields(0)]
    assert writer.plan_write(np.dtype(base + [("green", "<i8")]), "3dgs").refusal is None
    assert writer.plan_write(np.dtype(base + [("f_rest_7", "<f2")]), "cc", True, -1).refusal is None
    assert "f_rest_7" in writer.plan_write(np.dtype(base + [("f_rest_7", "<f2")]), "cc", False).refusal
    with pytest.raises(ValueError, match="1-D structured table"):
        writer.write_ply_3dgs(np.zeros((2, 3), np.float32), str(tmp_path / "plain.ply"))


def test_a_table_refused_after_the_scan_goes_to_the_fallback(writer, lib, tmp_path, monkeypatch):
    """crop_sh on float32 f_rest fields: the plan is made from the scan's answer, inside the session"""
    _model_device(monkeypatch, lib)
    monkeypatch.setattr(writer, "plyfile_available", lambda: False)
    t = np.zeros(5, [(f, "<f4") for f, _ in pn.canonical_fields(1)] + [("h", "<f2")])
    with pytest.raises(writer.UnsupportedPlyError, match="field 'h' is float16"):
        writer.write_ply_cc(t, str(tmp_path / "h.ply"), crop_sh=True)
    assert writer.write_ply_cc(t, str(tmp_path / "h.ply"), crop_sh=True, fallback=lambda: "reference") == "reference"


_STANDIN = {
    "gsconverter/__init__.py": "",
    "gsconverter/processing/__init__.py": "from . import gpu_ops\nfrom .data_processor import DataProcessor\n",
    "gsconverter/processing/gpu_ops.py": "HAS_TAICHI = False\n",
    "gsconverter/processing/data_processor.py": "class DataProcessor:\n    def __init__(self, data):\n        self.data = data\n",
    "gsconverter/converter.py": "from .processing import DataProcessor\n",
    "gsconverter/formats/__init__.py": "",
    "gsconverter/formats/ply_3dgs.py": ("class Ply3DGSFormat:\n    def read(self, path, **kw):\n        return ('own 3dgs', path, kw)\n"
                                        "    def write(self, data, path, **kw):\n        open(path, 'w').write('own 3dgs ' + ' '.join(sorted(kw)))\n"),
    "gsconverter/formats/ply_cc.py": ("class PlyCCFormat:\n    def read(self, path, **kw):\n        return ('own cc', path, kw)\n"
                                      "    def write(self, data, path, **kw):\n        open(path, 'w').write('own cc ' + ' '.join(sorted(kw)))\n"),
}


def test_install_binds_both_writes_on_a_stand_in_and_uninstall_restores_them(gsx, cases, writer, lib, tmp_path, monkeypatch):
    for rel, src in _STANDIN.items():
        (tmp_path / rel).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / rel).write_text(src)
    saved = {m: sys.modules.pop(m) for m in list(sys.modules) if m == "gsconverter" or m.startswith("gsconverter.")}
    mine = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    monkeypatch.setattr(mine, "_REFERENCE_CLASS", None)
    monkeypatch.syspath_prepend(str(tmp_path))
    _model_device(monkeypatch, lib)
    monkeypatch.setattr(writer, "plyfile_available", lambda: False)
    refused = _refusals()[0][1]
    try:
        import gsconverter.formats.ply_3dgs as r3
        import gsconverter.formats.ply_cc as rcc
        own3, owncc = r3.Ply3DGSFormat.write, rcc.PlyCCFormat.write
        try:
            gsx.install(ply_writer=False)
            assert r3.Ply3DGSFormat.write is own3 and rcc.PlyCCFormat.write is owncc
            gsx.uninstall()
            gsx.install()
            assert r3.Ply3DGSFormat.write is not own3 and rcc.PlyCCFormat.write is not owncc
            assert r3.Ply3DGSFormat.write.__wrapped__ is own3 and rcc.PlyCCFormat.write.__wrapped__ is owncc
            for cls, d in ((r3.Ply3DGSFormat, "3dgs"), (rcc.PlyCCFormat, "cc")):
                for name in ("crop_last_5", "extra_elements", "no_normals"):
                    c = cases[name]
                    path = str(tmp_path / ("bound_%s_%s.ply" % (name, d)))
                    assert cls().write(c.table, path, anything=1, **c.kwargs) is None
                    with open(path, "rb") as f:
                        assert f.read() == c.files[d], (name, d)
                with pytest.raises(writer.UnsupportedPlyError):                # no plyfile: nothing to hand a refused table to
                    cls().write(refused, str(tmp_path / "refused.ply"))
            monkeypatch.setattr(writer, "plyfile_available", lambda: True)     # with plyfile a refused table goes to the reference's write
            r3.Ply3DGSFormat().write(refused, str(tmp_path / "refused.ply"), crop_sh=False)
            assert (tmp_path / "refused.ply").read_text() == "own 3dgs crop_sh"
        finally:
            gsx.uninstall()
        assert r3.Ply3DGSFormat.write is own3 and rcc.PlyCCFormat.write is owncc
    finally:
        for m in [m for m in sys.modules if m == "gsconverter" or m.startswith("gsconverter.")]:
            del sys.modules[m]
        sys.modules.update(saved)


def test_compressed_ply_writer_shares_the_container(writer):
    cw = importlib.import_module("3dgsconverter_amd.formats.compressed_ply_writer")
    pc = importlib.import_module("3dgsconverter_amd.formats.ply_container")
    assert cw._write_ply is pc.write_ply and writer.header is pc.header
    formats = importlib.import_module("3dgsconverter_amd.formats")
    assert formats.write_ply_3dgs is writer.write_ply_3dgs and formats.write_ply_cc is writer.write_ply_cc


def test_golden_file_regenerates_identically_when_the_reference_is_there(tmp_path):
    from oracle import refload
    if not refload.available():
        pytest.skip("the reference is not mounted")
    env = dict(os.environ, PYTHONWARNINGS="ignore")
    code = ("import sys, runpy; sys.path.insert(0, %r); m = runpy.run_path(%r); m['main'].__globals__['OUT'] = %r; m['main']()"
            % (ROOT, os.path.join(ROOT, "tests", "devtools", "make_golden_ply_write.py"), str(tmp_path / "again.npz")))
    subprocess.run([sys.executable, "-c", code], check=True, env=env, capture_output=True, cwd=ROOT)
    a, b = np.load(GOLD), np.load(str(tmp_path / "again.npz"))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
