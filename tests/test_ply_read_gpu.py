"""-m gpu: the 3DGS / CloudCompare PLY readers on the device -- every golden case against the reference's own rows (dtype, field
order, every row's bytes) through the reader or readers the spec names, every source type in both byte orders at its edge values,
every tile boundary on both tile shapes with the body at every kind of file offset, the stride and field caps, random layouts,
the host-only identity path and concurrent readers.  Every check is on row bytes; the expected rows are the numpy restatement's
(tests/ply_read_numpy.py), which the host tests tie to the reference."""
import importlib
import json
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ply_read_numpy as pn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ply_read_ref.npz")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return g, json.loads(bytes(g["spec"]).decode())


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgsconverter_amd._lib")


@pytest.fixture(scope="module")
def reader(lib):
    mod = importlib.import_module("3dgsconverter_amd.formats.ply_reader")
    lib.require_hip()
    return mod


def _read(reader, dialect):
    return reader.read_ply_3dgs if dialect == "3dgs" else reader.read_ply_cc


def _assert_bytes(name, rows, want):
    """dtype, field order and every byte; names the first differing row and field"""
    assert rows.dtype == want.dtype and rows.dtype.names == want.dtype.names, name
    got = np.ascontiguousarray(rows).view(np.uint8).reshape(-1)
    exp = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert got.shape == exp.shape, "%s: %d bytes, %d expected" % (name, got.size, exp.size)
    bad = np.nonzero(got != exp)[0]
    if len(bad):
        rb = rows.dtype.itemsize
        row, col = bad[0] // rb, bad[0] % rb
        field = [f for f in rows.dtype.names if rows.dtype.fields[f][1] <= col][-1]
        o = rows.dtype.fields[field][1]
        raise AssertionError("%s: %d bytes differ, first at row %d field %s: %s != %s" % (
            name, len(bad), row, field, got[row * rb + o:][:8].tobytes().hex(), exp[row * rb + o:][:8].tobytes().hex()))


def _against_restatement(reader, path, dialect, name, stage_ms=None):
    rows, _ = _read(reader, dialect)(path, stage_ms=stage_ms)
    _assert_bytes(name, rows, pn.read(path, dialect)[0])
    return rows


def test_every_golden_case_is_the_references_rows(gold, reader, tmp_path):
    g, spec = gold
    checked = 0
    for name, rec in spec.items():
        p = tmp_path / (name + ".ply")
        p.write_bytes(g[name + "__file"].tobytes())
        for dialect, r in rec["readers"].items():
            if "error" in r:
                with pytest.raises(ValueError) as e:
                    _read(reader, dialect)(str(p))
                assert str(e.value) == r["error"]["message"]
                continue
            rows, extras = _read(reader, dialect)(str(p))
            assert list(rows.dtype.names) == r["names"] and [rows.dtype[f].str for f in rows.dtype.names] == r["dtype"], (name, dialect)
            assert rows.dtype.itemsize == r["itemsize"] and len(rows) == r["rows"], (name, dialect)
            want = np.frombuffer(g["%s__%s__rows" % (name, dialect)].tobytes(), rows.dtype)
            _assert_bytes("%s/%s" % (name, dialect), rows, want)
            assert [e.name for e in extras] == r["extra_elements"]
            checked += 1
    assert checked == 33


def test_every_source_type_in_both_byte_orders_converts_as_numpy_does(reader, lib, tmp_path):
    """16 files: one source type on all the standard float fields, 256 rows of edge values (pn.edge_values), each field a
    rotation of them; little- and big-endian.  The float32 little-endian file is the identity layout, which the readers never
    send to the device: it goes through the kernel by its plan as well."""
    for typ in pn.SOURCE_TYPES:
        table = pn.type_matrix_table(typ)
        for fmt in ("binary_little_endian", "binary_big_endian"):
            path = pn.write_ply(str(tmp_path / ("m_%s_%s.ply" % (typ, fmt[7]))), [("vertex", table)], fmt)
            st = {}
            _against_restatement(reader, path, "3dgs", "%s %s" % (typ, fmt), st)
            assert ("kernel" in st) == (not (typ == "f4" and fmt == "binary_little_endian"))
            _against_restatement(reader, path, "cc", "%s %s cc" % (typ, fmt))
    path = str(tmp_path / "m_f4_l.ply")
    p = reader.plan(reader.parse_header(path), "3dgs")
    assert p.identity
    rows = lib.ply_unpack_table(path, p.body_offset, p.count, p.layout(), p.dtype)
    _assert_bytes("f4 through the kernel", rows, pn.read(path, "3dgs")[0])


def test_every_tile_boundary_on_both_tile_shapes_at_every_body_offset(reader, tmp_path):
    """68-byte rows (degree 0, float32: tiles of 128 rows) and 496-byte rows (degree 3, float64: tiles of 64 rows); the header's
    comment padding puts the body at file offsets 0, 1, 7 and 15 mod 16"""
    rng = np.random.default_rng(11)
    for fields, stride in ((pn.canonical_fields(0), 68), (pn.canonical_fields(3, "f8"), 496)):
        full = pn.build(257, fields, rng)
        assert full.dtype.itemsize == stride
        for n in (1, 63, 64, 65, 127, 128, 129, 257):
            want = pn.convert(full[:n], "3dgs")
            for mod in (0, 1, 7, 15):
                path = pn.write_ply(str(tmp_path / "t.ply"), [("vertex", full[:n])], body_mod16=mod)
                h = reader.parse_header(path)
                assert h.element("vertex").body_offset % 16 == mod
                st = {}
                rows, _ = reader.read_ply_3dgs(path, stage_ms=st)
                assert "kernel" in st
                _assert_bytes("stride %d n %d offset %d" % (stride, n, mod), rows, want)


def test_strides_and_field_counts_at_the_caps_are_read_and_past_them_refused(reader, tmp_path):
    rng = np.random.default_rng(12)
    f8 = [(f, "f8") for f in pn.FLOAT_FIELDS]
    wide_out = pn.canonical_fields(0) + [("e%d" % i, "f8") for i in range(33)]
    many = pn.canonical_fields(3) + [("e%d" % i, "u1") for i in range(66)]
    for name, fields, what in (("in512", f8 + [("e0", "f8"), ("e1", "f8")], (512, None, None)),
                               ("out512", wide_out, (None, 512, None)),
                               ("fields128", many, (None, None, 128)),
                               # both tiles at their widest: 128 rows of 256 bytes, 64 rows of 512 bytes, in and out (the most LDS)
                               ("both256", pn.canonical_fields(3) + [("e0", "f4"), ("e1", "i4")], (256, 256, None)),
                               ("both512", pn.canonical_fields(3) + [("e%d" % i, "f8") for i in range(33)], (512, 512, None))):
        path = pn.write_ply(str(tmp_path / (name + ".ply")), [("vertex", pn.build(131, fields, rng))], body_mod16=5)
        p = reader.plan(reader.parse_header(path), "3dgs")
        assert p.refusal is None and [a == b for a, b in zip((p.in_stride, p.out_stride, len(p.fields)), what) if b is not None] in ([True], [True, True])
        for dialect in ("3dgs", "cc"):
            _against_restatement(reader, path, dialect, name)
    for name, fields in (("in513", f8 + [("e0", "f8"), ("e1", "f8"), ("b", "u1")]), ("out513", wide_out + [("b", "u1")]), ("fields129", many + [("e66", "u1")])):
        path = pn.write_ply(str(tmp_path / (name + ".ply")), [("vertex", pn.build(5, fields, rng))])
        with pytest.raises(reader.UnsupportedPlyError):
            reader.read_ply_3dgs(path)
        assert reader.read_ply_cc(path, fallback=lambda p: "fallback") == "fallback"


def test_random_layouts_equal_the_restatement(reader, tmp_path):
    for seed in range(20):
        table, dialect = pn.random_layout(seed, 1000)
        path = pn.write_ply(str(tmp_path / "r.ply"), [("vertex", table)], body_mod16=(5 * seed) % 16)
        _against_restatement(reader, path, dialect, "seed %d (%s)" % (seed, dialect))


def test_identity_layout_is_read_on_the_host_alone(reader, tmp_path):
    rng = np.random.default_rng(13)
    path = pn.write_ply(str(tmp_path / "canonical.ply"), [("vertex", pn.build(1000, pn.canonical_fields(3), rng))])
    for dialect in ("3dgs", "cc"):
        st = {}
        _against_restatement(reader, path, dialect, "canonical " + dialect, st)
        assert "file_read" in st and not {"upload", "kernel", "download"} & set(st)


def test_four_threads_read_four_files_at_once(reader, tmp_path):
    rng = np.random.default_rng(14)
    jobs = []
    for k, (fields, dialect, fmt) in enumerate(((pn.canonical_fields(0), "3dgs", "binary_little_endian"), (pn.cc_fields(3), "cc", "binary_little_endian"),
                                                (pn.canonical_fields(3, "f8"), "3dgs", "binary_big_endian"), (pn.cc_fields(1), "3dgs", "binary_little_endian"))):
        path = pn.write_ply(str(tmp_path / ("c%d.ply" % k)), [("vertex", pn.build(3000 + 97 * k, fields, rng))], fmt, body_mod16=3 * k)
        single, _ = _read(reader, dialect)(path)
        _assert_bytes("single %d" % k, single, pn.read(path, dialect)[0])
        jobs.append((path, dialect, single))
    results, errors = [None] * 4, []
    start = threading.Barrier(4)

    def run(i):
        try:
            start.wait(timeout=30)
            out = []
            for _ in range(3):
                out.append(_read(reader, jobs[i][1])(jobs[i][0])[0])
            results[i] = out
        except BaseException as e:  # noqa: BLE001 -- reported below, on the main thread
            errors.append((i, e))
    threads = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, (path, dialect, single) in enumerate(jobs):
        for rows in results[i]:
            _assert_bytes("thread %d" % i, rows, single)
