"""-m gpu: the 3DGS / CloudCompare PLY writers on the device -- every golden case through both writers against the file the
reference's own writer made, byte for byte; a `pack` stage for every table whose rows are not the file's already and none for
the others (no silent way round the kernel); the crop scan's answer; the written file read back by this package's readers; the
strides at both ends of the kernel's range and both tile shapes against the numpy restatement (tests/ply_write_numpy.py, which
the host tests tie to the reference); and install()'s bound `write`."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ply_read_numpy as pn  # noqa: E402
import ply_write_numpy as pw  # noqa: E402
import rest_scan_cases as rsc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ply_write_ref.npz")
BOTH = ("3dgs", "cc")
pytestmark = pytest.mark.gpu
# the table's rows are the file's rows already: written as they are; with crop_sh on f_rest fields, after the device's scan
IDENTITY = {"canonical_deg3", "canonical_rgb", "deg0_crop", "deg1_crop", "deg2_crop", "crop_last_44", "extra_elements_zero_rows"}
EMPTY = {"zero_rows", "zero_rows_crop", "extra_elements_zero_rows"}
SCANNED_IDENTITY = {"deg1_crop", "deg2_crop", "crop_last_44"}
HOST_SCAN = {"f8_rest_3_crop"}                                   # an f_rest field that is not <f4: numpy scans, the device packs


@pytest.fixture(scope="module")
def cases():
    return pw.load_cases(GOLD)


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgsconverter_amd._lib")


@pytest.fixture(scope="module")
def writer(lib):
    mod = importlib.import_module("3dgsconverter_amd.formats.ply_writer")
    lib.require_hip()
    return mod


@pytest.fixture(scope="module")
def written(cases, writer, tmp_path_factory):
    """every case through both writers, once: {(case, dialect): (path, plan, stage_ms)}"""
    tmp = tmp_path_factory.mktemp("ply_write")
    out = {}
    for c in cases.values():
        for d in BOTH:
            st = {}
            path = str(tmp / ("%s_%s.ply" % (c.name, d)))
            plan = _write(writer, d)(c.table, path, stage_ms=st, **c.kwargs)
            out[(c.name, d)] = (path, plan, st)
    return out


def _write(writer, dialect):
    return writer.write_ply_3dgs if dialect == "3dgs" else writer.write_ply_cc


def _first_difference(got, want):
    if len(got) != len(want):
        return "%d bytes, %d expected" % (len(got), len(want))
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    bad = np.nonzero(a != b)[0]
    return "%d bytes differ, first at byte %d: %s != %s" % (len(bad), bad[0], got[bad[0]:bad[0] + 8].hex(), want[bad[0]:bad[0] + 8].hex())


def test_every_golden_file_is_reproduced_byte_for_byte(cases, written):
    assert len(written) == 2 * len(cases) == 66
    for (name, d), (path, plan, st) in written.items():
        with open(path, "rb") as f:
            got = f.read()
        want = cases[name].files[d]
        assert got == want, "%s %s: %s" % (name, d, _first_difference(got, want))
        assert plan.refusal is None and [list(p) for p in plan.properties] == cases[name].writers[d]["properties"], (name, d)


def test_pack_stage_for_every_table_that_is_not_the_files_rows_already(cases, written):
    for (name, d), (path, plan, st) in written.items():
        packed = name not in IDENTITY and name not in EMPTY
        assert ("pack" in st) == packed == ("download" in st), (name, d, st)
        assert ("upload" in st) == (packed or name in SCANNED_IDENTITY), (name, d, st)
        assert plan.identity == (name in IDENTITY) and {"plan", "file_write"} <= set(st), (name, d, st)


def test_crop_scan_finds_the_references_last_idx(cases, written):
    seen = set()
    for (name, d), (path, plan, st) in written.items():
        c = cases[name]
        assert plan.last_idx == c.writers[d].get("last_idx"), (name, d)
        if c.crop_sh:
            seen.add(plan.last_idx)
            on_device = len(c.table) > 0 and name not in HOST_SCAN and any(f.startswith("f_rest_") for f in c.table.dtype.names)
            assert "sh_detect" in st and ("upload" in st) >= on_device, (name, d, st)
    assert seen >= {-1, 0, 5, 8, 9, 23, 24, 44}


@pytest.mark.parametrize("row_bytes,n", rsc.CASES)
def test_rest_scan_is_numpys_any_nonzero_at_the_edge_values(lib, writer, row_bytes, n):
    """gsx_ply_rest_nonzero_dev on rows of 248 bytes (tiles of 128) and of 261 (tiles of 64, every field at an odd offset), one
    row, one full tile and one row more: -0.0 in the last row sets no bit; the smallest denormal of either sign, a NaN and 1.0
    set exactly their field's bit; the fields that are not asked for hold 1.0 and never show"""
    import ctypes as C
    t = rsc.table(row_bytes, n)
    offsets = (C.c_int32 * 45)(*[t.dtype.fields[f][1] for f in rsc.REST])
    ctx = lib.Context(0)
    d_rows = ctx.alloc(t.nbytes + 64)
    try:
        for i, want, word in rsc.plantings(t):
            d_rows.upload(t)
            got = C.c_uint64(0)
            lib.check(ctx.lib.gsx_ply_rest_nonzero_dev(ctx.handle, d_rows.ptr, row_bytes, n, offsets, want, C.byref(got)), "gsx_ply_rest_nonzero_dev")
            assert got.value == word, "f_rest_%d: got %#x, numpy %#x" % (i, got.value, word)
    finally:
        d_rows.free()
        ctx.close()


def test_written_files_read_back_the_tables_standard_fields(cases, written, lib):
    reader = importlib.import_module("3dgsconverter_amd.formats.ply_reader")
    std = set(pn.get_standard_order(True))
    checked = 0
    for (name, d), (path, plan, st) in written.items():
        c = cases[name]
        rows, extras = (reader.read_ply_3dgs if d == "3dgs" else reader.read_ply_cc)(path)
        assert len(rows) == len(c.table) and [e.name for e in extras] == [e.name for e in c.extras], (name, d)
        for e, x in zip(extras, c.extras):
            assert [e.data[f].tolist() for f in e.data.dtype.names] == [x.data[f].tolist() for f in x.data.dtype.names], (name, d, e.name)
        kept = {f.source for f in plan.fields if f.source is not None}
        for f in c.table.dtype.names:
            if f in std and f in kept and f in rows.dtype.names and rows.dtype[f] == c.table.dtype[f]:
                assert np.ascontiguousarray(rows[f]).tobytes() == np.ascontiguousarray(c.table[f]).tobytes(), (name, d, f)
                checked += 1
    assert checked >= 66 * 13                                      # x y z, f_dc_0..2, scale_0..2, rot_0..3 are in every table


def test_strides_at_both_ends_and_both_tile_shapes_equal_the_restatement(writer, tmp_path):
    """rows of 1 byte in and 13 out, of 512 bytes in and out (tiles of 64 rows), fields at every byte phase; more rows than one tile"""
    rng = np.random.default_rng(11)
    layouts = [[("e", "u1")],
               [("a", "u1"), ("x", "f4"), ("b", "u2"), ("y", "f4"), ("c", "u1"), ("z", "f8"), ("opacity", "f4"), ("d", "u1")],
               [("k%d" % i, "u1") for i in range(3)] + pn.canonical_fields(3) + [("t%d" % i, "f8") for i in range(30)] + [("w", "u1")],
               [("t0", "f8")] + pn.canonical_fields(3) + [("t%d" % i, "f8") for i in range(1, 33)]]
    for k, fields in enumerate(layouts):
        for n in (65, 257):
            t = pn.build(n, fields, rng)
            for d in BOTH:
                for crop in (False, True):
                    st = {}
                    path = str(tmp_path / "s.ply")
                    plan = _write(writer, d)(t, path, stage_ms=st, crop_sh=crop)
                    _, _, want, last = pw.write(t, d, crop)
                    with open(path, "rb") as f:
                        got = f.read()
                    assert got == want, "layout %d, %d rows, %s, crop %s: %s" % (k, n, d, crop, _first_difference(got, want))
                    assert "pack" in st and plan.last_idx == last
    assert pn.build(1, layouts[3], rng).dtype.itemsize == 512


def test_refused_tables_are_refusals_on_the_device_too(writer, tmp_path, monkeypatch):
    monkeypatch.setattr(writer, "plyfile_available", lambda: False)
    base = [(f, "<f4") for f, _ in pn.canonical_fields(1)]
    for table, words in ((np.zeros(5, base + [("h", "<f2")]), "field 'h' is float16"),
                         (np.zeros(5, base + [("t%d" % i, "<f8") for i in range(52)]), "rows of 520 bytes")):
        for crop in (False, True):                                # crop_sh on: refused after the upload and the scan
            with pytest.raises(writer.UnsupportedPlyError, match=words):
                writer.write_ply_3dgs(table, str(tmp_path / "r.ply"), crop_sh=crop)


def test_bound_write_after_install_produces_the_same_file(gsx, cases, tmp_path):
    try:
        from oracle import refload
        ok = refload.available()
    except ImportError:
        ok = False
    if not ok:
        pytest.skip("the reference is not mounted: its modules cannot be imported")
    refload.load()
    import gsconverter.formats.ply_3dgs as r3  # type: ignore
    import gsconverter.formats.ply_cc as rcc  # type: ignore
    gsx.install()
    try:
        for cls, d in ((r3.Ply3DGSFormat, "3dgs"), (rcc.PlyCCFormat, "cc")):
            for name in ("rgb_no_normals", "crop_last_5", "extra_elements", "holes"):
                c = cases[name]
                path = str(tmp_path / ("%s_%s.ply" % (name, d)))
                cls().write(c.table, path, **c.kwargs)
                with open(path, "rb") as f:
                    assert f.read() == c.files[d], (name, d)
    finally:
        gsx.uninstall()
