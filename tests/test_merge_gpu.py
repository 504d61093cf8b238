"""-m gpu: the merge on the device (csrc/rows_remap.hip) -- gsx_rows_remap_dev against the numpy definition of
tests/merge_numpy.py byte for byte for every source layout, both sides of the tile sizes, every alignment of the source and of
the destination's first byte, with guard bytes over everything that must stay; two sources back to back across an odd seam;
``ResidentRows.concat``; and ``Converter.run(merge=...)`` and the command line end to end on files this package wrote."""
import contextlib
import importlib
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limit_numpy as ln  # noqa: E402
import merge_cases as mc  # noqa: E402
import merge_numpy as mn  # noqa: E402
import ply_read_numpy as pn  # noqa: E402
import transform_cases as tc  # noqa: E402
import transform_numpy as tn  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = mc.GUARD
SIZES = (1, 63, 64, 65, 127, 128, 129, 1000)
SRC_FIRST = (0, 5, 15)
DST_ROW0 = (0, 1, 3, 130)


@pytest.fixture(scope="module")
def lib():
    lib = importlib.import_module("3dgsconverter_amd._lib")
    lib.require_hip()
    return lib


@pytest.fixture(scope="module")
def merge():
    return importlib.import_module("3dgsconverter_amd.merge")


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------------------ the kernel

@pytest.mark.parametrize("dst_stride", sorted(mc.DESTINATIONS))
@pytest.mark.parametrize("name", list(mc.LAYOUTS))
def test_remap_kernel_is_the_definition(lib, merge, ctx, name, dst_stride):
    src_dtype, dst_dtype = mc.LAYOUTS[name], mc.DESTINATIONS[dst_stride]
    si, so = src_dtype.itemsize, dst_stride
    runs = merge.remap_runs(src_dtype, dst_dtype)
    table = mc.table(src_dtype, max(SIZES))
    want_rows = mn.merge_tables([table], dst_dtype).view(np.uint8)          # the definition, once: row j depends on source row j alone
    rows_max = max(SIZES) + max(DST_ROW0) + 2
    d_src, d_dst = ctx.alloc(16 + max(SIZES) * si + 16), ctx.alloc(rows_max * so + 16)
    bad, done = [], 0
    try:
        for first in SRC_FIRST:
            src = np.zeros(first + max(SIZES) * si + 16, np.uint8)
            src[first:first + table.nbytes] = table.view(np.uint8)
            d_src.upload(src)
            for n in SIZES:
                for row0 in DST_ROW0:
                    rows = n + row0 + 2
                    guard = np.full(rows * so + 16, GUARD, np.uint8)
                    d_dst.upload(guard)
                    lib.rows_remap_dev(ctx, d_src.ptr, first, si, n, runs, d_dst.ptr, 0, so, row0, rows)
                    ctx.synchronize()
                    got = d_dst.download(np.uint8, rows * so + 16)
                    guard[row0 * so:(row0 + n) * so] = want_rows[:n * so]
                    done += 1
                    if got.tobytes() != guard.tobytes():
                        at = int(np.nonzero(got != guard)[0][0])
                        bad.append((first, n, row0, "byte %d (row %d, byte %d of it): %#x for %#x" % (at, at // so, at % so, got[at], guard[at])))
    finally:
        d_src.free()
        d_dst.free()
    assert done == len(SRC_FIRST) * len(SIZES) * len(DST_ROW0)
    assert not bad, (len(bad), bad[:5])


def test_remap_kernel_destination_first_byte(lib, merge, ctx):
    """the destination's row 0 at byte 0 ... 15 of its base, as a ResidentRows may have it"""
    src_dtype, dst_dtype = mc.LAYOUTS["spz1"], mc.DESTINATIONS[251]
    table = mc.table(src_dtype, 129)
    want = mn.merge_tables([table], dst_dtype).view(np.uint8)
    runs = merge.remap_runs(src_dtype, dst_dtype)
    rr = lib.ResidentRows.from_host(table, first_byte=9)
    d_dst = ctx.alloc(16 + 140 * 251 + 16)
    try:
        for dst_first in (1, 8, 15):
            guard = np.full(16 + 140 * 251 + 16, GUARD, np.uint8)
            d_dst.upload(guard)
            lib.rows_remap_dev(ctx, rr.ptr, rr.first_byte, 107, 129, runs, d_dst.ptr, dst_first, 251, 7, 140)
            ctx.synchronize()
            guard[dst_first + 7 * 251:dst_first + 136 * 251] = want
            assert d_dst.download(np.uint8, len(guard)).tobytes() == guard.tobytes(), dst_first
    finally:
        rr.close()
        d_dst.free()


def test_two_sources_meet_at_an_odd_byte(lib, merge, ctx):
    """source A's rows end exactly where source B's begin, at an odd byte inside a 16-byte quad: both ranges exact, in either order
    of the launches, so the seam is never written by the wrong one"""
    dst_dtype = mc.DESTINATIONS[251]
    a, b = mc.table(mc.LAYOUTS["spz1"], 74), mc.table(mc.LAYOUTS["cc"], 131, seed=1)
    seam = (1 + len(a)) * 251
    assert seam % 2 == 1 and seam % 16 == 9
    want = np.full(210 * 251 + 16, GUARD, np.uint8)
    want[251:(1 + len(a) + len(b)) * 251] = mn.merge_tables([a, b], dst_dtype).view(np.uint8)
    ra, rb = lib.ResidentRows.from_host(a), lib.ResidentRows.from_host(b, first_byte=3)
    d_dst = ctx.alloc(len(want))
    try:
        for order in ((0, 1), (1, 0)):
            d_dst.upload(np.full(len(want), GUARD, np.uint8))
            for k in order:
                rr, row0 = ((ra, 1), (rb, 1 + len(a)))[k]
                lib.rows_remap_dev(ctx, rr.ptr, rr.first_byte, rr.dtype.itemsize, rr.n, merge.remap_runs(rr.dtype, dst_dtype), d_dst.ptr, 0, 251, row0, 210)
            ctx.synchronize()
            assert d_dst.download(np.uint8, len(want)).tobytes() == want.tobytes(), order
    finally:
        ra.close()
        rb.close()
        d_dst.free()


def test_whole_row_run_is_a_copy_and_refusals_write_nothing(lib, merge, ctx):
    dt = mc.DESTINATIONS[251]
    table = mc.table(dt, 100)
    assert merge.remap_runs(dt, dt) == [(0, 0, 251)]
    rr = lib.ResidentRows.from_host(table, first_byte=5)
    d_dst = ctx.alloc(120 * 251 + 16)
    L = lib.load()
    try:
        guard = np.full(120 * 251 + 16, GUARD, np.uint8)
        d_dst.upload(guard)
        runs, n_runs = lib.remap_runs_array(merge.remap_runs(mc.spz_dtype(1), dt))
        for what, args in mc.bad_remap_arguments(rr.ptr, d_dst.ptr, runs):
            assert L.gsx_rows_remap_dev(ctx.handle, *args) != 0, what
            assert lib.last_error().startswith("gsx_rows_remap_dev: "), (what, lib.last_error())
        assert L.gsx_rows_remap_dev(None, rr.ptr, 5, 251, 100, runs, n_runs, d_dst.ptr, 0, 251, 0, 120) != 0
        assert L.gsx_rows_remap_dev(ctx.handle, rr.ptr, 5, 107, 0, runs, n_runs, d_dst.ptr, 0, 251, 120, 120) == 0     # n = 0 launches nothing
        ctx.synchronize()
        assert d_dst.download(np.uint8, len(guard)).tobytes() == guard.tobytes(), "a refused call wrote the destination"
        lib.rows_remap_dev(ctx, rr.ptr, rr.first_byte, 251, 100, [(0, 0, 251)], d_dst.ptr, 0, 251, 11, 120)
        ctx.synchronize()
        guard[11 * 251:111 * 251] = table.view(np.uint8)
        assert d_dst.download(np.uint8, len(guard)).tobytes() == guard.tobytes()
    finally:
        rr.close()
        d_dst.free()


def test_concat(lib, merge):
    a, b, c = mc.table(mc.LAYOUTS["std"], 300), mc.table(mc.LAYOUTS["cc"], 41), mc.table(mc.LAYOUTS["spz1"], 0)
    union, _ = merge.merged_dtype([t.dtype for t in (a, b, c)])
    runs = [merge.remap_runs(t.dtype, union) for t in (a, b, c)]
    before = lib.ResidentRows.open_count
    parts = [lib.ResidentRows.from_host(t, first_byte=f) for t, f in ((a, 0), (b, 4), (c, 11))]
    try:
        ms = {}
        out = lib.ResidentRows.concat(parts, union, runs, stage_ms=ms)
        try:
            assert out.n == 341 and out.dtype == union and list(ms) == ["remap"] and ms["remap"] > 0
            assert out.download().tobytes() == mn.merge_tables([a, b, c]).tobytes()
            assert out.profile()["n"] == 341
            assert all(not p.closed for p in parts) and lib.ResidentRows.open_count == before + 4
        finally:
            out.close()
        with pytest.raises(lib.GsxError, match="gsx_rows_remap_dev: output byte 247 belongs to no run"):
            s, d, nb = runs[1][-1]      # the second part's last run a byte short: refused after the first part's launch
            lib.ResidentRows.concat(parts, union, [runs[0], runs[1][:-1] + [(s, d, nb - 1)], runs[2]])
        assert lib.ResidentRows.open_count == before + 3 and all(not p.closed for p in parts)
        with pytest.raises(ValueError, match="3 parts, runs for 2"):
            lib.ResidentRows.concat(parts, union, runs[:2])
        empty = lib.ResidentRows.concat([], union, [])
        assert empty.n == 0 and len(empty.download()) == 0
        empty.close()
    finally:
        for p in parts:
            p.close()
    assert lib.ResidentRows.open_count == before


# ------------------------------------------------------------------------------------------------------------ the converter

def _run(conv, src, dst, target, resident, **kw):
    c = conv.Converter(src, dst, target, resident=resident)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
        c.run(**kw)
    with open(dst, "rb") as f:
        return f.read(), buf.getvalue().split("\n"), c


@pytest.fixture(scope="module")
def scenes(lib, tmp_path_factory):
    """a 3000-row degree-3 PLY, a 1200-row .spz at degree 1 and an 800-row .splat, the last two written by this package's writers
    -> (directory, {name: path}, {name: the table the package's reader returns for the file}): the definition's inputs"""
    conv = importlib.import_module("3dgsconverter_amd.converter")
    root = tmp_path_factory.mktemp("merge_converter")
    fields = [f for f in pn.canonical_fields(3) if f[0] not in ("nx", "ny", "nz")]
    paths = {"ply": str(root / "a.ply"), "spz": str(root / "b.spz"), "splat": str(root / "c.splat")}
    for name, n, seed in (("ply", 3000, 77), ("spz", 1200, 78), ("splat", 800, 79)):
        pn.write_ply(str(root / (name + "_source.ply")), [("vertex", pn.build(n, fields, np.random.default_rng(seed)))])
    os.replace(str(root / "ply_source.ply"), paths["ply"])
    _run(conv, str(root / "spz_source.ply"), paths["spz"], "spz", True, sh_level=1)
    _run(conv, str(root / "splat_source.ply"), paths["splat"], "splat", True)
    read = {"ply": lambda p: importlib.import_module("3dgsconverter_amd.formats.ply_reader").read_ply_3dgs(p)[0],
            "spz": importlib.import_module("3dgsconverter_amd.formats.spz_reader").read_spz,
            "splat": importlib.import_module("3dgsconverter_amd.formats.splat_reader").read_splat}
    tables = {name: read[name](paths[name]) for name in paths}
    assert [len(tables[k]) for k in ("ply", "spz", "splat")] == [3000, 1200, 800]
    assert [tables[k].dtype.itemsize for k in ("ply", "spz", "splat")] == [248, 107, 71]
    return root, paths, tables


def test_converter_merges_three_formats(lib, scenes):
    conv = importlib.import_module("3dgsconverter_amd.converter")
    read = importlib.import_module("3dgsconverter_amd.formats.ply_reader").read_ply_3dgs
    root, paths, tables = scenes
    want = mn.merge_tables([tables["ply"], tables["spz"], tables["splat"]])
    assert want.dtype == mc.standard_dtype()
    before = lib.ResidentRows.open_count
    blobs = {}
    for resident in (True, False):
        dst = str(root / ("union_%d.ply" % resident))
        blobs[resident], lines, c = _run(conv, paths["ply"], dst, "3dgs", resident, merge=[paths["spz"], paths["splat"]])
        back, _ = read(dst)
        assert back.dtype == want.dtype and back.tobytes() == want.tobytes(), resident
        assert c.data.tobytes() == want.tobytes() and c.profile["n"] == 5000
        said = [f"Merge: {paths['spz']} (SPZ, 1,200 splats)", f"Merge: {paths['splat']} (SPLAT, 800 splats)",
                "Merged 3 sources: 5,000 splats, 45 SH columns.",
                f"Merge: {paths['spz']!r} loses 3 fields the union does not have: red, green, blue",
                f"Merge: {paths['splat']!r} loses 3 fields the union does not have: red, green, blue"]
        at = [lines.index(s) for s in said]
        assert at == sorted(at), lines
        clocks = c.stage_ms
        assert clocks["merge_read"] > 0 and clocks["merge_remap"] > 0 and ("merge_download" in clocks) == resident, clocks
        assert "merge_transform" not in clocks
    assert blobs[True] == blobs[False]
    assert lib.ResidentRows.open_count == before


@pytest.mark.parametrize("resident", (True, False))
def test_converter_keeps_colours_every_source_has(lib, scenes, resident):
    conv = importlib.import_module("3dgsconverter_amd.converter")
    root, paths, tables = scenes
    want = mn.merge_tables([tables["spz"], tables["splat"]])
    assert want.dtype == mc.spz_dtype(1)
    _, lines, c = _run(conv, paths["spz"], str(root / ("coloured_%d.ply" % resident)), "3dgs", resident, merge=[paths["splat"]])
    assert c.data.dtype == want.dtype and c.data.tobytes() == want.tobytes()
    assert "Merged 2 sources: 2,000 splats, 9 SH columns." in lines and not [s for s in lines if " loses " in s]


@pytest.mark.parametrize("resident", (True, False))
def test_every_source_is_decoded_once_and_no_merge_changes_nothing(lib, scenes, resident, monkeypatch):
    conv = importlib.import_module("3dgsconverter_amd.converter")
    ply = importlib.import_module("3dgsconverter_amd.formats.ply_reader")
    writer = importlib.import_module("3dgsconverter_amd.formats.ply_writer")
    root, paths, tables = scenes
    reads = []
    real = conv.SourceHandler.read

    def counted(self, path, stage_ms=None):
        reads.append(path)
        return real(self, path, stage_ms=stage_ms)
    monkeypatch.setattr(conv.SourceHandler, "read", counted)
    _run(conv, paths["ply"], str(root / ("once_%d.ply" % resident)), "3dgs", resident, merge=[paths["spz"], paths["splat"]])
    assert reads == [paths["ply"], paths["spz"], paths["splat"]]
    del reads[:]
    blob, lines, c = _run(conv, paths["ply"], str(root / ("plain_%d.ply" % resident)), "3dgs", resident)
    assert reads == [paths["ply"]]
    assert not [k for k in c.stage_ms if k.startswith("merge")] and not [s for s in lines if s.startswith("Merge")]
    direct = str(root / "direct.ply")
    with contextlib.redirect_stdout(io.StringIO()):
        writer.write_ply_3dgs(ply.read_ply_3dgs(paths["ply"])[0], direct)
    with open(direct, "rb") as f:
        assert blob == f.read()


@pytest.mark.parametrize("resident", (True, False))
def test_a_merge_source_takes_its_own_transform(lib, scenes, resident):
    conv = importlib.import_module("3dgsconverter_amd.converter")
    tf = importlib.import_module("3dgsconverter_amd.transform")
    root, paths, tables = scenes
    moved = tn.transform_table(tables["spz"], tf.rotation_from_euler_deg(0, 90, 0), 2.0, (1, 2, 3))
    want = mn.merge_tables([tables["ply"], moved])
    _, lines, c = _run(conv, paths["ply"], str(root / ("moved_%d.ply" % resident)), "3dgs", resident, merge=[paths["spz"]],
                       merge_transforms=[{"rotate": (0, 90, 0), "scale": 2.0, "translate": (1, 2, 3)}])
    assert "Merge Transform [1]: scale 2, rotate [0, 90, 0] deg, translate [1, 2, 3]" in lines
    assert not [s for s in lines if s.startswith("Transform:")]
    got = c.data
    assert tn.same_by_class(got, want, tc.float_fields(want.dtype)) is None, tn.same_by_class(got, want, tc.float_fields(want.dtype))
    assert got[:3000].tobytes() == want[:3000].tobytes(), "the main source was moved"
    assert got[3000:].tobytes() != mn.merge_tables([tables["spz"]], want.dtype).tobytes()
    assert c.stage_ms["merge_transform"] > 0


BOX = (-3.0, -3.5, -3.0, 4.0, 3.0, 3.0)      # (the fixtures' coordinates are normal with sigma 3: about a third of the rows)


@pytest.mark.parametrize("resident", (True, False))
def test_the_filters_see_the_union(lib, scenes, resident):
    conv = importlib.import_module("3dgsconverter_amd.converter")
    root, paths, tables = scenes
    union = mn.merge_tables([tables["ply"], tables["spz"], tables["splat"]])
    x, y, z = union["x"], union["y"], union["z"]
    cropped = union[(x >= BOX[0]) & (x <= BOX[3]) & (y >= BOX[1]) & (y <= BOX[4]) & (z >= BOX[2]) & (z <= BOX[5])]
    assert 1000 < len(cropped) < 4000 and (cropped["f_rest_44"] == 0).any() and (cropped["f_rest_44"] != 0).any()     # rows of several sources
    N = len(cropped) // 3
    _, lines, c = _run(conv, paths["ply"], str(root / ("filtered_%d.ply" % resident)), "3dgs", resident, merge=[paths["spz"], paths["splat"]],
                       bbox=list(BOX), max_splats=N)
    assert c.data.tobytes() == ln.limit_table(cropped, N).tobytes()
    assert f"Splat Limit (max {N}): Retained {N} out of {len(cropped)} splats." in lines


def test_command_line_merges(scenes, capsys):
    """python -m 3dgsconverter_amd -i a.ply --merge b.spz --merge c.splat --merge_translate 1 0 0 --merge_translate 0 1 0 -f 3dgs --force
    (in this process)"""
    cli = importlib.import_module("3dgsconverter_amd.cli")
    read = importlib.import_module("3dgsconverter_amd.formats.ply_reader").read_ply_3dgs
    root, paths, tables = scenes
    dst = str(root / "cli_union.ply")
    with np.errstate(all="ignore"):
        cli.main(["-i", paths["ply"], "--merge", paths["spz"], "--merge", paths["splat"], "--merge_translate", "1", "0", "0",
                  "--merge_translate", "0", "1", "0", "-f", "3dgs", "-o", dst, "--force"])
    out = capsys.readouterr().out
    lines = out.split("\n")
    assert "Merge Transform [1]: scale 1, rotate [0, 0, 0] deg, translate [1, 0, 0]" in lines
    assert "Merge Transform [2]: scale 1, rotate [0, 0, 0] deg, translate [0, 1, 0]" in lines
    assert "Merged 3 sources: 5,000 splats, 45 SH columns." in lines
    assert out.count("Points: 3,000") == 1 and out.split(">>> TARGET FILE INFO")[1].count("Points: 5,000") == 1
    back, _ = read(dst)
    want = mn.merge_tables([tables["ply"], tn.transform_table(tables["spz"], None, None, (1, 0, 0)),
                            tn.transform_table(tables["splat"], None, None, (0, 1, 0))])
    assert back.tobytes() == want.tobytes()
