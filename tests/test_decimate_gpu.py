"""-m gpu: voxel decimation on the device (csrc/decimate.hip) against the numpy definition of tests/decimate_numpy.py under the
comparison rule of transform_numpy.same_by_class -- the two entry points on every row layout, first byte, size and group shape
with guard bytes around the output, the rows the merge cannot use, a survivor list with zeroed fields, the refusal of a cell
beyond +-2^20; ``decimate`` of a lazy processor over resident rows, over a host table and of an eager processor, composed with
the other filters; and ``Converter.run(decimate_voxel_size=)`` end to end."""
import contextlib
import ctypes as C
import importlib
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decimate_cases as dc  # noqa: E402
import decimate_numpy as dn  # noqa: E402
import limit_numpy as ln  # noqa: E402
import ply_read_numpy as pn  # noqa: E402
import transform_numpy as tn  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 0xA5
dec = importlib.import_module("3dgsconverter_amd.decimate")


@pytest.fixture(scope="module")
def lib():
    lib = importlib.import_module("3dgsconverter_amd._lib")
    lib.require_hip()
    return lib


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dp(lib):
    return importlib.import_module("3dgsconverter_amd.processing.data_processor")


def _quiet(call):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        return call()


def device_decimate(lib, ctx, table, H, first_byte=0, idx=None, zero_names=()):
    """the two entry points on buffers of this test: the rows at byte `first_byte`, the output between guard bytes ->
    (status, table or None, info words).  The guards in front of and behind the output rows are checked here."""
    L = lib.load()
    n_in, stride = len(table), table.dtype.itemsize
    n = n_in if idx is None else len(idx)
    lay = lib.decimate_layout(dec.plan_decimate(table.dtype, H, zero_names))
    d_rows = ctx.alloc(first_byte + n_in * stride + 16)
    d_rows.upload(np.concatenate((np.zeros(first_byte, np.uint8), table.view(np.uint8).reshape(-1), np.zeros(16, np.uint8))))
    d_idx = ctx.alloc(4 * max(n, 1) + 16).upload(np.ascontiguousarray(idx, np.uint32)) if idx is not None and n else None
    need = C.c_int64(0)
    assert L.gsx_rows_decimate_work_dev(ctx.handle, n, C.byref(need)) == 0, lib.last_error()
    d_work = ctx.alloc(max(need.value, 16))
    words = (C.c_int64 * lib.DECIMATE_INFO_WORDS)()
    out_bytes = first_byte + n * stride + 64
    d_out = ctx.alloc(out_bytes).upload(np.full(out_bytes, GUARD, np.uint8))
    try:
        rc = L.gsx_rows_decimate_plan_dev(ctx.handle, d_rows.ptr, first_byte, stride, n_in, d_idx.ptr if d_idx is not None else None, n,
                                          C.byref(lay), d_work.ptr, need.value, words, None)
        assert rc == 0, lib.last_error()
        if words[0] != lib.DECIMATE_OK:
            ctx.synchronize()
            assert (d_out.download(np.uint8, out_bytes) == GUARD).all(), "a refused plan wrote the output"
            return int(words[0]), None, list(words)
        m = int(words[1])
        rc = L.gsx_rows_decimate_write_dev(ctx.handle, d_rows.ptr, first_byte, stride, n_in, d_idx.ptr if d_idx is not None else None, n,
                                           C.byref(lay), d_work.ptr, need.value, d_out.ptr, first_byte, m, None)
        assert rc == 0, lib.last_error()
        ctx.synchronize()
        got = d_out.download(np.uint8, out_bytes)
        assert (got[:first_byte] == GUARD).all() and (got[first_byte + m * stride:] == GUARD).all(), "bytes outside the output rows were written"
        return 0, got[first_byte:first_byte + m * stride].copy().view(table.dtype), list(words)
    finally:
        for d in (d_rows, d_idx, d_work, d_out):
            if d is not None:
                d.free()


def check(lib, ctx, table, H=dc.H, first_byte=0, idx=None, zero_names=()):
    taken = table if idx is None else table[idx]
    with np.errstate(all="ignore"):
        want, info = dn.decimate_table(taken, H, zero_names=zero_names)
    status, got, words = device_decimate(lib, ctx, table, H, first_byte, idx, zero_names)
    assert status == 0
    assert words[1:3] == [info["groups"], info["merged_groups"]] and words[4] == info["passed_through"], (words, info)
    diff = tn.same_by_class(got, want, dn.float_names(table.dtype))
    assert diff is None, diff
    return got, info


# ------------------------------------------------------------------------------------------------------------ the kernels

@pytest.fixture(scope="module")
def edge_scenes():
    """per stride: the 1000-row mixed scene with the rows the merge cannot use and non-finite SH planted, computed once"""
    out = {}
    for stride in dc.STRIDES:
        t, rows = dc.plant_unmergeable(dc.plant_nonfinite_sh(dc.scene(stride, 1000)))
        out[stride] = (t, rows)
    return out


@pytest.mark.parametrize("first_byte", (0, 5))
@pytest.mark.parametrize("stride", dc.STRIDES)
def test_every_layout_is_the_definition(lib, ctx, edge_scenes, stride, first_byte):
    t, rows = edge_scenes[stride]
    got, info = check(lib, ctx, t, first_byte=first_byte)
    assert info["merged_groups"] >= 8 and info["passed_through"] >= len(rows)
    sh = [nm for nm in t.dtype.names if nm.startswith(("f_dc_", "f_rest_"))]
    assert any(np.isnan(got[nm]).any() for nm in sh), "no non-finite SH value reached a merged row"


@pytest.mark.parametrize("shape", ("singletons", "mixed"))
@pytest.mark.parametrize("n", (0, 1, 2, 255, 256, 257, 1000))
def test_sizes_and_shapes(lib, ctx, n, shape):
    t = dc.scene(248, n, shape)
    got, info = check(lib, ctx, t)
    if shape == "singletons":
        assert got.tobytes() == t.tobytes() and info["merged_groups"] == 0


@pytest.mark.parametrize("n", (257, 513))
def test_one_cell_at_the_block_edges(lib, ctx, n):
    got, info = check(lib, ctx, dc.scene(251, n, "one_cell"), first_byte=3)
    assert len(got) == 1 and info == {"groups": 1, "merged_groups": 1, "passed_through": 0}


def test_points_on_cell_faces_and_negative_coordinates(lib, ctx):
    t = dc.scene(104, 700, on_faces=True)
    assert (t["x"] < 0).any() and (t["z"] < 0).any() and ((t["x"] / np.float32(dc.H)) % 1 == 0).all()
    check(lib, ctx, t)
    check(lib, ctx, t, H=2.0 ** -18)                    # a tiny voxel: the table again


def test_a_tiny_voxel_returns_the_table(lib, ctx):
    t = dc.scene(248, 1000)
    got, _ = check(lib, ctx, t, H=2.0 ** -18, first_byte=9)
    assert got.tobytes() == t.tobytes()


@pytest.mark.parametrize("stride", (104, 251))
def test_survivor_list_and_zeroed_fields(lib, ctx, edge_scenes, stride):
    """the key kernel reads rows idx[j]; zeroed fields are zero in merged and in copied rows: the definition on the taken table"""
    t, _ = edge_scenes[stride]
    idx = dc.survivor_list(len(t), 600)
    zero = [nm for nm in ("f_rest_%d" % i for i in range(3, 45)) if nm in t.dtype.names]
    got, _ = check(lib, ctx, t, idx=idx, zero_names=zero, first_byte=5)
    assert all((got[nm].view(np.uint32) == 0).all() for nm in zero)


def test_a_cell_beyond_the_range_is_refused(lib, ctx):
    t = dc.scene(248, 300)
    t["y"][123] = np.float32(2.0 ** 20 * dc.H)          # cell 2^20: one beyond
    status, got, _ = device_decimate(lib, ctx, t, dc.H)
    assert status == lib.DECIMATE_CELL_RANGE and got is None
    rr = lib.ResidentRows.from_host(t)
    before = lib.ResidentRows.open_count
    try:
        with pytest.raises(ValueError, match="too small for the scene's coordinates"):
            rr.decimate(dec.plan_decimate(t.dtype, dc.H))
        assert lib.ResidentRows.open_count == before
        t["y"][123] = np.float32(-(2.0 ** 20) * dc.H)   # cell -2^20 is the lowest cell
    finally:
        rr.close()
    check(lib, ctx, t)
    t["y"][123] = np.inf                                # ... and a row that is not mergeable has no cell
    check(lib, ctx, t)


def test_a_bad_list_is_refused(lib, ctx):
    t = dc.scene(68, 50)
    status, got, _ = device_decimate(lib, ctx, t, dc.H, idx=np.array([3, 2, 9], np.uint32))
    assert status == lib.DECIMATE_BAD_LIST and got is None


# ------------------------------------------------------------------------------------------------------------ the processor

def _processor(lib, dp, source, how):
    if how == "resident":
        return dp.ChainedDataProcessor(source, resident=lib.ResidentRows.from_host(source))
    return dp.ChainedDataProcessor(source) if how == "lazy" else dp.DataProcessor(source)


@pytest.mark.parametrize("how", ("resident", "lazy", "eager"))
def test_decimate_is_the_definition(lib, dp, edge_scenes, how):
    table, _ = edge_scenes[251]
    with np.errstate(all="ignore"):
        want, info = dn.decimate_table(table, dc.H)
    before = lib.ResidentRows.open_count
    source = table.copy()
    p = _processor(lib, dp, source, how)
    try:
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
            out = p.decimate(dc.H)
        assert (out is p.data) if how == "eager" else (out is None)
        assert len(p) == info["groups"] and p.last_decimate == info
        got = p.data
        assert source.tobytes() == table.tobytes(), "the caller's array was written"
        assert tn.same_by_class(got, want, dn.float_names(table.dtype)) is None
        assert (f"Decimate (voxel 0.25): Merged {len(table)} splats into {info['groups']} ({info['merged_groups']} voxels held more than one)."
                in buf.getvalue().split("\n"))
        if how == "resident":
            assert p.resident is not None and p.resident.download().tobytes() == got.tobytes()
    finally:
        p.close()
    assert lib.ResidentRows.open_count == before


def test_resident_decimate_downloads_the_merged_rows_once(lib, dp, edge_scenes, monkeypatch):
    """pending survivors and cap_sh_degree's fills are consumed in HBM: one download, of the merged row count"""
    table, _ = edge_scenes[248]
    box = (-0.6, -2.0, -2.0, 2.0, 2.0, 2.0)
    x, y, z = table["x"], table["y"], table["z"]
    with np.errstate(all="ignore"):
        cropped = table[(x >= box[0]) & (x <= box[3]) & (y >= box[1]) & (y <= box[4]) & (z >= box[2]) & (z <= box[5])]
        zero = ["f_rest_%d" % i for i in range(9, 45)]
        want, info = dn.decimate_table(cropped, dc.H, zero_names=zero)
    assert 100 < len(cropped) < len(table) and info["merged_groups"] >= 3
    seen = []
    real = lib.ResidentRows.download_into
    monkeypatch.setattr(lib.ResidentRows, "download_into", lambda self, out: seen.append(len(out)) or real(self, out))
    p = _processor(lib, dp, table.copy(), "resident")
    try:
        _quiet(lambda: p.cap_sh_degree(1))
        _quiet(lambda: p.crop_by_bbox(*box))
        _quiet(lambda: p.decimate(dc.H))
        assert seen == [] and len(p) == info["groups"]
        got = p.data
        assert seen == [info["groups"]]
        assert tn.same_by_class(got, want, dn.float_names(table.dtype)) is None
        assert p.resident.n == info["groups"] and p.data is got and seen == [info["groups"]]
    finally:
        p.close()


@pytest.mark.parametrize("how", ("resident", "lazy", "eager"))
def test_bbox_sor_decimate_limit(lib, dp, how):
    """composed: crop -> SOR -> decimate -> limit_splats equals numpy's crop, the SOR filter's own mask, the definition and
    limit_numpy chained; the budget builds its chain over the merged rows"""
    table = dc.scene(248, 1000)
    box = (-0.6, -2.0, -2.0, 2.0, 2.0, 2.0)
    x, y, z = table["x"], table["y"], table["z"]
    cropped = table[(x >= box[0]) & (x <= box[3]) & (y >= box[1]) & (y <= box[4]) & (z >= box[2]) & (z <= box[5])]
    xyz = np.ascontiguousarray(np.stack([cropped[a] for a in "xyz"], axis=1))
    kept = cropped[lib.sor_filter(xyz, 8, 1.0, want_mean=False)["mask"]]
    assert 100 < len(kept) < len(cropped) < len(table)
    with np.errstate(all="ignore"):
        merged, info = dn.decimate_table(kept, dc.H)
    N = info["groups"] // 2
    want = ln.limit_table(merged, N)
    p = _processor(lib, dp, table.copy(), how)
    try:
        _quiet(lambda: p.crop_by_bbox(*box))
        _quiet(lambda: p.remove_flyers(8, 1.0))
        _quiet(lambda: p.decimate(dc.H))
        assert len(p) == info["groups"]
        _quiet(lambda: p.limit_splats(N))
        if how == "resident":
            assert p._chain is not None and p._chain.n0 == info["groups"]
        got = p.data
        assert tn.same_by_class(got, want, dn.float_names(table.dtype)) is None
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------------------ the converter

@pytest.fixture(scope="module")
def scene_files(tmp_path_factory):
    """a 2000-row degree-3 3DGS PLY without normals, and the PLY of its decimation by the definition"""
    root = tmp_path_factory.mktemp("decimate_converter")
    read = importlib.import_module("3dgsconverter_amd.formats.ply_reader").read_ply_3dgs
    fields = [f for f in pn.canonical_fields(3) if f[0] not in ("nx", "ny", "nz")]
    t = pn.build(2000, fields, np.random.default_rng(5))
    src = dc.scene(248, 2000, seed=2)
    for nm in t.dtype.names:
        t[nm] = src[nm]
    path = str(root / "scene.ply")
    pn.write_ply(path, [("vertex", t)])
    table, _ = read(path)
    with np.errstate(all="ignore"):
        want, info = dn.decimate_table(table, dc.H)
    wanted = pn.build(len(want), fields, np.random.default_rng(6))
    for nm in wanted.dtype.names:
        wanted[nm] = want[nm]
    want_path = str(root / "wanted.ply")
    pn.write_ply(want_path, [("vertex", wanted)])
    return root, path, want_path, info


def _run(src, dst, target, resident, **kw):
    conv = importlib.import_module("3dgsconverter_amd.converter")
    c = conv.Converter(src, dst, target, resident=resident)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
        c.run(**kw)
    with open(dst, "rb") as f:
        return f.read(), buf.getvalue().split("\n")


@pytest.mark.parametrize("resident", (True, False))
@pytest.mark.parametrize("target", ("splat", "spz"))
def test_converter_writes_the_definition(lib, scene_files, target, resident):
    root, src, want_src, info = scene_files
    before = lib.ResidentRows.open_count
    got, lines = _run(src, str(root / ("got_%d.%s" % (resident, target))), target, resident, decimate_voxel_size=dc.H)
    want, _ = _run(want_src, str(root / ("want_%d.%s" % (resident, target))), target, resident)
    assert got == want and info["merged_groups"] >= 8
    assert f"Decimate (voxel 0.25): Merged 2000 splats into {info['groups']} ({info['merged_groups']} voxels held more than one)." in lines
    plain, _ = _run(src, str(root / ("plain_%d.%s" % (resident, target))), target, resident)
    tiny, _ = _run(src, str(root / ("tiny_%d.%s" % (resident, target))), target, resident, decimate_voxel_size=2.0 ** -18)
    assert tiny == plain and plain != got
    assert lib.ResidentRows.open_count == before
