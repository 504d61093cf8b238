"""-m gpu: the scene transform on the device (csrc/transform.hip) -- gsx_rows_transform_dev against the numpy definition of
tests/transform_numpy.py bit for bit (a NaN of the definition: any payload) at every stride, row count and first byte of the
issue, in place and into a second buffer, with the bytes around the rows untouched; ``apply_transform`` of a lazy processor over
resident rows and over a host table; and ``Converter.run(rotate=, scale=, translate=)`` end to end."""
import contextlib
import importlib
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ply_read_numpy as pn  # noqa: E402
import transform_cases as tc  # noqa: E402
import transform_numpy as tn  # noqa: E402

pytestmark = pytest.mark.gpu
tf = importlib.import_module("3dgsconverter_amd.transform")
GUARD, FILL = 0xA5, 0x5C


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


# ------------------------------------------------------------------------------------------------------------ the kernel

def _device_rows(ctx, table, first_byte, fill):
    """a device buffer: `first_byte` bytes of `fill`, the rows, 16 bytes of slack and 64 guard bytes of `fill`"""
    raw = table.view(np.uint8).reshape(-1)
    buf = np.full(first_byte + raw.size + 16 + 64, fill, np.uint8)
    buf[first_byte:first_byte + raw.size] = raw
    return ctx.alloc(buf.nbytes).upload(buf), buf


def _rows_back(d, table, first_byte, fill, what):
    """-> the rows of the buffer as a table; every byte before row 0 and behind the last row must still be `fill`"""
    nbytes = table.nbytes
    got = d.download(np.uint8, first_byte + nbytes + 80)
    assert (got[:first_byte] == fill).all(), what + ": bytes before row 0 were written"
    assert (got[first_byte + nbytes:] == fill).all(), what + ": bytes behind the last row were written"
    return got[first_byte:first_byte + nbytes].copy().view(table.dtype)


@pytest.mark.parametrize("stride", tc.STRIDES)
def test_kernel_is_the_definition(lib, ctx, stride):
    floats = tc.float_fields(tc.splat_dtype(stride))
    bad, launches = [], 0
    counts = (1, 63, 64, 65, 127, 128, 129, 1000) if stride > 256 else (1, 127, 128, 129, 1000)     # around the tile: 64 rows above 256 bytes
    for n in counts:
        table = tc.table(stride, n)
        for kind, (R, s, t) in tc.transforms().items():
            want = tn.transform_table(table, R, s, t)
            lay = lib.transform_layout(tf.plan_transform(table.dtype, R, s, t))
            for first_byte in (0, 7):
                d_in, _ = _device_rows(ctx, table, first_byte, FILL)
                d_out = ctx.alloc(first_byte + table.nbytes + 80).upload(np.full(first_byte + table.nbytes + 80, GUARD, np.uint8))
                try:
                    lib.rows_transform_dev(ctx, d_in.ptr, first_byte, stride, n, lay, d_out.ptr)      # into a second buffer
                    ctx.synchronize()
                    got = _rows_back(d_out, table, first_byte, GUARD, "second buffer")
                    same = _rows_back(d_in, table, first_byte, FILL, "source")
                    assert same.tobytes() == table.tobytes(), "the source rows were written"
                    diff = tn.same_by_class(got, want, floats)
                    if diff:
                        bad.append((n, kind, first_byte, "out", diff))
                    lib.rows_transform_dev(ctx, d_in.ptr, first_byte, stride, n, lay, d_in.ptr)       # in place
                    ctx.synchronize()
                    diff = tn.same_by_class(_rows_back(d_in, table, first_byte, FILL, "in place"), want, floats)
                    if diff:
                        bad.append((n, kind, first_byte, "in place", diff))
                    launches += 2
                finally:
                    d_in.free()
                    d_out.free()
    assert launches == len(counts) * 5 * 2 * 2
    assert not bad, (len(bad), bad[:6])


def test_kernel_refusals_and_no_rows(lib, ctx):
    table = tc.table(248, 8)
    plan = tf.plan_transform(table.dtype, tc.transforms()["rotation"][0], 2.0, (1, 2, 3))
    lay = lib.transform_layout(plan)
    d, _ = _device_rows(ctx, table, 0, FILL)
    try:
        L = lib.load()
        import ctypes as C
        call = lambda *a: L.gsx_rows_transform_dev(ctx.handle, *a)     # noqa: E731
        assert call(d.ptr, 0, 248, 0, C.byref(lay), d.ptr) == 0         # n = 0 launches nothing
        assert call(None, 0, 248, 0, C.byref(lay), None) == 0
        ctx.synchronize()
        assert _rows_back(d, table, 0, FILL, "no rows").tobytes() == table.tobytes()
        for args in ((d.ptr, 16, 248, 8, d.ptr), (d.ptr, -1, 248, 8, d.ptr), (d.ptr + 4, 0, 248, 8, d.ptr), (d.ptr, 0, 248, 8, d.ptr + 8),
                     (d.ptr, 0, 0, 8, d.ptr), (d.ptr, 0, 513, 8, d.ptr), (d.ptr, 0, 248, -1, d.ptr), (None, 0, 248, 8, d.ptr),
                     (d.ptr, 0, 244, 8, d.ptr)):       # (rows of 244 bytes: rot_3 lies outside)
            assert call(*args[:4], C.byref(lay), args[4]) != 0, args[1:4]
            assert "gsx_rows_transform_dev" in lib.last_error()
        assert call(d.ptr, 0, 248, 8, None, d.ptr) != 0
        ctx.synchronize()
        assert _rows_back(d, table, 0, FILL, "refused").tobytes() == table.tobytes()
    finally:
        d.free()


# ------------------------------------------------------------------------------------------------------------ the processor

def numpy_crop(table, box):
    x, y, z = table["x"], table["y"], table["z"]
    return table[(x >= box[0]) & (x <= box[3]) & (y >= box[1]) & (y <= box[4]) & (z >= box[2]) & (z <= box[5])]


BOX = (-3.5, -2.0, -1.0, 4.0, 3.25, 5.0)      # in the OUTPUT frame of "all_three"


@pytest.mark.parametrize("stride", (248, 251, 71))
def test_lazy_processor_transforms_resident_rows(lib, dp, stride):
    table = tc.table(stride, 1000)
    table = table[np.isfinite(table["x"]) & np.isfinite(table["y"]) & np.isfinite(table["z"])].copy()     # (a crop's own subject)
    R, s, t = tc.transforms()["all_three"]
    floats = tc.float_fields(table.dtype)
    defined = tn.transform_table(table, R, s, t)
    want = numpy_crop(defined, BOX)
    assert 10 < len(want) < len(table)
    before = lib.ResidentRows.open_count
    results = []
    for resident in (True, False):
        source = table.copy()
        p = dp.ChainedDataProcessor(source, resident=lib.ResidentRows.from_host(source)) if resident else dp.ChainedDataProcessor(source)
        try:
            assert _quiet(lambda: p.apply_transform(rotation=R, translation=t, scale=s)) is None
            _quiet(lambda: p.crop_by_bbox(*BOX))
            got = p.data
            assert source.tobytes() == table.tobytes(), "the caller's array was written"
            assert tn.same_by_class(got, want, floats) is None, tn.same_by_class(got, want, floats)
            if resident:
                assert p.resident is not None and p.resident.download().tobytes() == got.tobytes()
                assert "transform" in p.resident_ms and "take" in p.resident_ms
            else:
                assert p.resident is None
            results.append(got.tobytes())
        finally:
            p.close()
    assert results[0] == results[1] and lib.ResidentRows.open_count == before


def test_transform_alone_owes_one_download(lib, dp):
    """no filter removes a row: .data is still the transformed table, a new one; a deferred cap is filled after the transform"""
    table = tc.table(248, 300)
    R, s, t = tc.transforms()["rotation"]
    floats = tc.float_fields(table.dtype)
    zero = tc.capped_names(table.dtype, 1)
    before = lib.ResidentRows.open_count
    for capped in (False, True):
        want = tn.transform_table(table, R, s, t, zero_names=zero if capped else ())
        for resident in (True, False):
            source = table.copy()
            p = dp.ChainedDataProcessor(source, resident=lib.ResidentRows.from_host(source)) if resident else dp.ChainedDataProcessor(source)
            try:
                if capped:
                    p.cap_sh_degree(1)
                _quiet(lambda: p.apply_transform(rotation=R))
                assert len(p) == len(table)
                got = p.data
                assert got is not source and source.tobytes() == table.tobytes()
                assert tn.same_by_class(got, want, floats) is None, (capped, resident, tn.same_by_class(got, want, floats))
                assert p.data is got                                # (nothing is owed any more)
                if resident:
                    assert p.resident.download().tobytes() == got.tobytes()
                # a second transform composes on the result; a chain built afterwards gathers the new coordinates
                _quiet(lambda: p.apply_transform(translation=(1.0, 0.0, -2.0), scale=2.0))
                _quiet(lambda: p.crop_by_bbox(-1e30, -1e30, -1e30, 1e30, 1e30, 1e30))
                again = tn.transform_table(want, None, 2.0, (1.0, 0.0, -2.0))
                again = again[(again["x"] >= -1e30) & (again["x"] <= 1e30) & (again["y"] >= -1e30) & (again["y"] <= 1e30)
                              & (again["z"] >= -1e30) & (again["z"] <= 1e30)]
                assert tn.same_by_class(p.data, again, floats) is None
            finally:
                p.close()
    eager = dp.DataProcessor(table.copy())
    out = _quiet(lambda: eager.apply_transform(rotation=R))
    assert out is eager.data and tn.same_by_class(out, tn.transform_table(table, R, s, t), floats) is None
    assert lib.ResidentRows.open_count == before


def test_filters_then_transform_materialises_first(lib, dp):
    table = tc.table(248, 600)
    table = table[np.isfinite(table["x"]) & np.isfinite(table["y"]) & np.isfinite(table["z"])].copy()
    R, s, t = tc.transforms()["all_three"]
    box = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)                         # in the INPUT frame: the crop comes first here
    want = tn.transform_table(numpy_crop(table, box), R, s, t)
    for resident in (True, False):
        source = table.copy()
        p = dp.ChainedDataProcessor(source, resident=lib.ResidentRows.from_host(source)) if resident else dp.ChainedDataProcessor(source)
        try:
            _quiet(lambda: p.crop_by_bbox(*box))
            _quiet(lambda: p.apply_transform(rotation=R, translation=t, scale=s))
            assert tn.same_by_class(p.data, want, tc.float_fields(table.dtype)) is None
        finally:
            p.close()


# ------------------------------------------------------------------------------------------------------------ the converter

@pytest.fixture(scope="module")
def scene_file(tmp_path_factory):
    """a 1000-row degree-3 3DGS PLY without normals (the reader transcodes it on the device, so its rows can stay in HBM) ->
    (directory, path, the table the reader returns for it)"""
    root = tmp_path_factory.mktemp("transform_converter")
    fields = [f for f in pn.canonical_fields(3) if f[0] not in ("nx", "ny", "nz")]
    path = str(root / "scene.ply")
    pn.write_ply(path, [("vertex", pn.build(1000, fields, np.random.default_rng(21)))])
    table, _ = importlib.import_module("3dgsconverter_amd.formats.ply_reader").read_ply_3dgs(path)
    assert len(table) == 1000 and table.dtype.itemsize == 248
    return root, path, table


RUN = dict(rotate=(-90.0, 30.0, 12.5), scale=1.75, translate=(0.5, -2.0, 10.0), min_opacity=100)


def _defined_and_filtered(table):
    R = tf.rotation_from_euler_deg(*RUN["rotate"])
    defined = tn.transform_table(table, R, RUN["scale"], RUN["translate"])
    a = np.clip(RUN["min_opacity"] / 255.0, 1e-6, 1.0 - 1e-6)
    kept = defined[defined["opacity"] >= np.log(a / (1.0 - a))]
    assert 100 < len(kept) < len(table)
    return kept


@pytest.mark.parametrize("target", ("3dgs", "splat"))
def test_converter_run_end_to_end(lib, dp, scene_file, target):
    conv = importlib.import_module("3dgsconverter_amd.converter")
    root, src, table = scene_file
    want = _defined_and_filtered(table)
    before = lib.ResidentRows.open_count
    blobs, lines = [], []
    for resident in (True, False):
        dst = str(root / ("out_%s_%d%s" % (target, resident, conv.EXTENSIONS[target])))
        c = conv.Converter(src, dst, target, resident=resident)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
            c.run(**RUN)
        lines.append(buf.getvalue().split("\n"))
        assert "process_transform" in c.stage_ms, c.stage_ms
        assert ("process_take" in c.stage_ms) == resident, c.stage_ms      # (the rows stayed in HBM from the reader on, or never were)
        if target == "splat":
            assert ("write_upload" in c.stage_ms) != resident, c.stage_ms  # the resident writer path reads them where they lie
        with open(dst, "rb") as f:
            blobs.append(f.read())
        if target == "3dgs":
            back, _ = importlib.import_module("3dgsconverter_amd.formats.ply_reader").read_ply_3dgs(dst)
            assert back.dtype == table.dtype
            assert tn.same_by_class(back, want, tc.float_fields(table.dtype)) is None
    assert blobs[0] == blobs[1]
    for ln in lines:
        assert "Transform: scale 1.75, rotate [-90, 30, 12.5] deg, translate [0.5, -2, 10]" in ln
        assert "Transform applied to 1000 splats." in ln
        assert ln.index("Transform applied to 1000 splats.") < next(i for i, s in enumerate(ln) if s.startswith("Alpha Filter"))
    if target == "splat":
        p = dp.DataProcessor(want.copy())
        _quiet(p.add_rgb_from_sh)
        records = importlib.import_module("3dgsconverter_amd.formats.splat_writer").encode(p.data)
        assert blobs[0] == records.tobytes()
    assert lib.ResidentRows.open_count == before
