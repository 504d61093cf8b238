"""-m gpu: the splat budget on the device (csrc/limit.hip) -- gsx_limit_keys_dev against the numpy definition of
tests/limit_numpy.py bit for bit on the edge table, gsx_limit_select_dev against the definition for every key case, size, budget
and a survivor list with the bytes behind the mask untouched, ``limit_splats`` of a lazy processor over resident rows, over a
host table and of an eager processor, composed with the other filters, and ``Converter.run(max_splats=)`` end to end, where a
budgeted .splat file must be the head of the unbudgeted one."""
import contextlib
import ctypes as C
import importlib
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limit_cases as lc  # noqa: E402
import limit_numpy as ln  # noqa: E402
import ply_read_numpy as pn  # noqa: E402
import transform_cases as tc  # noqa: E402
import transform_numpy as tn  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 0xA5


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


# ------------------------------------------------------------------------------------------------------------ the kernels

@pytest.mark.parametrize("n", (1, 255, 256, 257, 1000))
def test_keys_kernel_is_the_definition(lib, ctx, n):
    table = lc.table(248, n)
    cols = lib.limit_columns_host(table)
    assert cols.shape == (n, 4) and cols.dtype == np.float32
    d_cols = ctx.alloc(16 * n).upload(cols)
    d_keys = ctx.alloc(4 * n + 64).upload(np.full(4 * n + 64, GUARD, np.uint8))
    try:
        lib.limit_keys_dev(ctx, d_cols.ptr, n, d_keys.ptr)
        ctx.synchronize()
        got = d_keys.download(np.uint8, 4 * n + 64)
        assert (got[4 * n:] == GUARD).all(), "bytes behind the keys were written"
        keys, want = got[:4 * n].view(np.uint32), ln.keys(table)
        bad = np.nonzero(keys != want)[0]
        assert not len(bad), (len(bad), [(int(i), hex(keys[i]), hex(want[i]), cols[i].tolist()) for i in bad[:4]])
    finally:
        d_cols.free()
        d_keys.free()


@pytest.mark.parametrize("n", lc.SIZES)
def test_select_kernel_is_the_definition(lib, ctx, n):
    """every key case at every budget, on the rows themselves and through a survivor list; guard bytes behind the mask"""
    n0 = n + n // 2 + 3
    orig = lc.survivor_list(n0, n)
    d_keys, d_orig, d_mask = ctx.alloc(4 * n0), ctx.alloc(4 * n).upload(orig), ctx.alloc(n + 64)
    bad, runs = [], 0
    try:
        for listed in (False, True):
            for name, keys in lc.key_cases(n0 if listed else n, seed=1 if listed else 0).items():
                d_keys.upload(keys)
                sub = keys[orig] if listed else keys
                for N in lc.budgets("" if listed else name, n):
                    d_mask.upload(np.full(n + 64, GUARD, np.uint8))
                    info = lib.limit_select_dev(ctx, d_keys.ptr, d_orig.ptr if listed else None, n, N, d_mask.ptr)
                    got = d_mask.download(np.uint8, n + 64)
                    runs += 1
                    assert (got[n:] == GUARD).all(), (name, N, "bytes behind the mask were written")
                    assert set(np.unique(got[:n]).tolist()) <= {0, 1}, (name, N)
                    if (int(got[:n].sum()) != min(N, n) or not np.array_equal(got[:n].view(np.bool_), ln.mask(sub, N))
                            or (info["threshold_key"], info["ties_kept"], info["kept"]) != ln.info(sub, N)):
                        bad.append((listed, name, N, info, ln.info(sub, N)))
    finally:
        for d in (d_keys, d_orig, d_mask):
            d.free()
    assert runs >= 2 * 7
    assert not bad, (len(bad), bad[:5])


def test_select_kernel_refusals_and_no_rows(lib, ctx):
    keys = np.arange(8, dtype=np.uint32)
    d_keys = ctx.alloc(32).upload(keys)
    d_mask = ctx.alloc(64).upload(np.full(64, GUARD, np.uint8))
    d_cols = ctx.alloc(128)
    try:
        L = lib.load()
        info = (C.c_uint32 * 3)(7, 7, 7)
        call = lambda *a: L.gsx_limit_select_dev(ctx.handle, *a)      # noqa: E731
        assert call(d_keys.ptr, None, 0, 3, d_mask.ptr, info) == 0    # n = 0 launches nothing
        assert list(info) == [0, 0, 0]
        assert call(None, None, 0, 3, None, info) == 0
        for args in ((None, None, 8, 3, d_mask.ptr, info), (d_keys.ptr, None, 8, 3, None, info), (d_keys.ptr, None, 8, 3, d_mask.ptr, None),
                     (d_keys.ptr, None, -1, 3, d_mask.ptr, info), (d_keys.ptr, None, 1 << 32, 3, d_mask.ptr, info),
                     (d_keys.ptr, None, 8, 0, d_mask.ptr, info), (d_keys.ptr, None, 8, -2, d_mask.ptr, info)):
            assert call(*args) != 0, args[2:4]
            assert "gsx_limit_select_dev" in lib.last_error()
        assert L.gsx_limit_select_dev(None, d_keys.ptr, None, 8, 3, d_mask.ptr, info) != 0
        for args in ((None, 8, d_keys.ptr), (d_cols.ptr, 8, None), (d_cols.ptr, -1, d_keys.ptr), (d_cols.ptr + 4, 8, d_keys.ptr)):
            assert L.gsx_limit_keys_dev(ctx.handle, *args) != 0, args[1]
            assert "gsx_limit_keys_dev" in lib.last_error()
        assert L.gsx_limit_keys_dev(ctx.handle, None, 0, None) == 0
        ctx.synchronize()
        assert (d_mask.download(np.uint8, 64) == GUARD).all(), "a refused call wrote the mask"
        out = lib.limit_select_dev(ctx, d_keys.ptr, None, 8, 100, d_mask.ptr)                         # a budget above n keeps every row
        assert (out["kept"], out["threshold_key"], out["ties_kept"]) == (8, 7, 1)
        got = d_mask.download(np.uint8, 64)
        assert (got[:8] == 1).all() and (got[8:] == GUARD).all()
    finally:
        for d in (d_keys, d_mask, d_cols):
            d.free()


# ------------------------------------------------------------------------------------------------------------ the processor

def _processor(lib, dp, source, how):
    if how == "resident":
        return dp.ChainedDataProcessor(source, resident=lib.ResidentRows.from_host(source))
    return dp.ChainedDataProcessor(source) if how == "lazy" else dp.DataProcessor(source)


@pytest.fixture(scope="module")
def tables():
    """the 5000-row tables of the processor tests and the definition's keys for them, computed once"""
    out = {}
    for stride in (248, 300):
        t = lc.table(stride, 5000)
        out[stride] = (t, ln.keys(t))
    return out


@pytest.mark.parametrize("how", ("resident", "lazy", "eager"))
@pytest.mark.parametrize("stride", (248, 300))
def test_limit_splats_is_the_definition(lib, dp, tables, stride, how):
    table, keys = tables[stride]
    n = len(table)
    before = lib.ResidentRows.open_count
    for N in (1, 2500, 4999):
        source = table.copy()
        p = _processor(lib, dp, source, how)
        try:
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
                out = p.limit_splats(N)
            assert (out is p.data) if how == "eager" else (out is None)
            assert len(p) == N
            got = p.data
            assert source.tobytes() == table.tobytes(), "the caller's array was written"
            assert got.dtype == table.dtype and got.tobytes() == table[ln.kept(keys, N)].tobytes()
            assert f"Splat Limit (max {N}): Retained {N} out of {n} splats." in buf.getvalue().split("\n")
            T, ties, _ = ln.info(keys, N)
            assert p.last_limit["ties_kept"] == ties
            want_thr = -ln.sort_unkey(np.uint32(T))
            assert p.last_limit["threshold"] == want_thr or (np.isnan(want_thr) and np.isnan(p.last_limit["threshold"]))
            if how == "resident":
                assert p.resident is not None and p.resident.download().tobytes() == got.tobytes()
        finally:
            p.close()
    assert lib.ResidentRows.open_count == before


def numpy_crop(table, box):
    x, y, z = table["x"], table["y"], table["z"]
    return table[(x >= box[0]) & (x <= box[3]) & (y >= box[1]) & (y <= box[4]) & (z >= box[2]) & (z <= box[5])]


def numpy_alpha(table, min_opacity):
    a = np.clip(min_opacity / 255.0, 1e-6, 1.0 - 1e-6)
    return table[table["opacity"] >= np.log(a / (1.0 - a))]


BOX = (-1.0, -1.25, -1.0, 1.5, 1.0, 1.0)


@pytest.mark.parametrize("how", ("resident", "lazy", "eager"))
def test_limit_after_crop_and_alpha(lib, dp, tables, how):
    """the select reads its keys through the chain's survivor list: crop -> alpha -> limit is the definition applied to the
    numpy-filtered table; and a second, smaller budget nests (b)"""
    table = tables[248][0]
    table = table[np.isfinite(table["x"]) & np.isfinite(table["y"]) & np.isfinite(table["z"])].copy()
    with np.errstate(all="ignore"):
        filtered = numpy_alpha(numpy_crop(table, BOX), 100)
    assert 600 < len(filtered) < len(table) // 2
    N1, N2 = len(filtered) // 2, len(filtered) // 7
    p = _processor(lib, dp, table.copy(), how)
    try:
        _quiet(lambda: p.crop_by_bbox(*BOX))
        _quiet(lambda: p.apply_alpha_filter(100))
        assert len(p) == len(filtered)
        _quiet(lambda: p.limit_splats(N1))
        assert len(p) == N1
        if how != "eager":
            assert p._chain is not None and p._chain.n0 == len(table), "the chain was materialised between the filters"
        _quiet(lambda: p.limit_splats(N2))
        assert p.data.tobytes() == ln.limit_table(filtered, N2).tobytes()
        assert ln.limit_table(ln.limit_table(filtered, N1), N2).tobytes() == ln.limit_table(filtered, N2).tobytes()
    finally:
        p.close()
    q = _processor(lib, dp, table.copy(), how)
    try:
        _quiet(lambda: q.crop_by_bbox(*BOX))
        _quiet(lambda: q.apply_alpha_filter(100))
        _quiet(lambda: q.limit_splats(N1))
        assert q.data.tobytes() == ln.limit_table(filtered, N1).tobytes()
    finally:
        q.close()


@pytest.mark.parametrize("how", ("resident", "lazy", "eager"))
def test_limit_after_a_transform(lib, dp, tables, how):
    """apply_transform(scale=2) adds log 2 to the scales: the budget ranks the transformed rows"""
    table = tables[248][0][:1200].copy()
    floats = tc.float_fields(table.dtype)
    want = ln.limit_table(tn.transform_table(table, None, 2.0, None), 500)
    p = _processor(lib, dp, table.copy(), how)
    try:
        _quiet(lambda: p.apply_transform(scale=2.0))
        _quiet(lambda: p.limit_splats(500))
        got = p.data
        assert len(got) == 500 and tn.same_by_class(got, want, floats) is None, tn.same_by_class(got, want, floats)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------------------ the converter

@pytest.fixture(scope="module")
def scene_file(tmp_path_factory):
    """a 3000-row degree-3 3DGS PLY without normals (the reader transcodes it on the device, so its rows can stay in HBM) ->
    (directory, path, the table the reader returns for it)"""
    root = tmp_path_factory.mktemp("limit_converter")
    fields = [f for f in pn.canonical_fields(3) if f[0] not in ("nx", "ny", "nz")]
    path = str(root / "scene.ply")
    pn.write_ply(path, [("vertex", pn.build(3000, fields, np.random.default_rng(77)))])
    table, _ = importlib.import_module("3dgsconverter_amd.formats.ply_reader").read_ply_3dgs(path)
    assert len(table) == 3000 and table.dtype.itemsize == 248
    return root, path, table


def _run(conv, src, dst, target, resident, **kw):
    c = conv.Converter(src, dst, target, resident=resident)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
        c.run(**kw)
    with open(dst, "rb") as f:
        return f.read(), buf.getvalue().split("\n"), c.stage_ms


@pytest.mark.parametrize("resident", (True, False))
def test_converter_budgeted_splat_is_the_head_of_the_unbudgeted(lib, scene_file, resident):
    """(a): the oracle is the existing writer -- the same stable order, cut at N"""
    conv = importlib.import_module("3dgsconverter_amd.converter")
    root, src, table = scene_file
    before = lib.ResidentRows.open_count
    full, _, _ = _run(conv, src, str(root / ("full_%d.splat" % resident)), "splat", resident)
    assert len(full) == 32 * 3000
    for N in (1, 1000, 2999):
        blob, lines, clocks = _run(conv, src, str(root / ("cut_%d_%d.splat" % (resident, N))), "splat", resident, max_splats=N)
        assert len(blob) == 32 * N and blob == full[:32 * N], N
        assert f"Splat Limit (max {N}): Retained {N} out of 3000 splats." in lines
        assert ("process_limit" in clocks) == resident and ("write_upload" in clocks) != resident, clocks
    assert lib.ResidentRows.open_count == before


def test_command_line_writes_the_budget(scene_file, capsys):
    """python -m 3dgsconverter_amd -i scene.ply -f splat --max_splats 1000 --force (in this process)"""
    cli = importlib.import_module("3dgsconverter_amd.cli")
    root, src, _ = scene_file
    dst = str(root / "cli_cut.splat")
    with np.errstate(all="ignore"):
        cli.main(["-i", src, "-o", dst, "-f", "splat", "--max_splats", "1000", "--force"])
    out = capsys.readouterr().out
    assert "Splat Limit (max 1000): Retained 1000 out of 3000 splats." in out.split("\n")
    assert os.path.getsize(dst) == 32000
    assert "Points: 1,000" in out                       # the target's info block describes what was written


@pytest.mark.parametrize("resident", (True, False))
def test_converter_budgeted_3dgs_is_the_definition(lib, scene_file, resident):
    conv = importlib.import_module("3dgsconverter_amd.converter")
    read = importlib.import_module("3dgsconverter_amd.formats.ply_reader").read_ply_3dgs
    root, src, table = scene_file
    for N in (1000, 5000):
        dst = str(root / ("cut_%d_%d.ply" % (resident, N)))
        _, lines, _ = _run(conv, src, dst, "3dgs", resident, max_splats=N, min_opacity=100, auto_bbox=True)
        with np.errstate(all="ignore"):
            filtered = numpy_alpha(table, 100)
        want = ln.limit_table(filtered, N)
        back, _ = read(dst)
        assert back.dtype == table.dtype and back.tobytes() == want.tobytes()
        said = next(ln_ for ln_ in lines if ln_.startswith("Splat Limit"))
        if N < len(filtered):
            assert said == f"Splat Limit (max {N}): Retained {N} out of {len(filtered)} splats."
        else:
            assert said == f"Splat Limit (max {N}): {len(filtered)} splats, nothing to remove."
        # the budget comes after the alpha filter and before the box that is printed: the box is the box of what is written
        assert lines.index(said) > next(i for i, s in enumerate(lines) if s.startswith("Alpha Filter"))
        box = next(s for s in lines if s.startswith("Auto-BBox Applied"))
        assert lines.index(said) < lines.index(box)
        assert box == "Auto-BBox Applied: [%.4f, %.4f, %.4f] to [%.4f, %.4f, %.4f]" % (*(want[a].min() for a in "xyz"), *(want[a].max() for a in "xyz"))
