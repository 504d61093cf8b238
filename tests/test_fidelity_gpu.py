"""-m gpu: the compare kernel (csrc/fidelity.hip) against its definition (tests/fidelity_numpy.py) word for word at every size
and image pair of tests/fidelity_cases.py, fidelity.compare_rows against the definition applied to the rasteriser's own
downloads, and Converter.run(fidelity=...) end to end on both the resident and the host path."""
import contextlib
import importlib
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fidelity_cases as fc  # noqa: E402
import fidelity_numpy as fn  # noqa: E402
import ply_read_numpy as pn  # noqa: E402
import render_cases as rc  # noqa: E402
import transform_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu

rd = importlib.import_module("3dgsconverter_amd.render")
vw = importlib.import_module("3dgsconverter_amd.views")
fid = importlib.import_module("3dgsconverter_amd.fidelity")
conv = importlib.import_module("3dgsconverter_amd.converter")


@pytest.fixture(scope="module")
def lib():
    lib = importlib.import_module("3dgsconverter_amd._lib")
    lib.require_hip()
    return lib


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected():
    return {c: fn.compare(*fc.pair(*c)) for c in fc.CASES}


@pytest.mark.parametrize("case", fc.CASES, ids=fc.IDS)
def test_kernel_is_the_definition(lib, ctx, expected, case):
    a, b = fc.pair(*case)
    got = lib.image_compare(a, b, ctx=ctx)
    assert got == expected[case]
    if case[0] == "identical":
        assert got["sse"] == (0, 0, 0) and got["ssim"] == (got["windows"] * fn.ONE,) * 3
    if case[0] == "complement" and got["windows"]:
        assert min(got["ssim"]) < 0
    assert lib.image_compare(b, a, ctx=ctx) == got          # every sum is symmetric, and a second launch adds into fresh words


def _figures(a, b):
    """the per-view dict the definition gives for two downloaded images"""
    return fid.view_figures(fn.compare(a, b), a.shape[1], a.shape[0])


def _same_view(got, want):
    return all(got[k] == want[k] for k in ("sse", "windows", "ssim_fixed", "width", "height", "psnr", "ssim"))


def _second_table(t, dtype, seed):
    """`t` with every seventh row dropped and the opacities perturbed, in the row layout `dtype` (shared fields copied, the
    others zero)"""
    rng = np.random.default_rng(seed)
    keep = np.arange(len(t)) % 7 != 3
    out = np.zeros(int(keep.sum()), dtype)
    for nm in dtype.names:
        if nm in t.dtype.names:
            out[nm] = t[nm][keep]
    out["opacity"] = (out["opacity"] + rng.uniform(-0.5, 0.5, len(out)).astype(np.float32)).astype(np.float32)
    return out


@pytest.mark.parametrize("strides", ((248, 71), (107, 248)), ids=lambda s: "%d-%d" % s)
def test_compare_rows_is_the_definition_on_the_downloads(lib, strides):
    t = rc.scene(tc.splat_dtype(strides[0]), 300, 48, 40, seed=strides[1])
    u = _second_table(t, tc.splat_dtype(strides[1]), strides[0])
    cams = [rc.axis_camera(48, 40), rc.axis_camera(17, 33), rd.plan_camera((-1, -1, 2), (1, 1, 5), (37, 21), view=(200, 25))]
    before = lib.ResidentRows.open_count
    ra, rb = lib.ResidentRows.from_host(t), lib.ResidentRows.from_host(u, first_byte=5)
    try:
        ms = {}
        res = fid.compare_rows(ra, rb, cams, stage_ms=ms)
        assert set(lib.RENDER_STAGES) | {"compare"} <= set(ms)
        want = []
        for cam in cams:
            a = ra.render(rd.plan_render(t.dtype, cam, background=fid.BACKGROUND))
            visible_a = ra.render_info["visible"]
            b = rb.render(rd.plan_render(u.dtype, cam, background=fid.BACKGROUND))
            want.append(dict(_figures(a, b), visible_ref=visible_a, visible_test=rb.render_info["visible"]))
        assert len(res["views"]) == 3 and all(_same_view(g, w) for g, w in zip(res["views"], want))
        assert [(v["visible_ref"], v["visible_test"]) for v in res["views"]] == [(v["visible_ref"], v["visible_test"]) for v in want]
        pooled = fid.summarise(want)
        assert all(res[k] == pooled[k] for k in ("sse", "ssim_fixed", "windows", "psnr", "ssim", "worst_view", "size", "report"))
        assert sum(res["sse"]) > 0 and res["views"][1]["width"] == 17 and res["views"][1]["height"] == 33
        # a table against itself, in another layout position: no loss
        same = fid.compare_rows(ra, ra, cams[:2])
        assert same["sse"] == (0, 0, 0) and same["ssim_fixed"] == (same["windows"] * fn.ONE,) * 3 and same["psnr"] == float("inf")
        # a refusal of either render propagates
        with pytest.raises(rd.RenderRefused):
            fid.compare_rows(ra, rb, cams, max_work_bytes=1)
    finally:
        ra.close()
        rb.close()
    assert lib.ResidentRows.open_count == before


def test_processor_compare_with(lib):
    dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    t = rc.scene(tc.splat_dtype(248), 300, 48, 40)
    u = _second_table(t, tc.splat_dtype(248), 1)
    results = []
    for make in (lambda: dp.DataProcessor(t.copy()), lambda: dp.ChainedDataProcessor(t.copy(), resident=lib.ResidentRows.from_host(t))):
        p = make()
        try:
            res = p.compare_with(u, views=2, size=(40, 24))
            assert p.data.tobytes() == t.tobytes() and p.last_fidelity is res
            results.append(res)
        finally:
            p.close()
    prof = lib.host_table_profile(t)
    cams = vw.plan_views(prof["lo"], prof["hi"], views=2, size=(40, 24))
    want = [_figures(lib.render_table(t, rd.plan_render(t.dtype, c, background=fid.BACKGROUND)),
                     lib.render_table(u, rd.plan_render(u.dtype, c, background=fid.BACKGROUND))) for c in cams]
    for res in results:
        assert all(_same_view(g, w) for g, w in zip(res["views"], want)) and len(res["views"]) == 2


# ------------------------------------------------------------------------------------------------------------ the converter

VIEWS, SIZE = 3, (48, 40)


@pytest.fixture(scope="module")
def scene_file(tmp_path_factory):
    """a 600-row degree-3 3DGS PLY of a scene in front of the origin"""
    root = tmp_path_factory.mktemp("fidelity_converter")
    fields = [f for f in pn.canonical_fields(3) if f[0] not in ("nx", "ny", "nz")]
    t = pn.build(600, fields, np.random.default_rng(5))
    src = rc.distinct_depths(tc.splat_dtype(248), 600, 96, 64)
    for nm in t.dtype.names:
        t[nm] = src[nm]
    path = str(root / "scene.ply")
    pn.write_ply(path, [("vertex", t)])
    return root, path


def _run(src, dst, target, resident, **kw):
    c = conv.Converter(src, dst, target, resident=resident)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
        c.run(**kw)
    return c, buf.getvalue().split("\n")


def _read(path, fmt):
    """the table this package's reader returns for a file, through the host path"""
    h = conv.SourceHandler(fmt)
    h.keep = False
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        return h.read(path)


def _definition(lib, ref, test, **view_kw):
    """the per-view figures of two host tables: the ring on the reference's bounds, the rasteriser's downloads, the definition"""
    prof = lib.host_table_profile(np.ascontiguousarray(ref))
    cams = vw.plan_views(prof["lo"], prof["hi"], **dict({"views": VIEWS, "size": SIZE}, **view_kw))
    return [_figures(lib.render_table(ref, rd.plan_render(ref.dtype, c, background=fid.BACKGROUND)),
                     lib.render_table(test, rd.plan_render(test.dtype, c, background=fid.BACKGROUND))) for c in cams]


def _fidelity_lines(lines):
    return [ln for ln in lines if ln.startswith("Fidelity (")]


@pytest.mark.parametrize("resident", (True, False), ids=("resident", "host"))
def test_converter_written_3dgs_has_no_loss(lib, scene_file, resident):
    root, src = scene_file
    before = lib.ResidentRows.open_count
    dst = str(root / ("w_%d.ply" % resident))
    c, lines = _run(src, dst, "3dgs", resident, fidelity="written", fidelity_views=VIEWS, fidelity_size=SIZE)
    res = c.last_fidelity
    assert len(res["views"]) == VIEWS and res["size"] == SIZE
    for v in res["views"]:
        assert v["sse"] == (0, 0, 0) and v["ssim_fixed"] == (v["windows"] * fn.ONE,) * 3 and v["windows"] == 41 * 33
        assert v["visible_ref"] == v["visible_test"] > 0
    assert _fidelity_lines(lines) == [f"Fidelity (written table vs {dst}): 3 views of 48 x 40: PSNR inf (identical images), "
                                      f"SSIM 1.0000 (worst 1.0000, view 0)"]
    assert lines.index(_fidelity_lines(lines)[0]) < lines.index(f"Conversion completed: Saved to {dst}")
    assert {"fidelity_read", "fidelity_compare", "fidelity_blend"} <= set(c.stage_ms) and lib.ResidentRows.open_count == before


@pytest.mark.parametrize("resident", (True, False), ids=("resident", "host"))
def test_converter_written_spz_is_the_definition(lib, scene_file, resident):
    root, src = scene_file
    before = lib.ResidentRows.open_count
    dst = str(root / ("w_%d.spz" % resident))
    png = str(root / ("w_%d.png" % resident))
    c, lines = _run(src, dst, "spz", resident, fidelity="written", fidelity_views=VIEWS, fidelity_size=SIZE, fidelity_image=png)
    _, plain_lines = _run(src, str(root / ("plain_%d.spz" % resident)), "spz", resident)
    with open(dst, "rb") as f, open(str(root / ("plain_%d.spz" % resident)), "rb") as g:
        assert f.read() == g.read()                              # the output file does not know about the measurement
    assert not _fidelity_lines(plain_lines)
    res = c.last_fidelity
    want = _definition(lib, c.data, _read(dst, "spz"))
    assert len(res["views"]) == VIEWS and all(_same_view(g, w) for g, w in zip(res["views"], want))
    pooled = fid.summarise(want)
    assert sum(res["sse"]) > 0 and all(res[k] == pooled[k] for k in ("sse", "ssim_fixed", "windows", "psnr", "ssim", "worst_view", "report"))
    assert _fidelity_lines(lines) == [f"Fidelity (written table vs {dst}): {pooled['report']}"]
    from PIL import Image
    img = np.asarray(Image.open(png).convert("RGB"))
    assert img.shape == (SIZE[1], 3 * SIZE[0], 3)
    a, b = img[:, :SIZE[0]], img[:, SIZE[0]:2 * SIZE[0]]
    assert _same_view(_figures(a, b), want[res["worst_view"]])
    assert np.array_equal(img[:, 2 * SIZE[0]:], np.minimum(255, 4 * np.abs(a.astype(int) - b.astype(int))))
    assert lib.ResidentRows.open_count == before


@pytest.mark.parametrize("resident", (True, False), ids=("resident", "host"))
def test_converter_source_with_decimation_is_the_definition(lib, scene_file, resident):
    root, src = scene_file
    before = lib.ResidentRows.open_count
    dst = str(root / ("s_%d.ply" % resident))
    moved = dict(rotate=(10.0, 20.0, 30.0), scale=1.5, translate=(0.5, -1.0, 2.0))
    c, lines = _run(src, dst, "3dgs", resident, fidelity="source", fidelity_views=VIEWS, fidelity_size=SIZE, fidelity_up="+z",
                    decimate_voxel_size=0.75, sh_level=1, **moved)
    assert len(c.data) < 600
    # the reference: the input file read again, moved by the run's transform, no SH cap and no filter
    tf = importlib.import_module("3dgsconverter_amd.transform")
    source = _read(src, "3dgs")
    ref = lib.rows_transform_table(source, tf.plan_transform(source.dtype, tf.rotation_from_euler_deg(*moved["rotate"]), moved["scale"],
                                                             moved["translate"]))
    want = _definition(lib, ref, _read(dst, "3dgs"), up="+z")
    res = c.last_fidelity
    assert all(_same_view(g, w) for g, w in zip(res["views"], want)) and sum(res["sse"]) > 0
    assert all(v["visible_test"] <= len(c.data) < 600 for v in res["views"])
    assert _fidelity_lines(lines) == [f"Fidelity ({src} vs {dst}): {fid.summarise(want)['report']}"]
    assert "fidelity_transform" in c.stage_ms and lib.ResidentRows.open_count == before


@pytest.mark.parametrize("resident", (True, False), ids=("resident", "host"))
def test_converter_source_without_filters_has_no_loss(lib, scene_file, resident):
    root, src = scene_file
    dst = str(root / ("n_%d.ply" % resident))
    cams = [(0.0, 0.0, -2.0, 0.0, 0.0, 2.0), (3.0, -1.0, 0.0, 0.0, 0.0, 2.0)]
    c, lines = _run(src, dst, "3dgs", resident, fidelity="source", fidelity_cameras=cams, fidelity_size=(17, 33))
    res = c.last_fidelity
    assert len(res["views"]) == 2 and res["sse"] == (0, 0, 0) and res["ssim_fixed"] == (res["windows"] * fn.ONE,) * 3
    assert res["windows"] == 2 * 10 * 26 and res["size"] == (17, 33)
    assert _fidelity_lines(lines)[0].endswith("2 views of 17 x 33: PSNR inf (identical images), SSIM 1.0000 (worst 1.0000, view 0)")


@pytest.mark.parametrize("resident", (True, False), ids=("resident", "host"))
def test_render_refusal_is_a_warning(lib, scene_file, resident, monkeypatch):
    root, src = scene_file
    before = lib.ResidentRows.open_count
    dst = str(root / ("r_%d.spz" % resident))
    monkeypatch.setattr(fid, "MAX_WORK_BYTES", 1)
    c, lines = _run(src, dst, "spz", resident, fidelity="written", fidelity_views=VIEWS, fidelity_size=SIZE)
    assert c.last_fidelity == {} and not _fidelity_lines(lines)
    warn = [ln for ln in lines if ln.startswith("Warning: fidelity not measured: ")]
    assert len(warn) == 1 and "max_work_bytes is 1" in warn[0]
    assert f"Conversion completed: Saved to {dst}" in lines and os.path.getsize(dst) > 0
    assert len(_read(dst, "spz")) == 600 and lib.ResidentRows.open_count == before
