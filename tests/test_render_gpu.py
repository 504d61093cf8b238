"""-m gpu: the preview renderer (csrc/render.hip) against its definition (tests/render_numpy.py), bit for bit and with no
tolerance anywhere -- the per-splat records of the plan call on their own, then the image -- at every image size that has a
single tile or partial tiles on either edge, on every row layout, SH degree and colour source, through the blend's batch loop
and its early exits, and end to end through Converter.run(preview=...)."""
import contextlib
import importlib
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ply_read_numpy as pn  # noqa: E402
import render_cases as rc  # noqa: E402
import render_numpy as rn  # noqa: E402
import transform_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu

rd = importlib.import_module("3dgsconverter_amd.render")


@pytest.fixture(scope="module")
def lib():
    lib = importlib.import_module("3dgsconverter_amd._lib")
    lib.require_hip()
    return lib


def _both(lib, table, plan, first_byte=0):
    """-> (device records, device image, render_info) of `table`"""
    rr = lib.ResidentRows.from_host(table, first_byte=first_byte)
    try:
        rec = rr.render_records(plan)
        img = rr.render(plan)
        return rec, img, rr.render_info
    finally:
        rr.close()


def _check(lib, table, plan, first_byte=0):
    want_rec = rn.records(table, plan)
    want_img = rn.image(want_rec, plan)
    rec, img, info = _both(lib, table, plan, first_byte)
    assert rec.dtype == rn.RECORD and rec.tobytes() == want_rec.tobytes()
    assert img.shape == (plan.camera.height, plan.camera.width, 3) and img.dtype == np.uint8
    assert np.array_equal(img, want_img)
    assert info["visible"] == int(want_rec["visible"].sum()) and info["rows"] == len(table)
    return want_rec, want_img, info


@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: "%dx%d" % s)
def test_every_image_size(lib, size):
    w, h = size
    t = rc.scene(tc.splat_dtype(248), 300, w, h)
    rec, img, _ = _check(lib, t, rc.plan_for(t, w, h))
    # the planted rows do what they were planted for
    assert rec["visible"][0] and (rec["x0"][0], rec["x1"][0], rec["y0"][0], rec["y1"][0]) == (0, w - 1, 0, h - 1)
    assert not rec["visible"][2:20].any() and rec["visible"][20] and rec["opac"][20] > 0.99
    assert rec["opac"][21] > rn.ALPHA_MIN > rec["opac"][22]
    if w > 16 and h > 16:
        assert rec["visible"][1] and rec["x0"][1] < 16 <= rec["x1"][1] and rec["y0"][1] < 16 <= rec["y1"][1]
    assert len(np.unique(rec["depth"][40:52])) == 1 and rec["visible"][40:52].sum() >= 2


@pytest.mark.parametrize("first_byte", (0, 5))
@pytest.mark.parametrize("stride", rc.STRIDES)
def test_every_row_layout(lib, stride, first_byte):
    t = rc.scene(tc.splat_dtype(stride), 400, 37, 21, seed=stride)
    _check(lib, t, rc.plan_for(t, 37, 21), first_byte)


@pytest.mark.parametrize("degree", (0, 1, 2, 3))
def test_every_sh_degree(lib, degree):
    t = rc.scene(tc.splat_dtype(rc.DEGREE_STRIDES[degree]), 300, 48, 40, seed=degree)
    plan = rc.plan_for(t, 48, 40)
    assert plan.degree == degree
    _check(lib, t, plan)


@pytest.mark.parametrize("cap", (0, 1, 2))
def test_sh_degree_cap(lib, cap):
    t = rc.scene(tc.splat_dtype(248), 300, 48, 40, seed=11)
    plan = rc.plan_for(t, 48, 40, sh_degree=cap)
    assert plan.degree == cap
    _, img, _ = _check(lib, t, plan)
    assert not np.array_equal(img, rn.render(t, rc.plan_for(t, 48, 40)))


def test_colour_bytes_as_the_source(lib):
    t = rc.scene(rc.RGB_ONLY, 300, 37, 21)
    plan = rc.plan_for(t, 37, 21)
    assert plan.dc[0] < 0 and plan.rgb[0] >= 0
    _check(lib, t, plan)


def test_batches_with_some_pixels_finished(lib):
    """700 faint splats over one tile: three LDS batches; the middle pixels finish inside the second batch, the outer ones never"""
    t = rc.stack(tc.splat_dtype(68), 700, 0.03, 3.0)
    plan = rc.plan_for(t, 16, 16)
    details = {}
    rn.image(rn.records(t, plan), plan, details)
    stop = details["stop_rank"]
    assert 256 < stop[8, 8] < 511 and 256 < stop[7, 7] < 511 and stop[0, 0] == -1 and stop[15, 15] == -1
    assert 20 < int((stop >= 0).sum()) < 200
    _, _, info = _check(lib, t, plan)
    assert info["instances"] == 700


def test_batches_with_every_pixel_finished(lib):
    """600 dense splats over one tile: every pixel finishes inside the first batch and the workgroup leaves the loop"""
    t = rc.stack(tc.splat_dtype(248), 600, 0.5, 40.0)
    plan = rc.plan_for(t, 16, 16)
    details = {}
    rn.image(rn.records(t, plan), plan, details)
    assert details["stop_rank"].min() >= 0 and details["stop_rank"].max() < 256
    _check(lib, t, plan)


def test_no_rows_and_nothing_visible(lib):
    bg = np.floor(np.array(rc.BACKGROUND, np.float32) * np.float32(255) + np.float32(0.5)).astype(np.uint8)
    empty = np.zeros(0, tc.splat_dtype(248))
    rec, img, info = _both(lib, empty, rc.plan_for(empty, 17, 33))
    assert len(rec) == 0 and info == {"visible": 0, "instances": 0, "rows": 0}
    assert img.shape == (33, 17, 3) and (img == bg).all()
    t = rc.scene(tc.splat_dtype(68), 64, 17, 33)
    t["z"] = -np.abs(t["z"])                                        # everything behind the camera
    _, img, info = _check(lib, t, rc.plan_for(t, 17, 33))
    assert info["visible"] == 0 and info["instances"] == 0 and (img == bg).all()


def test_work_budget_refusal_allocates_nothing(lib, monkeypatch):
    w, h = 48, 40
    t = rc.scene(tc.splat_dtype(68), 64, w, h)[:3]
    rc.place(t, [0, 1, 2], w, h, [w / 2.0] * 3, [h / 2.0] * 3, [2.0, 3.0, 4.0], 4.0 * w, 0.3)
    sizes = []
    alloc = lib.Context.alloc
    monkeypatch.setattr(lib.Context, "alloc", lambda self, nbytes: (sizes.append(int(nbytes)), alloc(self, nbytes))[1])
    rr = lib.ResidentRows.from_host(t)
    try:
        sizes.clear()
        with pytest.raises(rd.RenderRefused, match=r"48 x 40 needs 27 \(tile, splat\) instances") as e:      # 3 x 3 tiles, three splats
            rr.render(rc.plan_for(t, w, h, max_work_bytes=300))
        assert isinstance(e.value, ValueError)
        assert len(sizes) == 1                                      # the fixed workspace of the plan call, and nothing after it
        sizes.clear()
        img = rr.render(rc.plan_for(t, w, h))                       # ... and with the default budget the same rows render
        assert len(sizes) == 3 and np.array_equal(img, rn.render(t, rc.plan_for(t, w, h)))
    finally:
        rr.close()


def test_row_order_does_not_matter_between_distinct_depths(lib):
    t = rc.distinct_depths(tc.splat_dtype(104), 500, 37, 21)
    plan = rc.plan_for(t, 37, 21)
    _, img, _ = _check(lib, t, plan)
    perm = np.random.default_rng(3).permutation(len(t))
    _, img2, _ = _check(lib, np.ascontiguousarray(t[perm]), plan)
    assert np.array_equal(img, img2)


def test_processor_preview_leaves_the_table(lib):
    dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    t = rc.scene(tc.splat_dtype(248), 300, 48, 40)
    for make in (lambda: dp.DataProcessor(t.copy()), lambda: dp.ChainedDataProcessor(t.copy(), resident=lib.ResidentRows.from_host(t))):
        p = make()
        try:
            img = p.render_preview(size=(48, 40), view=(20, 10), camera=(0, 0, 0, 0, 0, 1), background=rc.BACKGROUND)
            plan = p.last_preview["plan"]
            assert np.array_equal(img, rn.render(t, plan)) and p.data.tobytes() == t.tobytes()
            assert p.last_preview["rows"] == 300 and p.last_preview["visible"] == int(rn.records(t, plan)["visible"].sum())
        finally:
            p.close()


# ------------------------------------------------------------------------------------------------------------ the converter

@pytest.fixture(scope="module")
def scene_file(tmp_path_factory):
    """a 600-row degree-3 3DGS PLY of a scene in front of the origin"""
    root = tmp_path_factory.mktemp("render_converter")
    fields = [f for f in pn.canonical_fields(3) if f[0] not in ("nx", "ny", "nz")]
    t = pn.build(600, fields, np.random.default_rng(5))
    src = rc.distinct_depths(tc.splat_dtype(248), 600, 96, 64)
    for nm in t.dtype.names:
        t[nm] = src[nm]
    path = str(root / "scene.ply")
    pn.write_ply(path, [("vertex", t)])
    return root, path


def _run(src, dst, target, resident, **kw):
    conv = importlib.import_module("3dgsconverter_amd.converter")
    c = conv.Converter(src, dst, target, resident=resident)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
        c.run(**kw)
    with open(dst, "rb") as f:
        return c, f.read(), buf.getvalue().split("\n")


@pytest.mark.parametrize("target,resident", (("splat", True), ("3dgs", True), ("3dgs", False)))
def test_converter_preview_is_the_definition(lib, scene_file, target, resident):
    from PIL import Image
    root, src = scene_file
    before = lib.ResidentRows.open_count
    ext = {"splat": "splat", "3dgs": "ply"}[target]
    png = str(root / ("p_%s_%d.png" % (target, resident)))
    c, got, lines = _run(src, str(root / ("got_%d.%s" % (resident, ext))), target, resident, preview=png, preview_size=(96, 64),
                         preview_view=(30, 15), preview_fov=60)
    _, plain, _ = _run(src, str(root / ("plain_%d.%s" % (resident, ext))), target, resident)
    assert got == plain                                             # the output file does not know about the preview
    table, plan = c.data, c.last_preview["plan"]
    prof = lib.host_table_profile(table)
    cam = rd.plan_camera(prof["lo"], prof["hi"], (96, 64), (30, 15), "-y", 60)
    assert np.array_equal(cam.view, plan.camera.view) and cam.near == plan.camera.near and (cam.fx, cam.cy) == (plan.camera.fx, plan.camera.cy)
    want_rec = rn.records(table, plan)
    want = rn.image(want_rec, plan)
    assert np.array_equal(np.asarray(Image.open(png).convert("RGB")), want) and len(np.unique(want)) > 50
    assert f"Preview: 96 x 64, {int(want_rec['visible'].sum()):,} of 600 splats visible, saved to {png}" in lines
    assert any(k.startswith("preview_") for k in c.stage_ms) and lib.ResidentRows.open_count == before
