"""-m gpu: the view scores (csrc/render.hip's score kernel) against their definition (tests/view_scores_numpy.py):
the device's peak and total equal the twin's byte for byte, with no tolerance anywhere -- at every image size that has a single
tile or partial tiles, on packed row layouts, through the batch loop and its early exits, past 32 bits of total, over several
views in either order -- and then the two selections through DataProcessor in its three executors and Converter.run."""
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
import view_scores_numpy as vn  # noqa: E402

pytestmark = pytest.mark.gpu

rd = importlib.import_module("3dgsconverter_amd.render")
vw = importlib.import_module("3dgsconverter_amd.views")
dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")


@pytest.fixture(scope="module")
def lib():
    lib = importlib.import_module("3dgsconverter_amd._lib")
    lib.require_hip()
    return lib


def _twin(table, cameras):
    """the twin's per-view scores of `table`; its plans carry a colour source (render_numpy.records evaluates one), which plays
    no part"""
    plans = [rd.plan_render(table.dtype, cam, sh_degree=0) for cam in cameras]
    recs = [rn.records(table, plan) for plan in plans]
    return [vn.scores(rec, plan) for rec, plan in zip(recs, plans)], recs


def _device(lib, table, cameras, first_byte=0, **kw):
    rr = lib.ResidentRows.from_host(table, first_byte=first_byte)
    try:
        peak, total = rr.view_scores([vw.plan_scores(table.dtype, cam, **kw) for cam in cameras])
        return peak, total, rr.view_scores_info
    finally:
        rr.close()


def _check(lib, table, cameras, first_byte=0):
    per_view, recs = _twin(table, cameras)
    want_peak, want_total = vn.accumulate(per_view, len(table))
    peak, total, info = _device(lib, table, cameras, first_byte)
    assert peak.dtype == np.float32 and total.dtype == np.uint64 and peak.shape == total.shape == (len(table),)
    assert peak.tobytes() == want_peak.tobytes() and total.tobytes() == want_total.tobytes()
    assert info["visible"] == [int(r["visible"].sum()) for r in recs] and info["rows"] == len(table) and info["views"] == len(cameras)
    return want_peak, want_total, info


@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: "%dx%d" % s)
def test_every_image_size(lib, size):
    w, h = size
    t = rc.scene(tc.splat_dtype(248), 300, w, h)
    peak, total, _ = _check(lib, t, [rc.axis_camera(w, h)])
    assert (peak[2:20] == 0).all() and (total[2:20] == 0).all() and peak[22] == 0 and total[22] == 0
    assert peak[21] > 0 and total[21] > 0
    if w > 16 or h > 16:
        assert total[0] > 0                                         # row 0 covers every tile: the sum across workgroups


@pytest.mark.parametrize("stride,first_byte", ((71, 5), (248, 0)))
def test_row_layouts(lib, stride, first_byte):
    t = rc.scene(tc.splat_dtype(stride), 400, 37, 21, seed=stride)
    _check(lib, t, [rc.axis_camera(37, 21)], first_byte)


def test_a_table_without_colours_scores_the_same(lib):
    full = rc.scene(tc.splat_dtype(68), 300, 37, 21)
    bare = np.zeros(len(full), np.dtype([(nm, "<f4") for nm in rc.GEOMETRY]))
    for nm in rc.GEOMETRY:
        bare[nm] = full[nm]
    per_view, _ = _twin(full, [rc.axis_camera(37, 21)])
    peak, total, _ = _device(lib, bare, [rc.axis_camera(37, 21)])
    assert peak.tobytes() == per_view[0][0].tobytes() and total.tobytes() == per_view[0][1].tobytes() and (peak > 0).sum() > 50


def test_batches_with_some_pixels_finished(lib):
    """700 faint splats over one tile: three LDS batches, the middle pixels finish inside the second"""
    t = rc.stack(tc.splat_dtype(68), 700, 0.03, 3.0)
    peak, total, info = _check(lib, t, [rc.axis_camera(16, 16)])
    assert info["instances"] == [700] and (total > 0).sum() > 512      # rows of the third batch still add to the outer pixels


def test_batches_with_every_pixel_finished(lib):
    """600 dense splats over one tile: T halves per splat and falls under 1e-4 after about 14, so every pixel finishes inside
    the first batch and the workgroup leaves the loop"""
    t = rc.stack(tc.splat_dtype(248), 600, 0.5, 40.0)
    peak, total, _ = _check(lib, t, [rc.axis_camera(16, 16)])
    assert (total == 0).sum() > 500 and (total > 0).sum() >= 10


def test_totals_beyond_32_bits(lib):
    """one opaque splat over 64 x 64 pixels: 4096 weights of 0.99 in sixteen tiles"""
    t = rc.scene(tc.splat_dtype(68), 64, 64, 64)[:1]
    rc.place(t, [0], 64, 64, [32.0], [32.0], 2.0, 4000.0, 0.5, quat=(1, 0, 0, 0))
    t["opacity"][0] = np.float32(20.0)
    peak, total, _ = _check(lib, t, [rc.axis_camera(64, 64)])
    assert int(total[0]) > 2 ** 32 and peak[0] == np.float32(0.99)


def test_several_views_in_either_order(lib):
    w, h = 48, 40
    t = rc.scene(tc.splat_dtype(248), 300, w, h)
    a = rc.axis_camera(w, h)
    view = np.eye(3, 4)
    view[0, 3] = 0.3
    b = rd.Camera(w, h, view, (-0.3, 0.0, 0.0), a.fx, a.fy, a.cx, a.cy, a.tan_fovx, a.tan_fovy, a.near)
    per_view, _ = _twin(t, [a, b])
    assert per_view[0][1].tobytes() != per_view[1][1].tobytes()
    want_peak, want_total = vn.accumulate(per_view)
    assert want_peak.tobytes() == np.maximum(per_view[0][0], per_view[1][0]).tobytes()
    assert want_total.tobytes() == (per_view[0][1] + per_view[1][1]).tobytes()
    for cams in ([a, b], [b, a]):
        peak, total, info = _device(lib, t, cams)
        assert peak.tobytes() == want_peak.tobytes() and total.tobytes() == want_total.tobytes() and info["views"] == 2


def test_no_rows_and_nothing_visible(lib):
    empty = np.zeros(0, tc.splat_dtype(248))
    peak, total, info = _device(lib, empty, [rc.axis_camera(17, 33)])
    assert len(peak) == 0 and len(total) == 0 and info == {"views": 1, "visible": [0], "instances": [0], "rows": 0}
    t = rc.scene(tc.splat_dtype(68), 64, 17, 33)
    t["z"] = -np.abs(t["z"])                                        # everything behind the camera
    peak, total, info = _check(lib, t, [rc.axis_camera(17, 33)])
    assert not peak.any() and not total.any() and info["instances"] == [0]     # no instance: no sort, no score kernel


def test_workspaces_and_the_refused_view(lib, monkeypatch):
    w, h = 48, 40
    t = rc.scene(tc.splat_dtype(68), 64, w, h)[:3]
    rc.place(t, [0, 1, 2], w, h, [w / 2.0] * 3, [h / 2.0] * 3, [2.0, 3.0, 4.0], 4.0 * w, 0.3)
    sizes = []
    alloc = lib.Context.alloc
    monkeypatch.setattr(lib.Context, "alloc", lambda self, nbytes: (sizes.append(int(nbytes)), alloc(self, nbytes))[1])
    cam = rc.axis_camera(w, h)
    rr = lib.ResidentRows.from_host(t)
    try:
        sizes.clear()
        with pytest.raises(rd.RenderRefused, match=r"view 1 of 2: an image of 48 x 40 needs 27 \(tile, splat\) instances"):
            rr.view_scores([vw.plan_scores(t.dtype, cam, max_work_bytes=300)] * 2)
        assert len(sizes) == 3                                      # peak, total, the fixed workspace -- and nothing of the refused view
        sizes.clear()
        rr.view_scores([vw.plan_scores(t.dtype, cam)] * 4)
        assert len(sizes) == 4                                      # ... and ONE instance workspace for four equal views
    finally:
        rr.close()
    # the instance workspace grows to the largest view: one tile first (every row has at most one instance), then 120 tiles
    scene = rc.scene(tc.splat_dtype(68), 300, w, h)
    cams = [rc.axis_camera(16, 16), rc.axis_camera(192, 160), rc.axis_camera(16, 16)]
    rr = lib.ResidentRows.from_host(scene)
    try:
        sizes.clear()
        rr.view_scores([vw.plan_scores(scene.dtype, c) for c in cams])
        inst = rr.view_scores_info["instances"]
        assert inst[0] == inst[2] <= 300 and inst[1] > 8 * inst[0]
        assert len(sizes) == 5 and sizes[4] > sizes[3]
    finally:
        rr.close()
    _check(lib, scene, cams)


# ------------------------------------------------------------------------------------------------------------ the processor

CAMERAS = [(0.0, 0.0, 0.0, 0.0, 0.0, 1.0), (0.3, 0.0, 0.0, 0.3, 0.0, 1.0)]
VIEW_KW = dict(size=(48, 40), cameras=CAMERAS, fov=60)
BOX = (-100.0, -100.0, -100.0, 100.0, 100.0, 5.0)


def _cameras(table, **kw):
    prof_lo, prof_hi = (0, 0, 0), (0, 0, 0)                          # (explicit cameras do not look at the box)
    return vw.plan_views(prof_lo, prof_hi, **kw)


@pytest.fixture(scope="module")
def processor_case():
    """the 2,000-row scene, cropped, and the twin's two passes: the threshold, then the budget on a new scoring of what is left"""
    t = rc.scene(tc.splat_dtype(248), 2000, 48, 40)
    with np.errstate(all="ignore"):
        inside = ((t["x"] >= BOX[0]) & (t["x"] <= BOX[3]) & (t["y"] >= BOX[1]) & (t["y"] <= BOX[4]) & (t["z"] >= BOX[2]) & (t["z"] <= BOX[5]))
    t1 = t[inside]
    cams = _cameras(t1, **VIEW_KW)
    rows1, peak1, _ = vn.select(t1, [rd.plan_render(t.dtype, c, sh_degree=0) for c in cams], 0.01)
    t2 = t1[rows1]
    rows2, _, total2 = vn.select(t2, [rd.plan_render(t.dtype, c, sh_degree=0) for c in cams], None, 500)
    shared, _, _ = vn.select(t1, [rd.plan_render(t.dtype, c, sh_degree=0) for c in cams], 0.01, 500)
    vis1 = [int(rn.records(t1, rd.plan_render(t.dtype, c, sh_degree=0))["visible"].sum()) for c in cams]
    assert 100 < len(t) - len(t1) and 600 < len(t2) < len(t1) - 100 and len(rows2) == 500 and not np.array_equal(t2[rows2], t1[shared])
    return {"t": t, "t1": t1, "t2": t2, "t3": t2[rows2], "shared": t1[shared], "never_seen": int((peak1 == 0).sum()), "visible": vis1,
            "last_total": int(total2[rows2].min())}


def _processors(lib, t):
    return (("eager", lambda: dp.DataProcessor(t.copy())), ("lazy host", lambda: dp.DataProcessor(t.copy(), lazy=True)),
            ("lazy resident", lambda: dp.ChainedDataProcessor(t.copy(), resident=lib.ResidentRows.from_host(t))))


def test_processor_in_three_executors(lib, processor_case, capsys):
    c = processor_case
    before = lib.ResidentRows.open_count
    for name, make in _processors(lib, c["t"]):
        p = make()
        try:
            p.crop_by_bbox(*BOX)
            p.prune_by_views(0.01, **VIEW_KW)
            out = capsys.readouterr().out
            assert p.last_view_scores == {"views": 2, "visible": c["visible"], "never_seen": c["never_seen"],
                                          "removed": len(c["t1"]) - len(c["t2"]), "rows": len(c["t1"])}, name
            assert (f"View Prune (2 views, 48 x 40, min 0.01): Retained {len(c['t2'])} out of {len(c['t1'])} splats "
                    f"({c['never_seen']} never seen).") in out, name
            assert len(p) == len(c["t2"])
            p.limit_splats(500, rank_by="views", **VIEW_KW)
            assert "Splat Limit (max 500, by 2 views, 48 x 40): Retained 500 out of %d splats." % len(c["t2"]) in capsys.readouterr().out
            assert p.data.dtype == c["t"].dtype and p.data.tobytes() == c["t3"].tobytes(), name
            assert p.last_limit["rank_by"] == "views" and p.last_limit["ties_kept"] >= 1
            assert p.last_limit["threshold"] == np.array([vn.fbits(c["last_total"])], np.uint32).view(np.float32)[0]
            assert p.last_view_scores["rows"] == len(c["t2"]) and p.last_view_scores["removed"] == len(c["t2"]) - 500
            if name == "lazy resident":
                assert p.resident is not None and p.resident.download().tobytes() == c["t3"].tobytes()
        finally:
            p.close()
    assert lib.ResidentRows.open_count == before


def test_processor_one_pass_serves_both(lib, processor_case):
    c = processor_case
    for name, make in _processors(lib, c["t"]):
        p = make()
        try:
            p.cap_sh_degree(1)                                      # (a deferred fill in the lazy executors)
            p.crop_by_bbox(*BOX)
            p.prune_by_views(0.01, max_count=500, **VIEW_KW)
            want = c["shared"].copy()
            for k in range(9, 45):
                want["f_rest_%d" % k] = 0
            assert p.data.tobytes() == want.tobytes(), name
            assert p.last_limit["rank_by"] == "views" and p.last_view_scores["removed"] == len(c["t1"]) - 500
            p.limit_splats(400)                                     # the default ranking is as it was
            assert p.last_limit["rank_by"] == "size" and len(p.data) == 400
        finally:
            p.close()


def test_refused_view_leaves_the_table(lib, processor_case, capsys):
    c = processor_case
    for name, make in _processors(lib, c["t"]):
        p = make()
        try:
            p.crop_by_bbox(*BOX)
            p.prune_by_views(0.01, max_work_bytes=1, **VIEW_KW)
            assert "Warning: View Prune skipped, the table is unchanged: view 1 of 2: an image of 48 x 40 needs" in capsys.readouterr().out
            p.limit_splats(10, rank_by="views", max_work_bytes=1, **VIEW_KW)
            assert "Warning: Splat Limit skipped, the table is unchanged:" in capsys.readouterr().out
            assert p.data.tobytes() == c["t1"].tobytes() and not hasattr(p, "last_view_scores"), name
        finally:
            p.close()


# ------------------------------------------------------------------------------------------------------------ the converter

@pytest.fixture(scope="module")
def scene_file(tmp_path_factory):
    """a 600-row degree-3 3DGS PLY of a scene in front of the origin"""
    root = tmp_path_factory.mktemp("view_scores_converter")
    fields = [f for f in pn.canonical_fields(3) if f[0] not in ("nx", "ny", "nz")]
    t = pn.build(600, fields, np.random.default_rng(5))
    src = rc.scene(tc.splat_dtype(248), 600, 96, 64)
    for nm in t.dtype.names:
        t[nm] = src[nm]
    path = str(root / "scene.ply")
    pn.write_ply(path, [("vertex", t)])
    return root, path, t


def _run(src, dst, target, resident, **kw):
    conv = importlib.import_module("3dgsconverter_amd.converter")
    c = conv.Converter(src, dst, target, resident=resident)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
        c.run(**kw)
    with open(dst, "rb") as f:
        return c, f.read(), buf.getvalue().split("\n")


@pytest.mark.parametrize("target,resident", (("splat", True), ("splat", False), ("3dgs", True), ("3dgs", False)))
def test_converter_writes_the_twins_rows(lib, scene_file, target, resident):
    root, src, t = scene_file
    before = lib.ResidentRows.open_count
    ext = {"splat": "splat", "3dgs": "ply"}[target]
    cams = vw.plan_views((0, 0, 0), (0, 0, 0), size=(96, 64), cameras=CAMERAS)
    rows, peak, _ = vn.select(t, [rd.plan_render(t.dtype, c, sh_degree=0) for c in cams], 0.02, 150)
    assert len(rows) == 150 and int(vn.keep_peak(peak, 0.02).sum()) > 200
    kept_path = str(root / ("kept_%s_%d.ply" % (target, resident)))
    pn.write_ply(kept_path, [("vertex", t[rows])])
    c, got, lines = _run(src, str(root / ("got_%d.%s" % (resident, ext))), target, resident, min_contribution=0.02, max_splats=150,
                         rank_by="views", views_size=(96, 64), view_cameras=CAMERAS)
    c2, want, _ = _run(kept_path, str(root / ("want_%d.%s" % (resident, ext))), target, resident)
    assert got == want and c.data.tobytes() == c2.data.tobytes() and len(c.data) == 150
    n_seen = int(vn.keep_peak(peak, 0.02).sum())
    assert (f"View Prune (2 views, 96 x 64, min 0.02): Retained {n_seen} out of 600 splats ({int((peak == 0).sum())} never seen).") in lines
    assert f"Splat Limit (max 150, by 2 views, 96 x 64): Retained 150 out of {n_seen} splats." in lines
    assert lib.ResidentRows.open_count == before
