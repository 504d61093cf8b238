"""-m "not gpu": the preview renderer's host side, no device touched -- the definition (tests/render_numpy.py) against closed
forms that can be derived by hand, the camera (render.plan_camera), the plan's refusals (render.plan_render), the PNG writer
against PIL, the command line's flags, and Converter.run(preview=...) with the renderer stubbed."""
import importlib
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ply_read_numpy as pn  # noqa: E402
import render_cases as rc  # noqa: E402
import render_numpy as rn  # noqa: E402
import transform_cases as tc  # noqa: E402

lib = importlib.import_module("3dgsconverter_amd._lib")
rd = importlib.import_module("3dgsconverter_amd.render")

W = 17                              # odd: the optical axis meets the middle pixel, (8, 8)
MID = 8
DT = tc.splat_dtype(68)             # degree 0: the colour is 0.5 + C0 f_dc


@pytest.fixture(scope="module")
def cli():
    return importlib.import_module("3dgsconverter_amd.cli")


def sigmoid(o):
    return 1.0 / (1.0 + math.exp(-o))


def splats(rows):
    """rows of (x, y, z, (s0, s1, s2), (qw, qx, qy, qz), opacity, (r, g, b)) as a degree-0 table"""
    t = np.zeros(len(rows), DT)
    for k, (x, y, z, s, q, o, col) in enumerate(rows):
        t["x"][k], t["y"][k], t["z"][k], t["opacity"][k] = x, y, z, o
        for i in range(3):
            t["scale_%d" % i][k] = math.log(s[i])
            t["f_dc_%d" % i][k] = (col[i] - 0.5) / rn.C0
        for i in range(4):
            t["rot_%d" % i][k] = q[i]
    return t


def plan_of(t, w=W, h=W, background=(0, 0, 0)):
    return rd.plan_render(t.dtype, rc.axis_camera(w, h), background=background)


# ------------------------------------------------------------------------------------------------------------ the definition

def test_one_isotropic_splat_on_the_axis():
    s, z, o, col = 0.4, 4.0, 1.0, (0.8, 0.4, 0.2)
    t = splats([(0, 0, z, (s, s, s), (1, 0, 0, 0), o, col)])
    plan = plan_of(t)
    rec = rn.records(t, plan)
    img = rn.image(rec, plan)
    f = rc.focal(W, W)
    var = (f * s / z) ** 2 + 0.3                                    # the 2D variance, both axes
    r = math.ceil(3.0 * math.sqrt(var + math.sqrt(0.1)))            # lambda_max: mid + sqrt(max(0.1, mid^2 - det)), the root's floor acting
    assert rec["visible"][0] and (rec["u"][0], rec["v"][0]) == (MID, MID) and rec["depth"][0] == z
    assert (rec["x0"][0], rec["x1"][0], rec["y0"][0], rec["y1"][0]) == (MID - r, MID + r, MID - r, MID + r) and MID - r > 0
    assert rec["b"][0] == 0 and abs(rec["a"][0] * var - 1) < 1e-6 and rec["a"][0] == rec["c"][0]
    for ch in range(3):
        assert img[MID, MID, ch] == math.floor(min(0.99, sigmoid(o)) * col[ch] * 255 + 0.5)
    assert np.array_equal(img, img[::-1]) and np.array_equal(img, img[:, ::-1]) and np.array_equal(img, img.transpose(1, 0, 2))
    assert not img[:MID - r].any() and not img[:, MID + r + 1:].any() and img[MID, MID - r + 1:MID + r].all()
    # one pixel off the centre: exp(-0.5 / var) of the peak
    want = sigmoid(o) * math.exp(-0.5 / var) * col[0] * 255
    assert abs(int(img[MID, MID + 1, 0]) - want) <= 0.51


def test_the_opacity_clamp_and_the_alpha_floor():
    hot = splats([(0, 0, 4.0, (0.4,) * 3, (1, 0, 0, 0), 20.0, (1.0, 1.0, 1.0))])
    assert rn.render(hot, plan_of(hot))[MID, MID, 0] == math.floor(0.99 * 255 + 0.5)
    for o, seen in ((-5.5, True), (-5.6, False)):                  # sigmoid: 0.00407 | 0.00368, around 1/255 = 0.00392
        faint = splats([(0, 0, 4.0, (0.4,) * 3, (1, 0, 0, 0), o, (1.0, 1.0, 1.0))])
        img = rn.render(faint, plan_of(faint, background=(1, 0, 0)))
        assert (img[MID, MID].tolist() == [255, 1, 1]) == seen and (img[MID, MID].tolist() == [255, 0, 0]) == (not seen)


def test_a_quarter_turn_about_the_view_axis_transposes_the_image():
    base = (0, 0, 3.0, (0.9, 0.15, 0.3), (1, 0, 0, 0), 2.0, (0.9, 0.5, 0.1))
    turned = base[:4] + ((1, 0, 0, 1),) + base[5:]                  # (w, z) = (1, 1): 90 degrees about z once normalised
    a, b = splats([base]), splats([turned])
    img_a, img_b = rn.render(a, plan_of(a)), rn.render(b, plan_of(b))
    assert np.array_equal(img_b, img_a.transpose(1, 0, 2)) and not np.array_equal(img_a, img_b)
    assert (img_a[MID, :, 0] > 0).sum() > (img_a[:, MID, 0] > 0).sum() + 4     # the long axis lies along x before the turn


def test_two_splats_on_one_ray():
    near_ = (0, 0, 2.0, (0.2,) * 3, (1, 0, 0, 0), 0.5, (1.0, 0.0, 0.0))
    far_ = (0, 0, 5.0, (0.5,) * 3, (1, 0, 0, 0), 1.5, (0.0, 0.0, 1.0))
    t = splats([near_, far_])
    img = rn.render(t, plan_of(t))
    a1, a2 = sigmoid(0.5), sigmoid(1.5)
    assert img[MID, MID].tolist() == [math.floor(a1 * 255 + 0.5), 0, math.floor(a2 * (1 - a1) * 255 + 0.5)]
    swapped = splats([far_, near_])
    assert np.array_equal(rn.render(swapped, plan_of(swapped)), img)


def test_equal_depths_fall_to_the_lower_row():
    red = (0, 0, 3.0, (0.3,) * 3, (1, 0, 0, 0), 0.5, (1.0, 0.0, 0.0))
    blue = red[:6] + ((0.0, 0.0, 1.0),)
    a = sigmoid(0.5)
    first, second = math.floor(a * 255 + 0.5), math.floor(a * (1 - a) * 255 + 0.5)
    t = splats([red, blue])
    assert rn.render(t, plan_of(t))[MID, MID].tolist() == [first, 0, second]
    t = splats([blue, red])
    assert rn.render(t, plan_of(t))[MID, MID].tolist() == [second, 0, first]


def test_invisible_rows_leave_zero_records_and_the_background():
    t = rc.scene(tc.splat_dtype(248), 64, 37, 21)
    plan = rc.plan_for(t, 37, 21)
    rec = rn.records(t, plan)
    assert not rec["visible"][2:20].any() and not rec[2:20].tobytes().strip(b"\0") and rec["visible"][[0, 20, 21, 22]].all()
    t["z"] = -np.abs(t["z"])
    img = rn.render(t, plan)
    assert (img == np.array([51, 128, 255], np.uint8)).all()       # floor(0.2 * 255 + 0.5), floor(127.5 + 0.5), 255


def test_the_pixel_rectangle_is_the_footprint():
    """a pixel outside a splat's rectangle never receives it, whatever tile it lies in"""
    t = splats([(0, 0, 4.0, (0.4,) * 3, (1, 0, 0, 0), 3.0, (1.0, 1.0, 1.0))])
    plan = plan_of(t, 48, 40)
    rec = rn.records(t, plan)
    img = rn.image(rec, plan)
    inside = np.zeros((40, 48), bool)
    inside[rec["y0"][0]:rec["y1"][0] + 1, rec["x0"][0]:rec["x1"][0] + 1] = True
    assert not img[~inside].any() and img[rec["y0"][0], rec["x0"][0] + (rec["x1"][0] - rec["x0"][0]) // 2].any()


# ------------------------------------------------------------------------------------------------------------ the camera

def _project(cam, p):
    pc = cam.view @ np.append(np.asarray(p, np.float64), 1.0)
    return cam.fx * pc[0] / pc[2] + cam.cx, cam.fy * pc[1] / pc[2] + cam.cy, pc[2]


@pytest.mark.parametrize("size", ((960, 540), (64, 200), (1, 1)))
@pytest.mark.parametrize("view", ((35, 20), (-170, -60), (0, 90), (90, -90)))
def test_auto_frame_holds_the_box(size, view):
    lo, hi = (-3.0, 0.5, 10.0), (5.0, 1.5, 14.0)
    cam = rd.plan_camera(lo, hi, size, view=view)
    w, h = size
    for corner in [(x, y, z) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]:
        u, v, z = _project(cam, corner)
        assert -0.5 <= u <= w - 0.5 and -0.5 <= v <= h - 0.5 and z > cam.near
    R = 0.5 * math.sqrt(8.0 ** 2 + 1.0 ** 2 + 4.0 ** 2)
    fovy = math.radians(50)
    fovx = 2 * math.atan(math.tan(fovy / 2) * w / h)
    dist = 1.05 * R / math.sin(min(fovx, fovy) / 2)
    centre = np.array([1.0, 1.0, 12.0])
    assert math.isclose(np.linalg.norm(cam.eye - centre), dist, rel_tol=1e-12) and math.isclose(cam.near, 0.01 * dist, rel_tol=1e-12)
    u, v, z = _project(cam, centre)
    assert math.isclose(u, (w - 1) / 2, abs_tol=1e-9) and math.isclose(v, (h - 1) / 2, abs_tol=1e-9) and math.isclose(z, dist, rel_tol=1e-12)
    R3 = cam.view[:, :3]
    assert np.allclose(R3 @ R3.T, np.eye(3), atol=1e-12) and np.linalg.det(R3) > 0
    assert (cam.fx, cam.fy) == (w / (2 * cam.tan_fovx), h / (2 * cam.tan_fovy)) and math.isclose(cam.tan_fovy, math.tan(fovy / 2))


@pytest.mark.parametrize("up", ("+x", "-x", "+y", "-y", "+z", "-z"))
def test_up_is_up_in_the_image(up):
    cam = rd.plan_camera((-1, -1, -1), (1, 1, 1), (200, 100), view=(35, 20), up=up)
    above = rd.up_vector(up) * 0.5
    u, v, _ = _project(cam, above)
    assert v < cam.cy - 5 and math.isclose(u, cam.cx, abs_tol=1e-9)
    assert float(cam.eye @ rd.up_vector(up)) > 0                    # a positive elevation looks down on the scene
    assert np.array_equal(rd.up_vector(up[1]), rd.up_vector("+" + up[1]))       # a bare axis is the positive one


def test_explicit_camera_degenerate_box_and_refusals():
    cam = rd.plan_camera((0, 0, 0), (9, 9, 9), (64, 48), camera=(1, 2, 3, 1, 2, 13), fov=90)
    assert np.allclose(cam.view @ [1, 2, 3, 1], 0) and np.allclose(cam.view @ [1, 2, 13, 1], [0, 0, 10]) and math.isclose(cam.near, 0.1)
    assert np.allclose(cam.view @ [2, 2, 13, 1], [1, 0, 10]) and np.allclose(cam.view @ [1, 3, 13, 1], [0, 1, 10])    # x right, y down
    assert math.isclose(cam.fy, 24.0) and (cam.cx, cam.cy) == (31.5, 23.5)
    point = rd.plan_camera((2, 2, 2), (2, 2, 2), (100, 100))
    assert math.isclose(np.linalg.norm(point.eye - 2.0), 1.05 / math.sin(math.radians(25)), rel_tol=1e-12)
    nan = float("nan")
    holed = rd.plan_camera((nan, 0, 0), (nan, 2, 4), (100, 100))
    assert np.all(np.isfinite(holed.view)) and np.allclose(_project(holed, (0, 1, 2))[:2], (49.5, 49.5))
    for bad in ({"size": (0, 5)}, {"size": (8193, 5)}, {"size": (10.5, 5)}, {"fov": 0}, {"fov": 170}, {"fov": "wide"}, {"up": "w"},
                {"view": (0, 91)}, {"view": (nan, 0)}, {"camera": (1, 2, 3, 1, 2, 3)}, {"camera": (1, 2, 3)}, {"camera": (nan,) * 6}):
        kw = dict({"size": (10, 10)}, **bad)
        with pytest.raises(ValueError, match="render: "):
            rd.plan_camera((0, 0, 0), (1, 1, 1), **kw)


# ------------------------------------------------------------------------------------------------------------ the plan

def test_plan_offsets_and_refusals():
    cam = rc.axis_camera(37, 21)
    dt = tc.splat_dtype(251)
    p = rd.plan_render(dt, cam)
    assert (p.degree, p.m, len(p.rest)) == (3, 15, 45) and p.dc == tuple(dt.fields[nm][1] for nm in rd.DC) and p.rgb == (-1, -1, -1)
    assert p.xyz == (0, 4, 8) and p.opacity == dt.fields["opacity"][1] and p.max_work_bytes == 4 << 30
    assert rd.plan_render(dt, cam, sh_degree=1).degree == 1 and rd.plan_render(tc.splat_dtype(104), cam, sh_degree=3).degree == 1
    p = rd.plan_render(rc.RGB_ONLY, cam, background=(0.25, 0.5, 1))
    assert p.dc == (-1, -1, -1) and p.rgb == (44, 45, 46) and p.background == (0.25, 0.5, 1.0) and p.degree == 0
    lay = lib.render_layout(rd.plan_render(tc.splat_dtype(167), cam))
    assert (lay.degree, lay.rest_m, lay.width, lay.height, lay.near) == (2, 8, 37, 21, rc.NEAR) and lay.rest_offset[23] > 0 > lay.rest_offset[24]
    names = list(tc.splat_dtype(248).names)
    for gone in ("y", "scale_2", "rot_3", "opacity"):
        with pytest.raises(ValueError, match=f"no field '{gone}'"):
            rd.plan_render(np.dtype([(nm, "<f4") for nm in names if nm != gone]), cam)
    with pytest.raises(ValueError, match="no colour source"):
        rd.plan_render(np.dtype([(nm, "<f4") for nm in rc.GEOMETRY]), cam)
    with pytest.raises(ValueError, match="no colour source"):       # colours that are no bytes are no source
        rd.plan_render(np.dtype([(nm, "<f4") for nm in rc.GEOMETRY + ("red", "green", "blue")]), cam)
    with pytest.raises(ValueError, match="rows of 600 bytes"):
        rd.plan_render(np.dtype([(nm, "<f4") for nm in names] + [("pad", "V352")]), cam)
    with pytest.raises(ValueError, match="no whole bands"):
        rd.plan_render(np.dtype([(nm, "<f4") for nm in names if nm != "f_rest_44"]), cam)
    for w, h in ((0, 5), (5, 8193)):
        with pytest.raises(ValueError, match="image size"):
            rd.plan_render(dt, rd.Camera(w, h, cam.view, cam.eye, 1, 1, 0, 0, 1, 1, 1))
    with pytest.raises(ValueError, match="near"):
        rd.plan_render(dt, rc.axis_camera(8, 8, near=0.0))
    for nm in ("x", "rot_1", "opacity", "f_dc_2", "f_rest_20"):
        with pytest.raises(TypeError, match=f"field '{nm}' is <f8"):
            rd.plan_render(np.dtype([(f, "<f8" if f == nm else "<f4") for f in names]), cam)
    rd.plan_render(np.dtype([(f, "<f8" if f == "f_rest_20" else "<f4") for f in names]), cam, sh_degree=1)   # (a band that is not read)
    for kw in ({"sh_degree": 4}, {"sh_degree": 1.5}, {"background": (0, 0)}, {"background": (0, 0, 1.5)}, {"max_work_bytes": -1}):
        with pytest.raises(ValueError, match="render: "):
            rd.plan_render(dt, cam, **kw)
    assert issubclass(rd.RenderRefused, ValueError)


# ------------------------------------------------------------------------------------------------------------ the PNG

@pytest.mark.parametrize("size", ((1, 1), (37, 21), (256, 3)))
def test_write_png_reads_back(tmp_path, size):
    from PIL import Image
    w, h = size
    img = np.random.default_rng(w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    path = str(tmp_path / "p.png")
    rd.write_png(path, img)
    with Image.open(path) as im:
        assert im.mode == "RGB" and im.size == (w, h) and np.array_equal(np.asarray(im), img)
    for bad in (img[:, :, 0], img.astype(np.float32), img[:0]):
        with pytest.raises(ValueError, match="write_png"):
            rd.write_png(path, bad)


# ------------------------------------------------------------------------------------------------------------ the command line

def _scene(path):
    t = pn.build(10, pn.canonical_fields(3), np.random.default_rng(3))
    pn.write_ply(str(path), [("vertex", t)])
    return str(path)


def test_flags_parse(cli):
    a = cli.build_parser().parse_args(["-i", "a.ply", "-f", "spz", "--preview", "p.png", "--preview_size", "64", "48", "--preview_view", "10", "-5",
                                       "--preview_up=-z", "--preview_camera", "1", "2", "3", "4", "5", "6", "--preview_fov", "70"])
    assert (a.preview, a.preview_size, a.preview_view, a.preview_up, a.preview_camera, a.preview_fov) == \
        ("p.png", [64, 48], [10.0, -5.0], "-z", [1.0, 2.0, 3.0, 4.0, 5.0, 6.0], 70.0)
    a = cli.build_parser().parse_args(["-i", "a.ply", "-f", "spz"])
    assert all(getattr(a, nm) is None for nm in ("preview",) + cli.PREVIEW_OPTIONS) and cli.preview_kwargs(a) == {}
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["-i", "a.ply", "-f", "spz", "--preview", "p.png", "--preview_size", "64"])


@pytest.mark.parametrize("flags,line", (
    (["--preview_size", "64", "48"], "Error: --preview_size needs --preview FILE."),
    (["--preview_fov", "60"], "Error: --preview_fov needs --preview FILE."),
    (["--preview_up=+z"], "Error: --preview_up needs --preview FILE."),
    (["--preview", "p.png", "--preview_size", "0", "48"], "Error: --preview_size must be between 1 and 8192 per side. Got 0 48."),
    (["--preview", "p.png", "--preview_size", "64", "8193"], "Error: --preview_size must be between 1 and 8192 per side. Got 64 8193."),
    (["--preview", "p.png", "--preview_fov", "170"], "Error: --preview_fov must be between 0 and 170 (exclusive). Got 170.0."),
    (["--preview", "p.png", "--preview_fov", "nan"], "Error: --preview_fov must be between 0 and 170 (exclusive). Got nan."),
    (["--preview", "p.png", "--preview_up", "w"], "Error: --preview_up must be one of +x -x +y -y +z -z. Got w."),
    (["--preview", "p.png", "--preview_view", "0", "95"], "Error: --preview_view must be a finite azimuth and an elevation between -90 and 90. Got 0.0 95.0."),
    (["--preview", "p.png", "--preview_camera", "1", "2", "3", "1", "2", "3"],
     "Error: --preview_camera must be six finite numbers with the eye apart from the target. Got 1 2 3 1 2 3."),
    (["--preview", "p.png", "--preview_view", "0", "5", "--preview_camera", "1", "2", "3", "1", "2", "4"],
     "Error: --preview_view and --preview_camera cannot be combined (angles about the scene, or an explicit eye and target)."),
))
def test_each_validation_line_comes_before_a_read(cli, capsys, tmp_path, monkeypatch, flags, line):
    conv = importlib.import_module("3dgsconverter_amd.converter")
    monkeypatch.setattr(conv.SourceHandler, "read", lambda self, path, stage_ms=None: (_ for _ in ()).throw(AssertionError("read " + path)))
    assert cli.main(["-i", _scene(tmp_path / "a.ply"), "-f", "spz"] + flags) is None
    assert capsys.readouterr().out.strip().split("\n") == [line]


def test_preview_is_an_action_and_reaches_run(cli, capsys, tmp_path, monkeypatch):
    src = _scene(tmp_path / "a.ply")
    seen = {}
    monkeypatch.setattr(cli, "report_info", lambda *a, **k: None)
    monkeypatch.setattr(cli.Converter, "run", lambda self, **kw: seen.update(kw))
    cli.main(["-i", src, "-f", "3dgs", "--preview", "p.png"])
    assert "Operation aborted" not in capsys.readouterr().out and seen["preview"] == "p.png"
    assert not any(k.startswith("preview_") for k in seen)         # flags that were not given stay the renderer's defaults
    seen.clear()
    cli.main(["-i", src, "-f", "3dgs", "--preview", "p.png", "--preview_size", "64", "48", "--preview_up=+z", "--force"])
    assert seen["preview_size"] == [64, 48] and seen["preview_up"] == "+z"
    seen.clear()
    cli.main(["-i", src, "-f", "3dgs"])
    assert "Operation aborted" in capsys.readouterr().out and not seen
    cli.main(["-i", src, "-f", "spz"])
    assert seen and not any(k.startswith("preview") for k in seen)


# ------------------------------------------------------------------------------------------------------------ the converter

def test_run_renders_the_written_table_after_the_writer(monkeypatch, tmp_path, capsys):
    from PIL import Image
    conv = importlib.import_module("3dgsconverter_amd.converter")
    table = rc.scene(tc.splat_dtype(248), 64, 48, 40)
    events = []
    picture = np.random.default_rng(1).integers(0, 256, (40, 48, 3), dtype=np.uint8)

    def read(self, path, stage_ms=None):
        self.profile = lib.host_table_profile(table)
        return table.copy()

    def write(self, data, path, stage_ms=None, **kw):
        assert not any(k.startswith("preview") for k in kw)
        events.append(("write", data))

    def render_table(data, plan, stage_ms=None, device=0, info=None):
        events.append(("render", data, plan))
        info.update({"visible": 41, "instances": 99, "rows": len(data)})
        return picture

    monkeypatch.setattr(conv.SourceHandler, "read", read)
    monkeypatch.setattr(conv.SourceHandler, "write", write)
    monkeypatch.setattr(lib, "render_table", render_table)
    src, png = _scene(tmp_path / "a.ply"), str(tmp_path / "p.png")
    c = conv.Converter(src, str(tmp_path / "o.spz"), "spz", resident=False)
    c.run(preview=png, preview_size=(48, 40), preview_view=(10, 5), preview_up="+z", preview_fov=70, sh_level=1)
    assert [e[0] for e in events] == ["write", "render"] and events[1][1] is events[0][1] and events[1][1] is c.data
    plan = events[1][2]
    prof = lib.host_table_profile(c.data)
    want = rd.plan_camera(prof["lo"], prof["hi"], (48, 40), (10, 5), "+z", 70)
    assert np.array_equal(plan.camera.view, want.view) and (plan.camera.width, plan.camera.height, plan.camera.near) == (48, 40, want.near)
    assert plan.dtype == c.data.dtype and plan.degree == 3 and c.last_preview["plan"] is plan
    with Image.open(png) as im:
        assert np.array_equal(np.asarray(im), picture)
    lines = capsys.readouterr().out.split("\n")
    assert f"Preview: 48 x 40, 41 of 64 splats visible, saved to {png}" in lines and "preview_png" in c.stage_ms
    assert lines.index(f"Preview: 48 x 40, 41 of 64 splats visible, saved to {png}") < lines.index(f"Conversion completed: Saved to {tmp_path / 'o.spz'}")

    events.clear()
    conv.Converter(src, str(tmp_path / "o2.spz"), "spz", resident=False).run(sh_level=1)
    assert [e[0] for e in events] == ["write"]                      # no keyword, no renderer

    def refuse(data, plan, stage_ms=None, device=0, info=None):
        raise rd.RenderRefused("render: an image of 48 x 40 needs 7 (tile, splat) instances")

    monkeypatch.setattr(lib, "render_table", refuse)
    png2 = str(tmp_path / "q.png")
    conv.Converter(src, str(tmp_path / "o3.spz"), "spz", resident=False).run(preview=png2, preview_size=(48, 40))
    out = capsys.readouterr().out.split("\n")
    assert "Warning: preview not written: render: an image of 48 x 40 needs 7 (tile, splat) instances" in out
    assert f"Conversion completed: Saved to {tmp_path / 'o3.spz'}" in out and not os.path.exists(png2)

    def broken(data, plan, stage_ms=None, device=0, info=None):
        raise RuntimeError("device lost")

    monkeypatch.setattr(lib, "render_table", broken)
    with pytest.raises(RuntimeError, match="device lost"):
        conv.Converter(src, str(tmp_path / "o4.spz"), "spz", resident=False).run(preview=png2)
