"""-m "not gpu": the view scores' host side, no device touched -- the ring of views (views.plan_views), the ranking key
(tests/view_scores_numpy.total_keys against csrc/view_key.h's function through gsx_view_keys_host), the selection through
gsx_limit_select_host, every refusal of prune_by_views / limit_splats(rank_by=...) with the device made unreachable, and the
command line's flags."""
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
import view_scores_numpy as vn  # noqa: E402

lib = importlib.import_module("3dgsconverter_amd._lib")
rd = importlib.import_module("3dgsconverter_amd.render")
vw = importlib.import_module("3dgsconverter_amd.views")
dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")

LO, HI = (-1.0, -2.0, 0.5), (3.0, 1.0, 2.5)


@pytest.fixture(scope="module")
def cli():
    return importlib.import_module("3dgsconverter_amd.cli")


# ------------------------------------------------------------------------------------------------------------ the ring of views

def _angles(cam, up_axis=1, up_sign=-1.0):
    """azimuth and elevation (degrees) of the eye about the box centre, in plan_camera's frame about `up`"""
    centre = 0.5 * (np.array(LO) + np.array(HI))
    d = cam.eye - centre
    dist = math.sqrt(float(d @ d))
    d = d / dist
    e1, e2, upv = np.zeros(3), np.zeros(3), np.zeros(3)
    e1[(up_axis + 1) % 3], e2[(up_axis + 2) % 3], upv[up_axis] = 1.0, up_sign, up_sign
    return math.degrees(math.atan2(float(d @ e2), float(d @ e1))) % 360.0, math.degrees(math.asin(float(d @ upv))), dist


@pytest.mark.parametrize("V,elevation", ((32, (-10, 70)), (1, (-10, 70)), (7, (-90, 90)), (1024, (0, 45))))
def test_ring_of_views(V, elevation):
    cams = vw.plan_views(LO, HI, views=V, elevation=elevation)
    assert len(cams) == V and all(isinstance(c, rd.Camera) and (c.width, c.height) == (512, 512) for c in cams)
    want_dist = _angles(rd.plan_camera(LO, HI, (512, 512)))[2]
    lo, hi = (math.sin(math.radians(v)) for v in elevation)
    last = -91.0
    for k, cam in enumerate(cams):
        az, el, dist = _angles(cam)
        want_az = (k * 137.50776405003785) % 360.0
        want_el = math.degrees(math.asin(lo + (k + 0.5) / V * (hi - lo)))
        assert abs(dist - want_dist) <= 1e-12 * want_dist and cam.near == rd.plan_camera(LO, HI, (512, 512)).near
        assert abs((az - want_az + 180.0) % 360.0 - 180.0) <= 1e-9 and abs(el - want_el) <= 1e-9
        assert elevation[0] <= el <= elevation[1] and el > last
        last = el
        ref = rd.plan_camera(LO, HI, (512, 512), view=(want_az, want_el))
        assert np.array_equal(ref.view, cam.view) and np.array_equal(ref.eye, cam.eye)


def test_explicit_cameras_replace_the_ring():
    given = [(5, 5, 5, 0, 0, 0), (0, 0, -4, 0, 0, 1), (1, 2, 3, 3, 2, 1)]
    cams = vw.plan_views(LO, HI, views=32, size=(64, 48), cameras=given, fov=60)
    assert len(cams) == 3
    for c, g in zip(cams, given):
        ref = rd.plan_camera(LO, HI, (64, 48), fov=60, camera=g)
        assert np.array_equal(c.eye, np.array(g[:3], float)) and np.array_equal(c.view, ref.view) and c.near == ref.near
        assert (c.width, c.height) == (64, 48)
    for bad in ([], [(1, 2, 3)], [(1, 2, 3, 1, 2, 3)], 5):
        with pytest.raises(ValueError):
            vw.plan_views(LO, HI, cameras=bad)


def test_scoring_plan_is_geometry_only():
    geometry = np.dtype([(nm, "<f4") for nm in rc.GEOMETRY])
    cam = rc.axis_camera(16, 16)
    with pytest.raises(ValueError, match="colour source"):
        rd.plan_render(geometry, cam)
    plan = vw.plan_scores(geometry, cam, max_work_bytes=77)
    assert plan.dc == (-1, -1, -1) and plan.rgb == (-1, -1, -1) and plan.degree == 0 and plan.max_work_bytes == 77
    full = vw.plan_scores(tc.splat_dtype(248), cam)
    assert full.dc == (-1, -1, -1) and full.rest == () and full.xyz == rd.plan_render(tc.splat_dtype(248), cam).xyz
    lay = lib.render_layout(plan)
    assert list(lay.dc_offset) == [-1] * 3 and list(lay.rgb_offset) == [-1] * 3


# ------------------------------------------------------------------------------------------------------------ the ranking key

EDGES = sorted(set([0, 1, 2, 3] + [2 ** k for k in range(2, 63)] + [2 ** 24 - 2, 2 ** 24 - 1, 2 ** 24 + 1, 2 ** 24 + 2, 2 ** 32, 2 ** 53 + 1, 2 ** 62 - 1]))


def test_total_keys_are_monotone_and_the_device_functions():
    keys = vn.total_keys(np.array(EDGES, np.uint64))
    assert keys[0] == 0xffffffff and keys.dtype == np.uint32
    powers = [k for k, t in zip(keys.tolist(), EDGES) if t and t & (t - 1) == 0]
    assert all(a > b for a, b in zip(powers, powers[1:]))                      # strictly falling across the powers of two
    assert all(a >= b for a, b in zip(keys.tolist(), keys.tolist()[1:]))
    k = dict(zip(EDGES, keys.tolist()))
    # strict wherever float32 tells the totals apart; 2^24 + 1 and 2^53 + 1 round toward zero onto the power of two below them
    assert k[2 ** 24 - 2] > k[2 ** 24 - 1] > k[2 ** 24] == k[2 ** 24 + 1] > k[2 ** 24 + 2] > k[2 ** 32] and k[2 ** 53 + 1] == k[2 ** 53]
    assert k[2 ** 62 - 1] < k[2 ** 61] and k[2 ** 62 - 1] > k[2 ** 62]
    # fbits is the float32 toward zero: the nearest float32 not above the integer
    for t in EDGES[1:]:
        f = float(np.array([0xffffffff - k[t]], np.uint32).view(np.float32)[0])
        assert f <= t < float(np.nextafter(np.float32(f), np.float32(np.inf)))
    rng = np.random.default_rng(1)
    many = np.concatenate([np.array(EDGES, np.uint64), rng.integers(0, 2 ** 62, 4000, dtype=np.uint64),
                           rng.integers(0, 2 ** 26, 4000, dtype=np.uint64)])
    assert np.array_equal(lib.view_keys_host(many), vn.total_keys(many))


def test_selection_through_the_budget_select():
    rng = np.random.default_rng(2)
    total = rng.integers(0, 2 ** 30, 3000, dtype=np.uint64)
    total[rng.integers(0, 3000, 900)] = 0                                       # never seen: ties at 0xffffffff
    total[100:140] = total[100]                                                # ties among the seen
    keys = lib.view_keys_host(total)
    for rows in (np.arange(3000), np.sort(rng.choice(3000, 1200, replace=False))):
        for N in (1, 37, 1100, len(rows) - 1):
            mask, info = lib.limit_select_host(keys, N, None if len(rows) == 3000 else rows.astype(np.uint32))
            assert np.array_equal(rows[mask], vn.keep_budget(total, rows, N)) and info["kept"] == N
    peak = rng.uniform(0, 0.99, 50).astype(np.float32)
    peak[7] = np.float32(0.01)
    keep = vn.keep_peak(peak, 0.01)
    assert keep[7] and np.array_equal(keep, peak.astype(np.float64) >= float(np.float32(0.01)))


def test_accumulate_is_max_and_sum():
    a = (np.array([0.5, 0, 0.25], np.float32), np.array([2 ** 40, 0, 5], np.uint64))
    b = (np.array([0.125, 0, 0.75], np.float32), np.array([2 ** 40, 0, 7], np.uint64))
    for views in ([a, b], [b, a]):
        peak, total = vn.accumulate(views)
        assert peak.tolist() == [0.5, 0, 0.75] and total.tolist() == [2 ** 41, 0, 12] and total.dtype == np.uint64


def test_twin_follows_the_image():
    """the weights the twin scores are the image's: colour 1 on a black background gives sum of the weights per pixel"""
    t = rc.scene(tc.splat_dtype(68), 120, 17, 33)
    plan = rc.plan_for(t, 17, 33, background=(0, 0, 0))
    rec = rn.records(t, plan)
    peak, total = vn.scores(rec, plan)
    assert (peak[~rec["visible"].astype(bool)] == 0).all() and (total[2:20] == 0).all() and peak[0] > 0
    assert ((peak > 0) == (total > 0)).all() and peak.max() <= np.float32(0.99)
    white = rec.copy()
    for nm in ("r", "g", "bl"):
        white[nm] = np.float32(1.0)
    details = {}
    img = rn.image(white, plan, details)
    assert abs(float(total.sum()) / 2 ** 24 - img[:, :, 0].astype(np.float64).sum() / 255.0) < 0.01 * img.shape[0] * img.shape[1]


# ------------------------------------------------------------------------------------------------------------ the refusals

@pytest.fixture()
def no_device(monkeypatch):
    def fail(*a, **k):
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(lib, "require_hip", fail)
    monkeypatch.setattr(lib, "load", fail)


def _table(n=20, dtype=None):
    return rc.scene(tc.splat_dtype(68), 64, 16, 16)[:n] if dtype is None else np.zeros(n, dtype)


@pytest.mark.parametrize("lazy", (False, True))
@pytest.mark.parametrize("kw,exc,match", (
    (dict(min_contribution=0), ValueError, "min_contribution"),
    (dict(min_contribution=1), ValueError, "min_contribution"),
    (dict(min_contribution=float("nan")), ValueError, "min_contribution"),
    (dict(min_contribution="x"), ValueError, "min_contribution"),
    (dict(views=0), ValueError, "1 ... 1024"),
    (dict(views=1025), ValueError, "1 ... 1024"),
    (dict(views=2.5), ValueError, "1 ... 1024"),
    (dict(views=True), ValueError, "1 ... 1024"),
    (dict(elevation=(-91, 0)), ValueError, "elevations"),
    (dict(elevation=(30, 20)), ValueError, "elevations"),
    (dict(elevation=(0, 91)), ValueError, "elevations"),
    (dict(size=(0, 5)), ValueError, "image size"),
    (dict(size=(8193, 5)), ValueError, "image size"),
    (dict(fov=170), ValueError, "field of view"),
    (dict(up="w"), ValueError, "up must be"),
    (dict(cameras=[(1, 2, 3, 1, 2, 3)]), ValueError, "eye and target"),
    (dict(cameras=[]), ValueError, "cameras"),
    (dict(max_work_bytes=-1), ValueError, "max_work_bytes"),
))
def test_refusals_come_before_any_device_work(no_device, lazy, kw, exc, match):
    t = _table()
    for call in ("prune",) if "min_contribution" in kw else ("prune", "limit"):        # (the budget has no threshold)
        p = dp.DataProcessor(t.copy(), lazy=lazy)
        args = dict(kw)
        with pytest.raises(exc, match=match):
            if call == "prune":
                p.prune_by_views(args.pop("min_contribution", 0.01), **args)
            else:
                p.limit_splats(5, rank_by="views", **args)
        assert p._data.tobytes() == t.tobytes() and p._chain is None


def test_dtype_and_budget_refusals(no_device):
    t = _table()
    f8 = np.dtype([(nm, "<f8" if nm == "scale_1" else "<f4") for nm in rc.GEOMETRY])
    big = np.dtype([(nm, ">f4" if nm == "x" else "<f4") for nm in rc.GEOMETRY])
    for dtype, field in ((f8, "scale_1"), (big, "'x'")):
        for lazy in (False, True):
            p = dp.DataProcessor(_table(5, dtype), lazy=lazy)
            with pytest.raises(TypeError, match=field):
                p.prune_by_views(0.01)
            with pytest.raises(TypeError, match=field):
                p.limit_splats(3, rank_by="views")
    p = dp.DataProcessor(t.copy())
    with pytest.raises(ValueError, match="rank_by"):
        p.limit_splats(5, rank_by="depth")
    with pytest.raises(ValueError, match="rank_by='views'"):
        p.limit_splats(5, views=4)
    with pytest.raises(ValueError):
        p.limit_splats(0, rank_by="views")
    with pytest.raises(ValueError):
        p.prune_by_views(0.01, max_count=0)
    with pytest.raises(TypeError, match="unknown option"):
        p.limit_splats(5, rank_by="views", sh_degree=1)


def test_a_budget_the_table_meets_scores_nothing(no_device, capsys):
    t = _table()
    for lazy in (False, True):
        p = dp.DataProcessor(t.copy(), lazy=lazy)
        p.limit_splats(len(t), rank_by="views", views=3, size=(8, 8))
        assert "Splat Limit (max 20, by 3 views, 8 x 8): 20 splats, nothing to remove." in capsys.readouterr().out
        assert p._data.tobytes() == t.tobytes() and p._chain is None


def test_table_without_geometry_is_left_alone(no_device, capsys):
    t = np.zeros(8, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("opacity", "<f4")]))
    for lazy in (False, True):
        p = dp.DataProcessor(t.copy(), lazy=lazy)
        out = p.prune_by_views(0.01)
        assert (out is None) == lazy and p._data.tobytes() == t.tobytes()
        assert "Warning: View scores need x y z, scale_0..2, rot_0..3 and opacity. View Prune skipped." in capsys.readouterr().out
        p.limit_splats(3, rank_by="views")
        assert "Splat Limit skipped." in capsys.readouterr().out and len(p._data) == 8
        with pytest.raises(ValueError, match="1 ... 1024"):
            p.prune_by_views(0.01, views=0)


# ------------------------------------------------------------------------------------------------------------ the command line

def _scene(path):
    t = pn.build(10, pn.canonical_fields(3), np.random.default_rng(3))
    pn.write_ply(str(path), [("vertex", t)])
    return str(path)


def test_flags_parse(cli):
    a = cli.build_parser().parse_args(["-i", "a.ply", "-f", "spz", "--min_contribution", "0.02", "--rank_by", "views", "--max_splats", "9", "--views",
                                       "8", "--views_size", "64", "48", "--views_elevation", "-5", "40", "--views_up=+z"])
    assert cli.view_kwargs(a) == {"min_contribution": 0.02, "rank_by": "views", "views": 8, "views_size": [64, 48],
                                  "views_elevation": [-5.0, 40.0], "views_up": "+z"}
    a = cli.build_parser().parse_args(["-i", "a.ply", "-f", "spz", "--min_contribution", "0.02", "--view_camera", "1", "2", "3", "4", "5", "6",
                                       "--view_camera", "0", "0", "0", "0", "0", "1"])
    assert cli.view_kwargs(a) == {"min_contribution": 0.02, "view_cameras": [(1.0, 2.0, 3.0, 4.0, 5.0, 6.0), (0.0, 0.0, 0.0, 0.0, 0.0, 1.0)]}
    assert cli.view_kwargs(cli.build_parser().parse_args(["-i", "a.ply", "-f", "spz"])) == {}
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["-i", "a.ply", "-f", "spz", "--rank_by", "depth"])
    text = cli.build_parser().format_help()
    assert "--min_contribution" in text and "non-finite geometry" in " ".join(text.split())


@pytest.mark.parametrize("flags,line", (
    (["--views", "8"], "Error: --views needs --min_contribution W or --rank_by views."),
    (["--views_size", "64", "48"], "Error: --views_size needs --min_contribution W or --rank_by views."),
    (["--views_elevation", "0", "10"], "Error: --views_elevation needs --min_contribution W or --rank_by views."),
    (["--views_up=+z"], "Error: --views_up needs --min_contribution W or --rank_by views."),
    (["--view_camera", "1", "2", "3", "4", "5", "6"], "Error: --view_camera needs --min_contribution W or --rank_by views."),
    (["--max_splats", "5", "--rank_by", "size", "--views", "8"], "Error: --views needs --min_contribution W or --rank_by views."),
    (["--rank_by", "views"], "Error: --rank_by views ranks the splats for --max_splats N; give --max_splats too."),
    (["--min_contribution", "0"], "Error: --min_contribution must be between 0 and 1 (exclusive). Got 0.0."),
    (["--min_contribution", "1"], "Error: --min_contribution must be between 0 and 1 (exclusive). Got 1.0."),
    (["--min_contribution", "nan"], "Error: --min_contribution must be between 0 and 1 (exclusive). Got nan."),
    (["--min_contribution", "0.1", "--views", "0"], "Error: --views must be between 1 and 1024. Got 0."),
    (["--min_contribution", "0.1", "--views", "1025"], "Error: --views must be between 1 and 1024. Got 1025."),
    (["--min_contribution", "0.1", "--views_size", "0", "4"], "Error: --views_size must be between 1 and 8192 per side. Got 0 4."),
    (["--min_contribution", "0.1", "--views_elevation", "20", "10"], "Error: --views_elevation must be two angles with -90 <= LO <= HI <= 90. Got 20.0 10.0."),
    (["--min_contribution", "0.1", "--views_up", "w"], "Error: --views_up must be one of +x -x +y -y +z -z. Got w."),
    (["--min_contribution", "0.1", "--view_camera", "1", "2", "3", "1", "2", "3"],
     "Error: --view_camera must be six finite numbers with the eye apart from the target. Got 1 2 3 1 2 3."),
    (["--min_contribution", "0.1", "--views", "4", "--view_camera", "1", "2", "3", "1", "2", "4"],
     "Error: --view_camera replaces the ring; it cannot be combined with --views or --views_elevation."),
    (["--min_contribution", "0.1", "--info"], "Error: --min_contribution and --rank_by views act on a conversion; they cannot be combined with --info."),
))
def test_each_validation_line_comes_before_a_read(cli, capsys, tmp_path, monkeypatch, flags, line):
    conv = importlib.import_module("3dgsconverter_amd.converter")
    monkeypatch.setattr(conv.SourceHandler, "read", lambda self, path, stage_ms=None: (_ for _ in ()).throw(AssertionError("read " + path)))
    assert cli.main(["-i", _scene(tmp_path / "a.ply"), "-f", "spz"] + flags) is None
    assert capsys.readouterr().out.strip().split("\n") == [line]


def test_view_options_are_actions_and_reach_run(cli, capsys, tmp_path, monkeypatch):
    src = _scene(tmp_path / "a.ply")
    seen = {}
    monkeypatch.setattr(cli, "report_info", lambda *a, **k: None)
    monkeypatch.setattr(cli.Converter, "run", lambda self, **kw: seen.update(kw))
    cli.main(["-i", src, "-f", "3dgs"])
    assert "Operation aborted" in capsys.readouterr().out and not seen
    cli.main(["-i", src, "-f", "3dgs", "--min_contribution", "0.05"])
    assert "Operation aborted" not in capsys.readouterr().out and seen["min_contribution"] == 0.05
    assert not any(k.startswith("view") or k == "rank_by" for k in seen)       # flags that were not given stay the defaults
    seen.clear()
    cli.main(["-i", src, "-f", "3dgs", "--max_splats", "4", "--rank_by", "views", "--views", "3", "--force"])
    assert seen["rank_by"] == "views" and seen["views"] == 3 and seen["max_splats"] == 4 and "min_contribution" not in seen


def test_run_orders_the_steps_and_shares_one_pass(monkeypatch, tmp_path, capsys):
    conv = importlib.import_module("3dgsconverter_amd.converter")
    t = pn.build(10, [f for f in pn.canonical_fields(0) if f[0] not in ("nx", "ny", "nz")], np.random.default_rng(3))
    calls = []

    def read(self, path, stage_ms=None):
        self.profile = lib.host_table_profile(t)
        return t

    monkeypatch.setattr(conv.SourceHandler, "read", read)
    monkeypatch.setattr(conv.SourceHandler, "write", lambda self, data, path, stage_ms=None, **kw: calls.append(("write", sorted(kw))))
    for name in ("decimate", "prune_by_views", "limit_splats"):
        monkeypatch.setattr(dp.DataProcessor, name, lambda self, *a, _n=name, **k: calls.append((_n, a, k)))

    def run(**kw):
        calls.clear()
        conv.Converter(str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "3dgs", resident=False).run(**kw)
        return [c for c in calls if c[0] != "write"]

    monkeypatch.setattr(conv.Converter, "_detect_format", lambda self, path: "3dgs")
    assert run(decimate_voxel_size=0.5, min_contribution=0.02, max_splats=4, rank_by="views", views=3, views_size=(8, 8)) == [
        ("decimate", (0.5,), {}), ("prune_by_views", (0.02,), {"max_count": 4, "views": 3, "size": (8, 8)})]
    assert run(min_contribution=0.02, max_splats=4, view_cameras=[(0, 0, 0, 0, 0, 1)]) == [
        ("prune_by_views", (0.02,), {"max_count": None, "cameras": [(0, 0, 0, 0, 0, 1)]}), ("limit_splats", (4,), {})]
    assert run(max_splats=4, rank_by="views", views_elevation=(0, 10), views_up="+z") == [
        ("limit_splats", (4,), {"rank_by": "views", "elevation": (0, 10), "up": "+z"})]
    assert run(max_splats=4) == [("limit_splats", (4,), {})] and run(max_splats=4, rank_by="size") == [("limit_splats", (4,), {})]
    assert not any("view" in k or k in ("rank_by", "min_contribution") for c in calls if c[0] == "write" for k in c[1])
    for bad in (dict(rank_by="views"), dict(views=3), dict(max_splats=3, rank_by="depth")):
        with pytest.raises(ValueError):
            run(**bad)
