"""-m "not gpu": the fidelity sums' definition (tests/fidelity_numpy.py) against exact rational arithmetic, the host twin of the
compare kernel against the definition word for word, and everything of --fidelity that needs no device: the options' refusals,
the CLI's error lines, the pooled figures and the report's forms."""
import argparse
import contextlib
import importlib
import io
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fidelity_cases as fc  # noqa: E402
import fidelity_numpy as fn  # noqa: E402

fid = importlib.import_module("3dgsconverter_amd.fidelity")


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgsconverter_amd._lib")


@pytest.fixture(scope="module")
def expected():
    """the definition's nine integers of every case, computed once"""
    return {c: fn.compare(*fc.pair(*c)) for c in fc.CASES}


def test_tile_constant_is_the_library_s(lib):
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsx_hip.h")).read()
    assert "GSX_FIDELITY_TILE = %d" % fid.TILE in text and lib.FIDELITY_TILE == fid.TILE == fc.T


@pytest.mark.parametrize("case", [c for c in fc.CASES if c[1:] in ((8, 8), (9, 8), (71, 40), (fc.T + 7, fc.T + 7))], ids=lambda c: "%s-%dx%d" % c)
def test_definition_against_exact_rationals(case):
    """per window |q - floor(exact * 2^32)| <= 1: two divisions and a product, each within 2^-53 relative, of a value of
    magnitude at most 1, leave the float64 path within 2^-20 units of the exact rational before the floor"""
    a, b = fc.pair(*case)
    q = fn.window_q(a, b).ravel().tolist()
    exact = fn.window_q_exact(a, b)
    assert len(q) == len(exact) == 3 * (a.shape[0] - 7) * (a.shape[1] - 7)
    assert max(abs(x - y) for x, y in zip(q, exact)) <= 1
    got = fn.compare(a, b)
    d = a.astype(object) - b.astype(object)                 # Python ints: no width to overflow
    assert got["sse"] == tuple(int((d[:, :, c] ** 2).sum()) for c in range(3))
    assert got["windows"] == (a.shape[0] - 7) * (a.shape[1] - 7) and abs(sum(got["ssim"]) - sum(exact)) <= len(exact)


def test_definition_at_its_landmarks():
    h, w = 19, 23
    a, same = fc.pair("identical", h, w)
    r = fn.compare(a, same)
    assert r["sse"] == (0, 0, 0) and r["ssim"] == (r["windows"] * fn.ONE,) * 3 and r["windows"] == 12 * 16
    r = fn.compare(*fc.pair("black_white", h, w))
    assert r["sse"] == (h * w * 65025,) * 3
    # Sa = 0, Sb = 16320: r1 = c1 / (16320^2 + c1), r2 = 1 (no variance on either side)
    q = math.floor(np.float64(fn.C1) / np.float64(16320 ** 2 + fn.C1) * 1.0 * fn.ONE)
    assert r["ssim"] == (r["windows"] * q,) * 3
    a, b = fc.pair("complement", h, w)
    assert fn.window_q(a, b).min() < 0                       # negative covariance: floor on negative values
    assert fn.compare(a[:7], b[:7])["windows"] == 0 and fn.compare(a[:7], b[:7])["ssim"] == (0, 0, 0)
    assert fn.psnr(0, 4, 4) == math.inf and fn.ssim(0, 0) is None and fn.ssim(3 * fn.ONE, 1) == 1.0


@pytest.mark.parametrize("case", fc.CASES, ids=fc.IDS)
def test_host_twin_is_the_definition(lib, expected, case):
    a, b = fc.pair(*case)
    assert lib.image_compare_host(a, b) == expected[case]
    if case[0] == "identical":
        want = expected[case]
        assert want["sse"] == (0, 0, 0) and want["ssim"] == (want["windows"] * fn.ONE,) * 3


def test_host_twin_refusals(lib):
    a = np.zeros((8, 8, 3), np.uint8)
    empty = np.zeros((0, 8, 3), np.uint8)
    for x, y in ((a[:, :, :2], a[:, :, :2]), (a.astype(np.int8), a), (a, np.zeros((8, 9, 3), np.uint8)), (empty, empty), (a[0], a[0])):
        with pytest.raises(ValueError):
            lib.image_compare_host(x, y)
    words = (lib.C.c_int64 * 9)()
    assert lib.load().gsx_image_compare_host(a.ctypes.data, a.ctypes.data, 0, 8, words) != 0
    assert lib.load().gsx_image_compare_host(a.ctypes.data, a.ctypes.data, 8, 8193, words) != 0
    assert lib.load().gsx_image_compare_host(None, a.ctypes.data, 8, 8, words) != 0


REFUSALS = [
    (dict(mode="file"), "mode"),
    (dict(mode=None), "mode"),
    (dict(mode="source", merge=["b.ply"]), "merge"),
    (dict(views=0), "views"),
    (dict(views=1025), "views"),
    (dict(views=2.5), "views"),
    (dict(size=(0, 8)), "size"),
    (dict(size=(8, 8193)), "size"),
    (dict(size=(8,)), "size"),
    (dict(up="w"), "up"),
    (dict(fov=170), "field of view"),
    (dict(elevation=(50, 10)), "elevations"),
    (dict(cameras=[]), "cameras"),
    (dict(cameras=[(0, 0, 0, 0, 0, 0)]), "eye and target"),
    (dict(cameras=[(0, 0, 0, 1, 1)]), "six finite"),
    (dict(cameras=[(0, 0, 0, 0, 0, 1)], views=4), "not both"),
]


@pytest.mark.parametrize("kw,needle", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_check_options_refuses(kw, needle):
    with pytest.raises(ValueError, match=needle):
        fid.check_options(**dict({"mode": "written"}, **kw))


def test_check_options_normalises():
    o = fid.check_options()
    assert (o["mode"], o["views"], o["size"], o["up"], o["fov"], o["cameras"]) == ("written", 8, (512, 512), "-y", 50, None)
    o = fid.check_options("source", views=3.0, size=[17, 33], up="z")
    assert (o["mode"], o["views"], o["size"], o["up"]) == ("source", 3, (17, 33), "z")
    o = fid.check_options("written", cameras=[[0, 0, 0, 0, 0, 1], (1, 0, 0, 0, 0, 0)], merge=["b.ply"])
    assert o["views"] == 2 and o["cameras"] == [(0, 0, 0, 0, 0, 1), (1, 0, 0, 0, 0, 0)]


def _view(sse, windows, fixed, w=16, h=12):
    return fid.view_figures({"sse": sse, "windows": windows, "ssim": fixed}, w, h)


def test_pooled_figures_use_summed_integers():
    one = fn.ONE
    views = [_view((10, 20, 30), 45, (40 * one, 41 * one, 42 * one)), _view((1000, 0, 0), 45, (30 * one, 45 * one, 45 * one)),
             _view((0, 0, 60), 45, (45 * one, 45 * one, 33 * one))]
    s = fid.summarise(views)
    assert s["sse"] == (1010, 20, 90) and s["windows"] == 135 and s["ssim_fixed"] == (115 * one, 131 * one, 120 * one)
    assert s["psnr"] == fn.psnr(1120, 3 * 12, 16) == 10.0 * math.log10(255.0 ** 2 * (3 * 3 * 12 * 16) / 1120)
    assert s["ssim"] == 366 / 405 == fn.ssim(366 * one, 135)
    assert s["psnr"] != pytest.approx(sum(v["psnr"] for v in views) / 3, abs=0.5)      # no mean of decibels
    assert s["worst_view"] == 1 and s["worst_psnr"] == views[1]["psnr"] == fn.psnr(1000, 12, 16)
    assert s["worst_ssim_view"] == 1 and s["worst_ssim"] == 120 / 135 and s["size"] == (16, 12)
    assert s["report"] == "3 views of 16 x 12: PSNR %.2f dB (worst %.2f, view 1), SSIM %.4f (worst %.4f, view 1)" % (
        s["psnr"], views[1]["psnr"], 366 / 405, 120 / 135)
    assert fid.report_line(s, "written table vs out.spz").startswith("Fidelity (written table vs out.spz): 3 views of 16 x 12: PSNR ")
    # ties go to the lowest index
    tie = fid.summarise([_view((5, 5, 5), 45, (one, one, one)), _view((5, 5, 5), 45, (one, one, one))])
    assert tie["worst_view"] == 0 and tie["worst_ssim_view"] == 0


def test_report_forms_for_identical_images_and_no_windows():
    one = fn.ONE
    s = fid.summarise([_view((0, 0, 0), 45, (45 * one,) * 3)])
    assert s["psnr"] == math.inf and s["ssim"] == 1.0
    assert s["report"] == "1 view of 16 x 12: PSNR inf (identical images), SSIM 1.0000 (worst 1.0000, view 0)"
    s = fid.summarise([_view((7, 0, 0), 0, (0, 0, 0), w=40, h=5), _view((0, 0, 0), 0, (0, 0, 0), w=40, h=5)])
    assert s["ssim"] is None and s["worst_ssim_view"] is None and s["worst_view"] == 0
    assert s["report"].endswith(", SSIM n/a") and "PSNR %.2f dB (worst %.2f, view 0)" % (s["psnr"], s["views"][0]["psnr"]) in s["report"]
    s = fid.summarise([_view((0, 0, 0), 0, (0, 0, 0), w=7, h=7)])
    assert s["report"] == "1 view of 7 x 7: PSNR inf (identical images), SSIM n/a"
    with pytest.raises(ValueError):
        fid.summarise([])


def test_side_by_side():
    a, b = fc.pair("random", 5, 9)
    img = fid.side_by_side(a, b)
    assert img.shape == (5, 27, 3) and img.dtype == np.uint8
    assert np.array_equal(img[:, :9], a) and np.array_equal(img[:, 9:18], b)
    assert np.array_equal(img[:, 18:], np.minimum(255, 4 * np.abs(a.astype(int) - b.astype(int))))


# ------------------------------------------------------------------------------------------------------------ the CLI

CLI_ERRORS = [
    (["--fidelity_views", "4"], "Error: --fidelity_views needs --fidelity."),
    (["--fidelity_image", "x.png"], "Error: --fidelity_image needs --fidelity."),
    (["--fidelity_camera", "0", "0", "0", "0", "0", "1"], "Error: --fidelity_camera needs --fidelity."),
    (["--fidelity", "--info"], "Error: --fidelity measures a conversion's result; it cannot be combined with --info."),
    (["--fidelity", "source", "--merge", "b.ply"],
     "Error: --fidelity source compares against the one input file; it cannot be combined with --merge (use --fidelity written)."),
    (["--fidelity", "--fidelity_views", "0"], "Error: --fidelity_views must be between 1 and 1024. Got 0."),
    (["--fidelity", "--fidelity_views", "1025"], "Error: --fidelity_views must be between 1 and 1024. Got 1025."),
    (["--fidelity", "--fidelity_size", "0", "9000"], "Error: --fidelity_size must be between 1 and 8192 per side. Got 0 9000."),
    (["--fidelity", "--fidelity_up=w"], "Error: --fidelity_up must be one of +x -x +y -y +z -z. Got w."),
    (["--fidelity", "--fidelity_camera", "1", "2", "3", "1", "2", "3"],
     "Error: --fidelity_camera must be six finite numbers with the eye apart from the target. Got 1 2 3 1 2 3."),
    (["--fidelity", "--fidelity_camera", "0", "0", "0", "0", "0", "1", "--fidelity_views", "3"],
     "Error: --fidelity_camera replaces the ring; it cannot be combined with --fidelity_views."),
]


@pytest.mark.parametrize("argv,line", CLI_ERRORS, ids=[str(i) for i in range(len(CLI_ERRORS))])
def test_cli_error_lines(argv, line):
    cli = importlib.import_module("3dgsconverter_amd.cli")
    args = cli.build_parser().parse_args(["-i", "a.ply", "-f", "spz"] + argv)
    assert cli.check_fidelity_args(args) == line
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert cli.main(["-i", "no_such_file.ply", "-f", "spz"] + argv) is None      # refused before the input is looked at
    assert buf.getvalue().strip() == line


def test_cli_flags_become_run_keywords():
    cli = importlib.import_module("3dgsconverter_amd.cli")
    parse = lambda argv: cli.build_parser().parse_args(["-i", "a.ply", "-f", "spz"] + argv)
    assert cli.fidelity_kwargs(parse([])) == {} and cli.check_fidelity_args(parse([])) is None
    assert cli.fidelity_kwargs(parse(["--fidelity"])) == {"fidelity": "written"}
    args = parse(["--fidelity", "source", "--fidelity_views", "3", "--fidelity_size", "64", "48", "--fidelity_up=-z", "--fidelity_image", "w.png"])
    assert cli.check_fidelity_args(args) is None
    assert cli.fidelity_kwargs(args) == {"fidelity": "source", "fidelity_views": 3, "fidelity_size": (64, 48), "fidelity_up": "-z",
                                         "fidelity_image": "w.png"}
    args = parse(["--fidelity", "--fidelity_camera", "0", "0", "0", "0", "0", "1", "--fidelity_camera", "1", "0", "0", "0", "0", "0"])
    assert cli.check_fidelity_args(args) is None
    assert cli.fidelity_kwargs(args) == {"fidelity": "written", "fidelity_cameras": [(0.0, 0.0, 0.0, 0.0, 0.0, 1.0), (1.0, 0.0, 0.0, 0.0, 0.0, 0.0)]}
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        parse(["--fidelity", "both"])


def test_converter_refuses_before_any_file_is_read(tmp_path):
    conv = importlib.import_module("3dgsconverter_amd.converter")
    missing = str(tmp_path / "missing.ply")
    c = conv.Converter(missing, str(tmp_path / "out.spz"), "spz")
    with pytest.raises(ValueError, match="merge"):
        c.run(fidelity="source", merge=[str(tmp_path / "other.ply")])
    with pytest.raises(ValueError, match="mode"):
        c.run(fidelity="both")
    with pytest.raises(ValueError, match="fidelity_views need fidelity"):
        c.run(fidelity_views=4)
    with pytest.raises(ValueError, match="views"):
        c.run(fidelity="written", fidelity_views=0)
    assert c.last_fidelity == {} and not os.path.exists(str(tmp_path / "out.spz"))
