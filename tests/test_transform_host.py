"""-m "not gpu": the scene transform's host side, no device touched -- transform.py's mathematics held to its identities in
float64, gsx_rows_transform_host (the kernel's per-row functions on the host) against the numpy definition of
tests/transform_numpy.py bit for bit, every refusal of plan_transform with its message, and the command line's three flags."""
import importlib
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ply_read_numpy as pn  # noqa: E402
import transform_cases as tc  # noqa: E402
import transform_numpy as tn  # noqa: E402

tf = importlib.import_module("3dgsconverter_amd.transform")
lib = importlib.import_module("3dgsconverter_amd._lib")
TOL = 1e-10     # a wrong sign, axis order or basis convention gives 0.1 ... 1; correct float64 about 1e-14


@pytest.fixture(scope="module")
def conv():
    return importlib.import_module("3dgsconverter_amd.converter")


@pytest.fixture(scope="module")
def cli():
    return importlib.import_module("3dgsconverter_amd.cli")


@pytest.fixture()
def no_reads(conv, monkeypatch):
    """any load of a source fails the test"""
    def refuse(self, path, stage_ms=None):
        raise AssertionError("the command line read %s" % path)
    monkeypatch.setattr(conv.SourceHandler, "read", refuse)


# ------------------------------------------------------------------------------------------------------------ mathematics

def axis_permutations():
    """the 24 proper signed permutation matrices"""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            for i in range(3):
                R[i, perm[i]] = signs[i]
            if np.linalg.det(R) > 0:
                out.append(R)
    assert len(out) == 24
    return out


def random_rotations(count, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        Q, r = np.linalg.qr(rng.standard_normal((3, 3)))
        Q = Q * np.sign(np.diag(r))
        if np.linalg.det(Q) < 0:
            Q[:, 0] = -Q[:, 0]
        out.append(Q)
    return out


ROTATIONS = random_rotations(50, 11) + axis_permutations()


def unit_directions(count, seed):
    d = np.random.default_rng(seed).standard_normal((count, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def rotmat(q):
    w, x, y, z = q
    n = w * w + x * x + y * y + z * z
    return np.array([[n - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), n - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), n - 2 * (x * x + y * y)]]) / n


def hamilton(p, q):
    w, x, y, z = p
    a, b, c, d = q
    return (((w * a - x * b) - y * c) - z * d, ((w * b + x * a) + y * d) - z * c, ((w * c - x * d) + y * a) + z * b,
            ((w * d + x * c) - y * b) + z * a)


def test_band_matrices_are_orthogonal_and_rotate_the_colour():
    dirs = unit_directions(32, 5)
    rng = np.random.default_rng(6)
    worst = {"orth": 0.0, "colour": 0.0}
    for R in ROTATIONS:
        tf.check_rotation(R)
        for band, D in zip((1, 2, 3), tf.sh_rotation(R)):
            nb = 2 * band + 1
            assert D.shape == (nb, nb)
            worst["orth"] = max(worst["orth"], float(np.max(np.abs(D @ D.T - np.eye(nb)))))
            c = rng.standard_normal(nb)
            diff = tf.sh_basis(dirs @ R.T, band) @ (D @ c) - tf.sh_basis(dirs, band) @ c
            worst["colour"] = max(worst["colour"], float(np.max(np.abs(diff))))
    print("max |D D^T - I| %.3g, max colour difference %.3g" % (worst["orth"], worst["colour"]))
    assert worst["orth"] <= TOL and worst["colour"] <= TOL, worst


def test_band_matrices_compose():
    worst = 0.0
    for R1, R2 in zip(ROTATIONS, ROTATIONS[7:] + ROTATIONS[:7]):
        for Da, Db, Dab in zip(tf.sh_rotation(R1), tf.sh_rotation(R2), tf.sh_rotation(R1 @ R2)):
            worst = max(worst, float(np.max(np.abs(Da @ Db - Dab))))
    print("max |D(R1) D(R2) - D(R1 R2)| %.3g" % worst)
    assert worst <= TOL


def test_quaternion_of_a_rotation():
    rng = np.random.default_rng(8)
    worst = 0.0
    for R in ROTATIONS:
        qr = tf.quat_from_rotation(R)
        assert qr[0] >= 0 and abs(sum(v * v for v in qr) - 1.0) <= TOL
        worst = max(worst, float(np.max(np.abs(rotmat(qr) - R))))
        q = tuple(rng.standard_normal(4))           # (any norm: the product keeps it)
        worst = max(worst, float(np.max(np.abs(rotmat(hamilton(qr, q)) - R @ rotmat(q)))))
    print("max |rotmat(q_R (x) q) - R rotmat(q)| %.3g" % worst)
    assert worst <= TOL


def test_identity_and_permutations_are_exact():
    for D, nb in zip(tf.sh_rotation(np.eye(3)), (3, 5, 7)):
        assert np.array_equal(D, np.eye(nb))
    assert tf.quat_from_rotation(np.eye(3)) == (1.0, 0.0, 0.0, 0.0)
    for R in axis_permutations():
        D1, D2, D3 = tf.sh_rotation(R)
        # band 1 is a signed permutation of (y, z, x) for every axis permutation; the higher bands mix under some of them, but
        # every entry that is 0 or +-1 to 1e-12 is exactly that
        assert set(np.unique(np.abs(D1))) <= {0.0, 1.0} and np.array_equal(np.abs(D1).sum(axis=0), np.ones(3))
        for D in (D2, D3):
            near = (np.abs(D) < 1e-9) | (np.abs(np.abs(D) - 1.0) < 1e-9)
            assert np.all((D[near] == 0.0) | (np.abs(D[near]) == 1.0))
    for angles in ((-90, 0, 0), (0, 90, 0), (0, 0, 180), (90, 270, -180), (360, -450, 90)):
        R = tf.rotation_from_euler_deg(*angles)
        assert set(np.unique(np.abs(R))) == {0.0, 1.0} and np.linalg.det(R) == 1.0 and not np.any(np.signbit(R[R == 0])), angles
        for D in tf.sh_rotation(R):
            near = (np.abs(D) < 1e-9) | (np.abs(np.abs(D) - 1.0) < 1e-9)
            assert np.all((D[near] == 0.0) | (np.abs(D[near]) == 1.0)), angles
    for deg in (90, 180, 270):          # quarter turns about Z permute every band up to signs
        for D in tf.sh_rotation(tf.rotation_from_euler_deg(0, 0, deg)):
            assert set(np.unique(np.abs(D))) <= {0.0, 1.0} and np.array_equal(np.abs(D).sum(axis=0), np.ones(len(D))), deg
    assert np.array_equal(tf.rotation_from_euler_deg(-90, 0, 0), [[1, 0, 0], [0, 0, 1], [0, -1, 0]])


def test_euler_order_is_x_then_y_then_z():
    R = tf.rotation_from_euler_deg(90, 0, 90)       # about fixed X first: the Y axis goes to Z; then about Z: stays Z
    assert np.array_equal(R @ [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]) and np.array_equal(R @ [1.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    a = np.radians(30.0)
    want = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    assert np.max(np.abs(tf.rotation_from_euler_deg(0, 0, 30) - want)) <= 1e-15


def test_check_rotation():
    R = ROTATIONS[0]
    assert np.array_equal(tf.check_rotation(R.tolist()), R)
    for bad, msg in ((np.eye(4), "3x3"), ([1, 2, 3], "3x3"), (np.full((3, 3), np.nan), "finite"), (np.eye(3) * 1.001, "orthonormal"),
                     (np.diag([1.0, 1.0, -1.0]), "reflection"), (R + 1e-8, "orthonormal"), ("abc", "3x3")):
        with pytest.raises(ValueError, match=msg):
            tf.check_rotation(bad)
    tf.check_rotation(R + 1e-11)


# ------------------------------------------------------------------------------------------------------------ the host twin

def run_host(table, kind, zero=()):
    R, s, t = tc.transforms()[kind]
    plan = tf.plan_transform(table.dtype, R, s, t)
    before = table.copy()
    got = lib.rows_transform_host(table, plan)
    assert table.tobytes() == before.tobytes(), "the input was written"
    if zero:
        lib.host_zero_columns(got, list(zero))
    return plan, got, tn.transform_table(table, R, s, t, zero_names=zero)


def check_against_definition(table, plan, got, want):
    diff = tn.same_by_class(got, want, tc.float_fields(table.dtype))
    assert diff is None, diff
    for nm in table.dtype.names:                # inactive and unrelated fields: the input's bytes
        if nm not in plan.written:
            assert got[nm].tobytes() == table[nm].tobytes(), nm


@pytest.mark.parametrize("kind", list(tc.transforms()))
@pytest.mark.parametrize("stride", tc.STRIDES)
def test_host_twin_is_the_definition(stride, kind):
    for n in (1, 129, 1000):
        table = tc.table(stride, n)
        plan, got, want = run_host(table, kind)
        check_against_definition(table, plan, got, want)
        in_place = table.copy()
        assert lib.rows_transform_host(in_place, plan, out=in_place) is in_place
        assert tn.same_by_class(in_place, want, tc.float_fields(table.dtype)) is None


def test_parts_follow_the_arguments():
    dt = tc.splat_dtype(248)
    P = tf.plan_transform
    assert P(dt).identity and P(dt, np.eye(3), 1.0, (0, 0, 0)).identity and P(dt).parts == tf.PART_POSITION
    assert P(dt, None, None, (0, 0, 1)).parts == tf.PART_POSITION and not P(dt, None, None, (0, 0, 1)).identity
    assert P(dt, None, 2.0).parts == tf.PART_POSITION | tf.PART_SCALES
    assert P(dt, tc.transforms()["rotation"][0]).parts == 127 - tf.PART_SCALES
    assert P(tc.splat_dtype(56), tc.transforms()["rotation"][0], 2.0).parts == tf.PART_POSITION | tf.PART_SCALES | tf.PART_ROTATION
    assert P(tc.splat_dtype(104), tc.transforms()["rotation"][0]).parts == 1 | 2 | 8 | 16
    assert P(tc.splat_dtype(167), tc.transforms()["rotation"][0]).parts == 1 | 2 | 8 | 16 | 32
    only_xyz = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("scale_0", "<f4"), ("rot_0", "<f4")])
    p = P(only_xyz, tc.transforms()["rotation"][0], 3.0)      # incomplete groups are absent: not touched
    assert p.parts == tf.PART_POSITION and p.normals == (-1, -1, -1) and p.written == ("x", "y", "z")


def test_quarter_turn_moves_the_axes_by_bits():
    table = tc.table(248, 1000)
    _, got, _ = run_host(table, "quarter_turn")
    # ((1 X + 0 Y) + 0 Z) + 0 is X by bits for finite X, Y, Z and X != 0 (an infinity times 0 is NaN, and -0 + 0 is +0)
    ok = np.ones(len(table), bool)
    for nm in ("x", "y", "z"):
        ok &= np.isfinite(table[nm]) & (table[nm] != 0)
    assert ok.sum() >= 800
    u = lambda a: a.view(np.uint32)     # noqa: E731
    assert np.array_equal(u(got["x"][ok]), u(table["x"][ok])) and np.array_equal(u(got["y"][ok]), u(table["z"][ok]))
    assert np.array_equal(u(got["z"][ok]), u((-table["y"])[ok]))


def test_edge_rows_hold_what_they_are_for():
    """the planted rows do produce denormal results, overflows and NaNs in the definition (so the comparison sees them)"""
    table = tc.table(248, 129)
    _, _, small = run_host(table, "rotation")
    _, _, big = run_host(table, "scale_up")
    tiny = np.float32(1.1754944e-38)
    for nm in ("x", "nx", "rot_0", "f_rest_0", "f_rest_10", "f_rest_44"):      # denormal results in every part a rotation writes
        assert np.any((np.abs(small[nm][:5]) < tiny) & (small[nm][:5] != 0)), nm
    assert np.isinf(big["x"][4]) and np.isfinite(table["x"][4])
    assert np.signbit(table["x"][1]) and table["x"][1] == 0
    for nm in tc.frame_fields(table.dtype):
        assert np.isnan(table[nm]).sum() == 1 and np.isinf(table[nm]).sum() == 1, nm


@pytest.mark.parametrize("degree", (0, 1, 2))
def test_capped_bands_are_filled_after_the_transform(degree):
    for stride in (248, 251, 167):
        table = tc.table(stride, 129)
        zero = tc.capped_names(table.dtype, degree)
        if not zero:
            continue
        capped_in = table.copy()
        lib.host_zero_columns(capped_in, zero)      # a table the cap has zeroed already ...
        for t, z in ((capped_in, ()), (table, zero), (capped_in, zero)):      # ... and the deferred fill, after the transform
            plan, got, want = run_host(t, "all_three", z)
            assert tn.same_by_class(got, want, tc.float_fields(t.dtype)) is None
            for nm in z:
                assert not got[nm].view(np.uint32).any(), nm


def test_host_twin_refusals():
    import ctypes as C
    dt = tc.splat_dtype(248)
    table = tc.table(248, 4)
    plan = tf.plan_transform(dt, tc.transforms()["rotation"][0], 2.0, (1, 2, 3))
    L = lib.load()
    out = np.empty_like(table)

    def call(lay, stride=248, n=4):
        return L.gsx_rows_transform_host(table.ctypes.data, stride, n, C.byref(lay), out.ctypes.data)
    lay = lib.transform_layout(plan)
    assert call(lay) == 0 and call(lay, n=0) == 0
    assert call(lay, stride=0) != 0 and call(lay, stride=513) != 0 and call(lay, n=-1) != 0
    assert "gsx_rows_transform_host" in lib.last_error()
    for field, value, word in (("xyz_offset", 246, "position"), ("rot_offset", -1, "rotation"), ("scale_offset", 0, "overlaps"),
                               ("rest_offset", 245, "f_rest")):
        lay = lib.transform_layout(plan)
        getattr(lay, field)[1] = value
        assert call(lay) != 0 and word in lib.last_error(), (field, lib.last_error())
    lay = lib.transform_layout(plan)
    lay.parts = 128
    assert call(lay) != 0
    lay = lib.transform_layout(plan)
    lay.rest_m = 8                                  # band 3 of 8 coefficients per channel
    assert call(lay) != 0 and "band 3" in lib.last_error()
    assert L.gsx_rows_transform_host(None, 248, 4, C.byref(lib.transform_layout(plan)), out.ctypes.data) != 0
    with pytest.raises(ValueError, match="1-D C-contiguous table"):
        lib.rows_transform_host(tc.table(251, 4), plan)


# ------------------------------------------------------------------------------------------------------------ refusals

def test_plan_transform_refusals():
    dt = tc.splat_dtype(248)
    R = tc.transforms()["rotation"][0]
    P = tf.plan_transform
    for missing in "xyz":
        with pytest.raises(ValueError, match=f"the table has no field '{missing}'; x, y and z are needed"):
            P(np.dtype([(nm, "<f4") for nm in dt.names if nm != missing]), R)
    for s in (0, -1.0, float("inf"), float("nan"), "big"):
        with pytest.raises(ValueError, match="the scale must be a finite number greater than 0, got"):
            P(dt, None, s)
    for t in ((0, 0, float("nan")), (0, float("inf"), 0), (1, 2), "abc", (1, 2, 3, 4)):
        with pytest.raises(ValueError, match="the translation must be three finite numbers, got"):
            P(dt, None, None, t)
    with pytest.raises(ValueError, match="not orthonormal"):
        P(dt, np.eye(3) * 2)
    with pytest.raises(ValueError, match="reflection"):
        P(dt, np.diag([1.0, -1.0, 1.0]))

    def with_type(name, other):
        return np.dtype([(nm, other if nm == name else "<f4") for nm in dt.names])
    for name, args in (("x", (None, None, (1, 0, 0))), ("z", (R,)), ("scale_1", (None, 2.0)), ("rot_3", (R,)), ("nx", (R,)), ("f_rest_44", (R,)),
                       ("f_rest_0", (R,))):
        for other in ("<f8", ">f4", "<f2", "<i4"):
            with pytest.raises(TypeError, match=f"field '{name}' is {np.dtype(other).str}, and the transform writes '<f4' fields only"):
                P(with_type(name, other), *args)
    # a field the transform would NOT write may have any type
    assert P(with_type("scale_1", "<f8"), R).parts == 127 - tf.PART_SCALES
    assert P(with_type("rot_3", "<f8"), None, 2.0).parts == tf.PART_POSITION | tf.PART_SCALES
    assert P(with_type("f_rest_7", "<i4"), None, 2.0, (1, 1, 1)).parts == tf.PART_POSITION | tf.PART_SCALES
    assert P(with_type("opacity", "<f8"), R, 2.0).parts == 127 and P(with_type("f_dc_0", "<f2"), R).parts == 127 - tf.PART_SCALES
    base = [(nm, "<f4") for nm in tc.splat_dtype(56).names]
    for n_rest in (1, 3, 8, 10, 12, 30, 44, 46, 48):
        dtn = np.dtype(base + [("f_rest_%d" % i, "<f4") for i in range(n_rest)])
        with pytest.raises(ValueError, match=f"{n_rest} f_rest fields cannot be rotated: whole bands of three colour channels"):
            P(dtn, R)
        assert P(dtn, None, 2.0, (1, 0, 0)).parts == tf.PART_POSITION | tf.PART_SCALES      # ... and are no obstacle without a rotation
    gap = np.dtype(base + [("f_rest_%d" % i, "<f4") for i in range(10) if i != 4])
    with pytest.raises(ValueError, match="9 f_rest fields cannot be rotated"):
        P(gap, R)
    for n_rest, parts in ((0, 0), (9, 16), (24, 48), (45, 112)):
        dtn = np.dtype(base + [("f_rest_%d" % i, "<f4") for i in range(n_rest)])
        assert P(dtn, R).parts == (tf.PART_POSITION | tf.PART_ROTATION | parts) and P(dtn, R).m == n_rest // 3
    with pytest.raises(ValueError, match="finite"):
        tf.rotation_from_euler_deg(float("nan"), 0, 0)


def test_apply_transform_refuses_before_any_device_work(monkeypatch):
    dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    monkeypatch.setattr(lib, "require_hip", lambda: (_ for _ in ()).throw(AssertionError("device work")))
    table = tc.table(248, 10)
    for lazy in (False, True):
        p = dp.DataProcessor(table.copy(), lazy=lazy)
        with pytest.raises(ValueError, match="scale"):
            p.apply_transform(scale=0.0)
        with pytest.raises(ValueError, match="orthonormal"):
            p.apply_transform(rotation=np.ones((3, 3)))
        bad = dp.DataProcessor(table.astype(np.dtype([(nm, "<f8" if nm == "y" else "<f4") for nm in table.dtype.names])), lazy=lazy)
        with pytest.raises(TypeError, match="field 'y' is <f8"):
            bad.apply_transform(translation=(1, 0, 0))
        # identity arguments return at once: the table itself, no device
        out = p.apply_transform(rotation=np.eye(3), translation=(0, 0, 0), scale=1.0)
        assert (out is None) if lazy else (out is p.data)
        assert p.data.tobytes() == table.tobytes() and p.apply_transform() is out
    with pytest.raises(TypeError, match="structured array"):
        dp.DataProcessor([1, 2, 3]).apply_transform(scale=2.0)


# ------------------------------------------------------------------------------------------------------------ the command line

def _scene(path):
    t = pn.build(10, pn.canonical_fields(3), np.random.default_rng(3))
    pn.write_ply(str(path), [("vertex", t)])
    return str(path)


def test_flags_parse(cli):
    a = cli.build_parser().parse_args(["-i", "a.ply", "-f", "spz", "--rotate", "-90", "0", "12.5", "--scale", "0.5", "--translate", "1", "-2", "3e-1"])
    assert a.rotate == [-90.0, 0.0, 12.5] and a.scale == 0.5 and a.translate == [1.0, -2.0, 0.3]
    a = cli.build_parser().parse_args(["-i", "a.ply", "-f", "spz"])
    assert a.rotate is None and a.scale is None and a.translate is None


@pytest.mark.parametrize("value", ["0", "-2", "nan", "inf"])
def test_scale_error_returns_before_a_read(cli, no_reads, capsys, tmp_path, value):
    assert cli.main(["-i", _scene(tmp_path / "a.ply"), "-f", "spz", "--scale=" + value]) is None
    assert capsys.readouterr().out.strip().split("\n") == [f"Error: --scale must be a finite number greater than 0. Got {float(value)}."]


@pytest.mark.parametrize("flags", [["--translate", "1", "0", "0"], ["--rotate", "0", "0", "90"], ["--scale", "2"]])
def test_a_transform_is_no_no_op(cli, capsys, tmp_path, monkeypatch, flags):
    """.ply -> .ply 3dgs with only a transform flag is not stopped by the same-extension rule: it goes on to the conversion"""
    src = _scene(tmp_path / "a.ply")
    seen = {}
    monkeypatch.setattr(cli, "report_info", lambda *a, **k: None)
    monkeypatch.setattr(cli.Converter, "run", lambda self, **kw: seen.update(kw))
    cli.main(["-i", src, "-f", "3dgs"] + flags)
    out = capsys.readouterr().out
    assert "Operation aborted" not in out and "no filters are active" not in out
    want = {"rotate": None, "scale": None, "translate": None}
    want[flags[0][2:]] = [float(v) for v in flags[1:]] if len(flags) > 2 else float(flags[1])
    assert {k: seen[k] for k in want} == want
    cli.main(["-i", src, "-f", "3dgs"])             # ... and without one it still is
    assert "Operation aborted to prevent redundant processing." in capsys.readouterr().out
