"""-m "not gpu": voxel decimation's host side, no device touched -- the promises of the definition (tests/decimate_numpy.py), its
moments against an independent two-pass computation and its eigen-solve against the matrix it decomposes, the conservation of
mass, the blocked-sum rule at the block edges, the plan's refusals (3dgsconverter_amd/decimate.py), the processor's refusals
before any device work, the command line's flag and the order of Converter.run's steps."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decimate_cases as dc  # noqa: E402
import decimate_numpy as dn  # noqa: E402
import ply_read_numpy as pn  # noqa: E402

lib = importlib.import_module("3dgsconverter_amd._lib")
dec = importlib.import_module("3dgsconverter_amd.decimate")

# 10 x the worst relative error the two tests below observed on their seeded inputs (numpy 2.x, x86-64): moments 7.57e-16
# (Frobenius; mean and covariance), reconstruction 2.26e-15
MOMENT_BOUND = 7.6e-15
RECONSTRUCTION_BOUND = 2.3e-14


@pytest.fixture(scope="module")
def cli():
    return importlib.import_module("3dgsconverter_amd.cli")


@pytest.fixture(scope="module")
def mixed():
    """the 1000-row mixed scene and its decimation with details, computed once"""
    t = dc.scene(248, 1000)
    out, info, details = dn.decimate_table(t, dc.H, want_details=True)
    return t, out, info, details


# ------------------------------------------------------------------------------------------------------------ the definition

@pytest.mark.parametrize("stride", dc.STRIDES)
def test_singletons_come_back_unchanged(stride):
    t = dc.scene(stride, 300, "singletons")
    out, info = dn.decimate_table(t, dc.H)
    assert out.tobytes() == t.tobytes() and info == {"groups": 300, "merged_groups": 0, "passed_through": 300}


def test_a_tiny_voxel_returns_the_table():
    t = dc.scene(248, 1000)                             # up to 300 rows per voxel of side H ...
    out, info = dn.decimate_table(t, 2.0 ** -18)        # ... and one per voxel of side 2^-18 (cells up to +-2^19)
    assert out.tobytes() == t.tobytes() and info["merged_groups"] == 0
    with pytest.raises(ValueError, match="too small for the scene's coordinates"):
        dn.decimate_table(t, 2.0 ** -21)


def test_groups_leave_in_first_appearance_order(mixed):
    t, out, info, details = mixed
    runs, _ = dn.groups_of(t, dc.H)
    firsts = [int(r[0]) for r in runs]
    assert firsts == sorted(firsts) and len(set(firsts)) == len(firsts) and firsts[0] == 0
    assert all(np.all(np.diff(r) > 0) for r in runs)                    # members in row order
    assert sorted(len(r) for r in runs) == sorted(dc.group_sizes(1000, "mixed"))
    assert info == {"groups": len(runs), "merged_groups": sum(len(r) > 1 for r in runs), "passed_through": sum(len(r) == 1 for r in runs)}
    for g, r in enumerate(runs):
        if len(r) == 1:
            assert out[g].tobytes() == t[r[0]].tobytes()
        else:                                                           # a field of no class: the first member's bytes
            assert out[g]["nx"] != t[r[0]]["nx"] or len(r) == 1
    copy_fields = [nm for nm in dc.splat_dtype(300).names if nm.startswith(("label", "extra_", "flag_"))]
    t3 = dc.scene(300, 400)
    out3, _ = dn.decimate_table(t3, dc.H)
    for g, r in enumerate(dn.groups_of(t3, dc.H)[0]):
        assert all(out3[nm][g].tobytes() == t3[nm][r[0]].tobytes() for nm in copy_fields)


def test_every_member_of_the_largest_group_is_in_one_cell(mixed):
    t, _, _, details = mixed
    big = max(details, key=lambda d: len(d["rows"]))
    assert len(big["rows"]) == 300
    cells = dn.cells_f32(t[big["rows"]], dc.H)
    assert (cells == cells[0]).all() and np.all(np.abs(cells) < 2 ** 20)


@pytest.mark.parametrize("k", (2, 7, 300))
def test_identical_members_give_that_splat(k):
    one = dc.scene(251, 1, seed=5)
    t = np.repeat(one, k)
    out, info = dn.decimate_table(t, dc.H)
    assert info == {"groups": 1, "merged_groups": 1, "passed_through": 0}
    for nm in "xyz":
        assert out[nm][0] == one[nm][0]                                 # exactly
    for nm in dn.mean_names(t.dtype):
        assert abs(float(out[nm][0]) - float(one[nm][0])) <= 2e-7 * abs(float(one[nm][0]))
    assert all(out[nm][0] == one[nm][0] for nm in dn.RGB)
    # the covariance, up to the float32 rounding of exp and log: rebuilt from the output row
    want = dc.member_covariances(one)[0]
    got = dc.member_covariances(out)[0]
    assert np.linalg.norm(got - want) <= 4e-6 * np.linalg.norm(want)


def _reference_moments(t, rows):
    sub = t[rows]
    with np.errstate(all="ignore"):
        w = dn.weight(sub).astype(np.float64)
    pos = np.stack([sub[nm].astype(np.float64) for nm in "xyz"], axis=1)
    return dc.two_pass_moments(pos, w, dc.member_covariances(sub))


def test_moments_against_a_two_pass_computation(mixed):
    """Observed on these seeded groups (2 ... 300 members): worst relative Frobenius error of the covariance and of the mean
    7.57e-16; MOMENT_BOUND is 10 x that."""
    t, _, _, details = mixed
    extra = dc.scene(104, 700, seed=3)
    groups = [(t, d) for d in details] + [(extra, d) for d in dn.decimate_table(extra, dc.H, want_details=True)[2]]
    assert len(groups) >= 12
    worst = 0.0
    for table, d in groups:
        mu, Sig = _reference_moments(table, d["rows"])
        got_mu = np.array([float(v) for v in d["mu"]])
        got_Sig = np.array([[float(d["Sigma"][j][k]) for k in range(3)] for j in range(3)])
        worst = max(worst, np.linalg.norm(got_Sig - Sig) / np.linalg.norm(Sig), np.linalg.norm(got_mu - mu) / np.linalg.norm(mu))
    print("moments: worst relative error %.3g" % worst)
    assert worst <= MOMENT_BOUND


def test_eigen_solve_reconstructs_its_matrix(mixed):
    """Observed: worst relative Frobenius error of V diag(lambda) V^T against Sigma 2.26e-15 over these groups and 2000 seeded
    SPD matrices with equal and triple eigenvalues and condition numbers up to e^20; RECONSTRUCTION_BOUND is 10 x that.  V is a
    proper rotation."""
    t, _, _, details = mixed
    mats = [np.array([[float(d["Sigma"][j][k]) for k in range(3)] for j in range(3)]) for d in details]
    rng = np.random.default_rng(11)
    for i in range(2000):
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        lam = np.exp(rng.uniform(-10, 10, 3))
        if i % 5 == 1:
            lam[1] = lam[0]
        if i % 5 == 2:
            lam[:] = lam[0]
        A = (Q * lam) @ Q.T
        mats.append((A + A.T) / 2)
    mats += [np.diag([3.0, 1.0, 2.0]), np.eye(3) * 0.25]
    worst = 0.0
    for A in mats:
        lam, V = dn.jacobi3([[A[j][k] for k in range(3)] for j in range(3)])
        V = np.array([[float(V[j][k]) for k in range(3)] for j in range(3)])
        lam = np.array([float(v) for v in lam])
        worst = max(worst, np.linalg.norm((V * lam) @ V.T - A) / np.linalg.norm(A))
        assert abs(np.linalg.det(V) - 1.0) < 1e-12 and np.linalg.norm(V @ V.T - np.eye(3)) < 1e-12
    print("reconstruction: worst relative error %.3g" % worst)
    assert worst <= RECONSTRUCTION_BOUND
    lam, V = dn.jacobi3([[3.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 2.0]])     # a diagonal matrix: nothing to rotate, nothing sorted
    assert [float(v) for v in lam] == [3.0, 1.0, 2.0] and all(float(V[j][k]) == (j == k) for j in range(3) for k in range(3))


def test_mass_is_conserved_where_the_clip_does_not_act(mixed):
    """alpha' vol' = W: in float64 from the definition's own intermediates to 4 ulp, and from the float32 fields of the output
    row to 1e-5 -- three log-scales and one logit, each a float32 log of relative error 2^-22 at most (csrc/np_log.h is within
    2 ulp), halved resp. amplified by 1 / (1 - alpha') <= 2 for alpha' <= 0.5 ... and never above 2^10 under the clip; the
    scenes' merged alphas stay far below 0.5, which the test checks."""
    t, out, _, details = mixed
    assert len(details) >= 8
    for g, d in zip([i for i, r in enumerate(dn.groups_of(t, dc.H)[0]) if len(r) > 1], details):
        assert float(d["alpha"]) == float(d["alpha_clamped"]) and float(d["alpha"]) < 0.5, "a scene built not to clip did"
        assert all(dn.LAMBDA_MIN < float(v) < dn.LAMBDA_MAX for v in d["lam"])
        vol = np.sqrt((d["lam"][0] * d["lam"][1]) * d["lam"][2])
        assert abs(float(d["alpha"] * vol) - float(d["W"])) <= 4 * np.spacing(float(d["W"]))
        row = out[g]
        vol32 = np.exp(np.float64(row["scale_0"]) + np.float64(row["scale_1"]) + np.float64(row["scale_2"]))
        alpha32 = 1.0 / (1.0 + np.exp(-np.float64(row["opacity"])))
        assert abs(alpha32 * vol32 - float(d["W"])) <= 1e-5 * float(d["W"])
    # ... and the cases built to clip do: opaque splats piled on one point
    pile = np.repeat(dc.scene(248, 1, seed=9, max_alpha=0.4), 50)
    pile["opacity"] = 6.0
    _, _, det = dn.decimate_table(pile, dc.H, want_details=True)
    assert float(det[0]["alpha"]) > 1.0 and float(det[0]["alpha_clamped"]) == 1.0 - 2.0 ** -10


@pytest.mark.parametrize("k", (1, 255, 256, 257, 513))
def test_blocked_sum_rule(k):
    rng = np.random.default_rng(k)
    terms = rng.standard_normal((k, 3)) * np.exp(rng.uniform(-20, 20, (k, 3)))
    terms[0, 1] = -0.0
    want = []
    for c in range(3):
        total = 0.0
        for a in range(0, k, 256):
            s = 0.0
            for v in terms[a:a + 256, c]:
                s = s + float(v)
            total = total + s
        want.append(total)
    got = dn.blocked_sum(terms)
    assert got.tobytes() == np.array(want).tobytes()
    assert np.signbit(dn.blocked_sum(np.full((1, 1), -0.0))[0]) == False   # noqa: E712  (from +0.0: no negative zero)


def test_the_unmergeable_rows_pass_through():
    t, rows = dc.plant_unmergeable(dc.scene(251, 600))
    with np.errstate(all="ignore"):
        ok = dn.mergeable(t)
    assert not ok[rows].any() and ok.sum() == len(t) - len(rows) and len(rows) >= 2 * len(dc.UNMERGEABLE)
    out, info = dn.decimate_table(t, dc.H)
    runs, _ = dn.groups_of(t, dc.H)
    alone = {int(r[0]) for r in runs if len(r) == 1}
    assert set(rows.tolist()) <= alone
    for g, r in enumerate(runs):
        if int(r[0]) in set(rows.tolist()):
            assert out[g].tobytes() == t[r[0]].tobytes()
    # a row beyond the cell range is refused only when it is mergeable
    far = t.copy()
    far["x"][rows[1]] = 1e30                                            # (its y is infinite)
    dn.decimate_table(far, dc.H)
    far["x"][0] = np.float32(2.0 ** 20 * dc.H)
    with pytest.raises(ValueError, match="too small"):
        dn.decimate_table(far, dc.H)
    far["x"][0] = np.float32(-(2.0 ** 20) * dc.H)                      # cell -2^20 is inside
    dn.decimate_table(far, dc.H)


def test_zero_names_are_zero_in_every_row():
    t = dc.scene(248, 300)
    names = ["f_rest_%d" % i for i in range(9, 45)]
    out, _ = dn.decimate_table(t, dc.H, zero_names=names)
    taken = t.copy()
    for nm in names:
        taken[nm] = 0
    want, _ = dn.decimate_table(taken, dc.H)
    assert out.tobytes() == want.tobytes() and all((out[nm].view(np.uint32) == 0).all() for nm in names)


# ------------------------------------------------------------------------------------------------------------ the plan

def test_plan_classes_and_refusals():
    for stride in dc.STRIDES:
        dt = dc.splat_dtype(stride)
        p = dec.plan_decimate(dt, 0.5)
        assert p.voxel_size == 0.5 and p.dtype == dt
        assert tuple(nm for nm, _ in p.mean) == dn.mean_names(dt) and tuple(nm for nm, _ in p.u8) == dn.u8_names(dt)
        assert p.xyz == tuple(dt.fields[nm][1] for nm in "xyz") and p.opacity == dt.fields["opacity"][1]
        assert p.float_names == dn.float_names(dt) and 10 + len(p.mean) + len(p.u8) <= 64
    dt = dc.splat_dtype(248)
    for bad in (0, -1.0, float("nan"), float("inf"), "x", None, True):
        with pytest.raises(ValueError, match="finite number greater than 0"):
            dec.plan_decimate(dt, bad)
    for nm in ("x", "scale_1", "rot_3", "opacity", "f_dc_1", "f_rest_7", "ny"):
        with pytest.raises(TypeError, match="field %r is <f8" % nm):
            dec.plan_decimate(np.dtype([(f, "<f8" if f == nm else "<f4") for f in dt.names]), 0.5)
    with pytest.raises(TypeError, match="field 'z' is >f4"):
        dec.plan_decimate(np.dtype([(f, ">f4" if f == "z" else "<f4") for f in dt.names]), 0.5)
    for nm in dec.GEOMETRY:
        less = np.dtype([(f, "<f4") for f in dt.names if f != nm])
        assert dec.missing_fields(less) == (nm,)
        with pytest.raises(ValueError, match="no field %r" % nm):
            dec.plan_decimate(less, 0.5)
    assert dec.missing_fields(dt) == ()
    assert tuple(nm for nm, _ in dec.plan_decimate(dt, 0.5, ["f_rest_44", "f_rest_9", "absent"]).zero) == ("f_rest_44", "f_rest_9")
    with pytest.raises(ValueError, match="cannot be zeroed"):
        dec.plan_decimate(dt, 0.5, ["scale_0"])
    with pytest.raises(ValueError, match="rows of 600 bytes"):
        dec.plan_decimate(np.dtype([(f, "<f4") for f in dt.names] + [("pad", "V352")]), 0.5)
    lay = lib.decimate_layout(dec.plan_decimate(dc.splat_dtype(251), 0.5, ["f_rest_3"]))
    assert (lay.n_mean, lay.n_u8, lay.n_zero, lay.voxel_size) == (51, 3, 1, 0.5) and lay.zero_offset[0] == dc.splat_dtype(251).fields["f_rest_3"][1]


# ------------------------------------------------------------------------------------------------------------ the processor

def test_decimate_refuses_before_any_device_work(monkeypatch, capsys):
    dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    monkeypatch.setattr(lib, "require_hip", lambda: (_ for _ in ()).throw(AssertionError("device work")))
    table = dc.scene(248, 10)
    for lazy in (False, True):
        p = dp.DataProcessor(table.copy(), lazy=lazy)
        for bad in (0, -3.0, float("nan"), float("inf"), "a", None):
            with pytest.raises(ValueError, match="finite number greater than 0"):
                p.decimate(bad)
        wide = dp.DataProcessor(table.astype(np.dtype([(nm, "<f8" if nm == "rot_1" else "<f4") for nm in table.dtype.names])), lazy=lazy)
        with pytest.raises(TypeError, match="field 'rot_1' is <f8"):
            wide.decimate(0.5)
        capsys.readouterr()
        for gone in ("z", "scale_1", "rot_0", "opacity"):
            bare = dp.DataProcessor(np.ascontiguousarray(table[[nm for nm in table.dtype.names if nm != gone]]), lazy=lazy)
            before = bare.data.tobytes()
            out = bare.decimate(0.5)
            assert capsys.readouterr().out.strip() == "Warning: Decimation needs x y z, scale_0..2, rot_0..3 and opacity. Decimation skipped."
            assert ((out is None) if lazy else (out is bare.data)) and bare.data.tobytes() == before
        with pytest.raises(AssertionError, match="device work"):        # ... and a good call does reach the device
            p.decimate(0.5)
    with pytest.raises(TypeError, match="structured array"):
        dp.DataProcessor([1, 2, 3]).decimate(0.5)


# ------------------------------------------------------------------------------------------------------------ the command line

def _scene(path):
    t = pn.build(10, pn.canonical_fields(3), np.random.default_rng(3))
    pn.write_ply(str(path), [("vertex", t)])
    return str(path)


def test_flag_parses(cli):
    a = cli.build_parser().parse_args(["-i", "a.ply", "-f", "spz", "--decimate_voxel_size", "0.05"])
    assert a.decimate_voxel_size == 0.05
    assert cli.build_parser().parse_args(["-i", "a.ply", "-f", "spz"]).decimate_voxel_size is None
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["-i", "a.ply", "-f", "spz", "--decimate_voxel_size", "small"])


@pytest.mark.parametrize("value", ["0", "-0.5", "nan", "inf"])
def test_voxel_size_error_returns_before_a_read(cli, capsys, tmp_path, monkeypatch, value):
    conv = importlib.import_module("3dgsconverter_amd.converter")
    monkeypatch.setattr(conv.SourceHandler, "read", lambda self, path, stage_ms=None: (_ for _ in ()).throw(AssertionError("read " + path)))
    assert cli.main(["-i", _scene(tmp_path / "a.ply"), "-f", "spz", "--decimate_voxel_size=" + value]) is None
    assert capsys.readouterr().out.strip().split("\n") == [f"Error: --decimate_voxel_size must be a finite number greater than 0. Got {float(value)}."]


def test_the_flag_is_an_active_filter_and_reaches_run(cli, capsys, tmp_path, monkeypatch):
    src = _scene(tmp_path / "a.ply")
    seen = {}
    monkeypatch.setattr(cli, "report_info", lambda *a, **k: None)
    monkeypatch.setattr(cli.Converter, "run", lambda self, **kw: seen.update(kw))
    cli.main(["-i", src, "-f", "3dgs", "--decimate_voxel_size", "0.125"])
    out = capsys.readouterr().out
    assert "Operation aborted" not in out and seen["decimate_voxel_size"] == 0.125
    seen.clear()
    cli.main(["-i", src, "-f", "spz"])
    assert "decimate_voxel_size" not in seen


def test_run_decimates_after_sor_and_before_the_budget(monkeypatch, tmp_path):
    """SOR -> decimate -> max_splats -> auto_bbox -> add_rgb_from_sh, whatever the order of the keywords"""
    conv = importlib.import_module("3dgsconverter_amd.converter")
    dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    table = dc.scene(248, 20)
    calls = []

    class Recorder:
        def __init__(self, data, resident=None):
            self.data, self.resident, self.resident_ms = data, None, {}

        def close(self):
            pass

        def __getattr__(self, name):
            if name.startswith("_"):
                raise AttributeError(name)
            return lambda *a, **k: calls.append((name, a, k))

    def read(self, path, stage_ms=None):
        self.profile = {"rest_nonzero": (1 << 45) - 1}
        return table

    monkeypatch.setattr(dp, "ChainedDataProcessor", Recorder)
    monkeypatch.setattr(conv.SourceHandler, "read", read)
    monkeypatch.setattr(conv.SourceHandler, "write", lambda self, data, path, stage_ms=None, **kw: None)
    monkeypatch.setattr(conv, "status_print", lambda *a, **k: None)
    src = _scene(tmp_path / "a.ply")
    conv.Converter(src, str(tmp_path / "o.splat"), "splat", resident=False).run(max_splats=5, decimate_voxel_size=0.5, sor_intensity=5.0,
                                                                                 auto_bbox=True, min_opacity=10)
    names = [c[0] for c in calls]
    assert names == ["cap_sh_degree", "apply_alpha_filter", "remove_flyers", "decimate", "limit_splats", "apply_auto_bbox", "add_rgb_from_sh"]
    assert calls[3][1] == (0.5,)
    calls.clear()
    conv.Converter(src, str(tmp_path / "o.spz"), "spz", resident=False).run(max_splats=5)
    assert "decimate" not in [c[0] for c in calls]
