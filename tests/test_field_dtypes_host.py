"""Tables whose fields are not little-endian float32, without a GPU (tests/dtypes_cases.py names the cases).

The rule ("Field dtypes"): every entry point gives the reference's answer for a dtype or raises TypeError naming the
field and its dtype -- before any device work, with the table and the device chain untouched.  Checked here: every refusal (it
comes before the device, so it needs none), the eager row filters that run on the host, and the dtype-preserving oracle against
the reference's own results in tests/golden/dtypes_ref.npz (tests/devtools/make_golden_dtypes.py).  The adversarial tables must
really change the reference's answer under a float32 cast, so that their refusal tests cannot pass vacuously.
"""
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dtypes_cases as dc                  # noqa: E402
from oracle import density as oden, sor as osor   # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "dtypes_ref.npz"))
SPEC = json.loads(bytes(GOLD["spec"]))


def _mod(name):
    return importlib.import_module("3dgsconverter_amd." + name)


def _mask(key, n):
    return np.unpackbits(GOLD[key])[:n].astype(bool)


def _snapshot(t):
    return dc.field_bytes(t), t.dtype, t.shape


def _bad_field(t, op):
    """the field the refusal must name: the first of x, y, z that the entry point cannot take"""
    lib = _mod("_lib")
    if op == "sor":
        return lib.f32_inexact_field(t, dc.XYZ)[0]
    return next(f for f in dc.XYZ if not lib.is_f4(t.dtype[f]))


# ------------------------------------------------------------------------------------------------------------ the fixture
def test_fixture_covers_every_case():
    assert SPEC["N"] == dc.N and SPEC["N_LARGE"] == dc.N_LARGE
    for case in dc.CASES:
        for key in ("sor/%s/mask", "density/%s/mask", "alpha/%s/mask", "crop/%s/mask", "rgb/%s", "cap/%s", "cply/%s/vertex"):
            assert key % case in GOLD.files, key % case
    for case in dc.LARGE_CASES:
        assert "large/sor/%s/mask" % case in GOLD.files


def test_cases_have_the_dtypes_and_layouts_they_claim():
    for case in dc.CASES:
        t = dc.table(case)
        assert len(t) == dc.N and t.dtype["extra"] == np.dtype("<f8") if "extra" in t.dtype.names else case == "subset"
        assert (t["orig_index"] == np.arange(dc.N)).all()
    assert not dc.table("strided").flags.c_contiguous
    sub = dc.table("subset")
    assert sub.dtype.itemsize > sum(sub.dtype[nm].itemsize for nm in sub.dtype.names)       # padding inside the row
    assert dc.table("f4be").dtype["opacity"] == np.dtype(">f4") and dc.table("f2").dtype["f_rest_3"] == np.dtype("<f2")
    lib = _mod("_lib")
    assert lib.f32_inexact_field(dc.table("f8r"), dc.XYZ) is None
    assert lib.f32_inexact_field(dc.table("f8"), dc.XYZ)[0] == "x"
    assert lib.f32_inexact_field(dc.table("mixed_x8"), dc.XYZ)[0] == "x"


# ------------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("case", dc.CASES)
def test_dtype_preserving_oracle_is_the_reference(case):
    """oracle.sor.sor_table / oracle.density.density_filter_table reproduce the reference's masks on every dtype; where an
    entry point takes the case, the float32 oracle on the float32 copy does too (the cast the device makes is exact there)"""
    t = dc.table(case)
    n = len(t)
    got = osor.sor_table(t, dc.SOR_K, dc.SOR_SIGMA)
    np.testing.assert_array_equal(got["mask"], _mask("sor/%s/mask" % case, n))
    assert np.float32(got["threshold"]).tobytes() == GOLD["sor/%s/threshold" % case].tobytes()
    d = oden.density_filter_table(t, **dc.DENSITY_KW)
    np.testing.assert_array_equal(d["mask"], _mask("density/%s/mask" % case, n))
    xyz32 = np.column_stack([np.asarray(t[f], np.float32) for f in dc.XYZ])
    if case in dc.ACCEPT["sor"]:
        np.testing.assert_array_equal(osor.sor(xyz32, dc.SOR_K, dc.SOR_SIGMA)["mask"], got["mask"])
    if case in dc.ACCEPT["density"]:
        np.testing.assert_array_equal(oden.density_filter(xyz32, **dc.DENSITY_KW)["mask"], d["mask"])


@pytest.mark.parametrize("case", dc.LARGE_CASES)
def test_dtype_preserving_oracle_is_the_reference_large(case):
    t = dc.table(case, dc.N_LARGE, seed=2)
    np.testing.assert_array_equal(osor.sor_table(t, dc.SOR_K, dc.SOR_SIGMA)["mask"], _mask("large/sor/%s/mask" % case, len(t)))
    if case in dc.ACCEPT["density"]:
        np.testing.assert_array_equal(oden.density_filter_table(t, **dc.DENSITY_KW)["mask"],
                                      _mask("large/density/%s/mask" % case, len(t)))


def test_adversarial_sor_table_changes_under_a_cast():
    t = dc.adv_sor_table()
    ref = osor.sor_table(t, dc.ADV_SOR["k"], dc.ADV_SOR["sigma"])
    np.testing.assert_array_equal(ref["mask"], _mask("adv_sor/mask", len(t)))
    np.testing.assert_array_equal(ref["mean_dists"], GOLD["adv_sor/mean_dists"])
    cast = osor.sor_table(dc.cast_f32(t), dc.ADV_SOR["k"], dc.ADV_SOR["sigma"])
    assert (cast["mean_dists"] != ref["mean_dists"]).any()
    assert (cast["mask"] != ref["mask"]).any()


def test_adversarial_density_tables_change_under_a_cast():
    t = dc.adv_density_table()
    kw = dict(voxel_size=dc.ADV_DENSITY["voxel_size"], threshold_percentage=dc.ADV_DENSITY["threshold_percentage"])
    ref = oden.density_filter_table(t, **kw)
    np.testing.assert_array_equal(ref["mask"], _mask("adv_density/mask", len(t)))
    assert (oden.voxel_keys_table(dc.cast_f32(t), kw["voxel_size"]) != oden.voxel_keys_table(t, kw["voxel_size"])).any()
    assert (oden.density_filter_table(dc.cast_f32(t), **kw)["mask"] != ref["mask"]).any()
    # float64 values that float32 holds exactly: the cast is exact, the float32 DIVISION still moves keys
    t = dc.adv_div_table()
    keys = oden.voxel_keys_table(t, dc.ADV_DIV["voxel_size"])
    np.testing.assert_array_equal(keys, GOLD["adv_div/keys"])
    assert _mod("_lib").f32_inexact_field(t, dc.XYZ) is None
    assert (oden.voxel_keys_table(dc.cast_f32(t), dc.ADV_DIV["voxel_size"]) != keys).any()


# ------------------------------------------------------------------------------------------------------------ refusals
def _check_refusal(fn, t, field, before):
    with pytest.raises(TypeError) as ei:
        fn()
    msg = str(ei.value)
    assert repr(field) in msg and t.dtype[field].str in msg, msg
    assert _snapshot(t) == before


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("intensity", [None, 5])
@pytest.mark.parametrize("case", [c for c in dc.CASES if c not in dc.ACCEPT["sor"]])
def test_remove_flyers_refuses(case, lazy, intensity):
    DP = _mod("processing.data_processor").DataProcessor
    t = dc.table(case)
    p = DP(t, lazy=lazy)
    _check_refusal(lambda: p.remove_flyers(dc.SOR_K, dc.SOR_SIGMA, intensity=intensity), t, _bad_field(t, "sor"), _snapshot(t))
    assert p._data is t and p._chain is None and len(p) == len(t)


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("sensitivity", [None, 0.5])
@pytest.mark.parametrize("case", [c for c in dc.CASES if c not in dc.ACCEPT["density"]])
def test_apply_density_filter_refuses(case, lazy, sensitivity):
    DP = _mod("processing.data_processor").DataProcessor
    t = dc.table(case)
    p = DP(t, lazy=lazy)
    _check_refusal(lambda: p.apply_density_filter(sensitivity=sensitivity, **dc.DENSITY_KW), t, _bad_field(t, "density"),
                   _snapshot(t))
    assert p._data is t and p._chain is None


@pytest.mark.parametrize("lazy", [False, True])
def test_adversarial_tables_are_refused(lazy):
    """the parent commit cast these to float32 and returned the float32 answer (test_adversarial_*_changes_under_a_cast)"""
    DP = _mod("processing.data_processor").DataProcessor
    t = dc.adv_sor_table()
    p = DP(t, lazy=lazy)
    _check_refusal(lambda: p.remove_flyers(dc.ADV_SOR["k"], dc.ADV_SOR["sigma"]), t, "x", _snapshot(t))
    for t, kw in ((dc.adv_density_table(), dict(voxel_size=dc.ADV_DENSITY["voxel_size"],
                                                 threshold_percentage=dc.ADV_DENSITY["threshold_percentage"])),
                  (dc.adv_div_table(), dict(voxel_size=dc.ADV_DIV["voxel_size"], threshold_percentage=0.1))):
        p = DP(t, lazy=lazy)
        _check_refusal(lambda: p.apply_density_filter(**kw), t, "x", _snapshot(t))
        assert p._chain is None


def test_host_gather_refuses_values_float32_does_not_hold():
    lib = _mod("_lib")
    t = dc.table("mixed_x8")
    with pytest.raises(TypeError, match="'x'"):
        lib.host_gather_xyz(t)
    got = lib.host_gather_xyz(dc.table("f8r"))
    assert got.tobytes() == lib.host_gather_xyz(dc.table("f4le")).tobytes()
    assert lib.host_gather_xyz(t, exact=False).dtype == np.float32      # the device chain's copy (DataProcessor checks first)


@pytest.mark.parametrize("case", [c for c in dc.CASES if c not in dc.ACCEPT["writer"]])
def test_compressed_ply_and_sog_writers_refuse(case, tmp_path):
    t = dc.table(case)
    before = _snapshot(t)
    cw = _mod("formats.compressed_ply_writer")
    with pytest.raises(TypeError, match="Compressed PLY writer: field '"):
        cw.encode(t)
    with pytest.raises(TypeError, match="Compressed PLY writer"):
        cw.write_compressed_ply(t, str(tmp_path / "a.ply"))
    sw = _mod("formats.sog_writer")
    for resident in (None, True, False):
        with pytest.raises(TypeError, match="SOG writer: field '"):
            sw.encode(t, 0, device_resident=resident)
    with pytest.raises(TypeError, match="SOG writer"):
        sw.write_sog(t, str(tmp_path / "a.sog"))
    assert _snapshot(t) == before and not any(tmp_path.iterdir())


def test_cply_pack_refuses_columns_that_are_not_float32():
    lib = _mod("_lib")
    cols = {nm: np.zeros(8, np.float32) for nm in lib.CPLY_COLUMNS}
    cols["y"] = np.zeros(8, np.float64)
    with pytest.raises(TypeError, match="'y' is <f8"):
        lib.cply_pack(cols, np.arange(8, dtype=np.uint32))
    cols["y"] = np.zeros(8, np.float32)
    with pytest.raises(TypeError, match=r"sh_columns\[1\]"):
        lib.cply_pack(cols, np.arange(8, dtype=np.uint32), [np.zeros(8, np.float32), np.zeros(8, np.float16)])


@pytest.mark.parametrize("case", [c for c in dc.CASES if c not in dc.ACCEPT["writer_le"]])
def test_spz_and_ksplat_writers_refuse(case, tmp_path):
    """the contract the SPZ and .ksplat writers already had: little-endian float32 only, refused before the device"""
    t = dc.table(case)
    before = _snapshot(t)
    with pytest.raises(TypeError, match="SPZ writer: field '.*' is "):
        _mod("formats.spz_writer").write_spz(t, str(tmp_path / "a.spz"))
    for level in (0, 1, 2):
        with pytest.raises(TypeError, match="KSplat writer: field '.*' is "):
            _mod("formats.ksplat_writer").write_ksplat(t, str(tmp_path / "a.ksplat"), compression_level=level)
    assert _snapshot(t) == before and not any(tmp_path.iterdir())


# ------------------------------------------------------------------------------------------------------------ host-side methods
@pytest.mark.parametrize("case", dc.CASES)
def test_eager_row_filters_keep_the_reference_expressions(case):
    """apply_alpha_filter / crop_by_bbox (eager: numpy's expressions on the columns in their own dtype, threaded compaction),
    cap_sh_degree and apply_auto_bbox give the reference's results for every dtype"""
    dpm = _mod("processing.data_processor")
    t = dc.table(case)
    n = len(t)
    np.testing.assert_array_equal(dc.masks_from_rows(dpm.DataProcessor(t).apply_alpha_filter(dc.ALPHA_MIN), n),
                                  _mask("alpha/%s/mask" % case, n))
    np.testing.assert_array_equal(dc.masks_from_rows(dpm.DataProcessor(t).crop_by_bbox(*dc.BOX), n), _mask("crop/%s/mask" % case, n))
    p = dpm.DataProcessor(np.array(t))
    p.cap_sh_degree(1)
    assert hashlib.sha256(dc.field_bytes(p.data)).digest() == GOLD["cap/" + case].tobytes()
    assert p.data.dtype == t.dtype
    msgs = []
    saved = dpm.status_print
    dpm.status_print = lambda *a, **kw: msgs.append(" ".join(map(str, a)))
    try:
        dpm.DataProcessor(t).apply_auto_bbox()
    finally:
        dpm.status_print = saved
    assert msgs[-1] == SPEC["bbox_message"][case]


def test_filter_sor_gpu_casts_like_the_reference_taichi_path():
    """gpu_ops.filter_sor_gpu takes an (N, 3) array and casts it to float32 -- what the reference's own Taichi path does
    (gpu_ops.py:200): a shape error is still raised before the cast and the device"""
    with pytest.raises(ValueError, match="Requires 3D data"):
        _mod("processing.gpu_ops").filter_sor_gpu(np.zeros((10, 2), np.float64))
