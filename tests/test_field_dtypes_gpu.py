"""Tables whose fields are not little-endian float32, on the MI355X: every case an entry point takes must give the reference's
answer (tests/golden/dtypes_ref.npz) and the dtype-preserving oracle's, bit for bit, and exactly what the little-endian float32
table with the same numbers gives.  The refusals themselves are tests/test_field_dtypes_host.py's."""
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

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "dtypes_ref.npz"))
SPEC = json.loads(bytes(GOLD["spec"]))


def _mod(name):
    return importlib.import_module("3dgsconverter_amd." + name)


def _mask(key, n):
    return np.unpackbits(GOLD[key])[:n].astype(bool)


def _dp(t, lazy):
    return _mod("processing.data_processor").DataProcessor(t, lazy=lazy)


def _survivors(p, n):
    return dc.masks_from_rows(p.data, n)


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("case", sorted(dc.ACCEPT["sor"]))
def test_remove_flyers_is_the_reference(gsx, case, lazy):
    t = dc.table(case)
    n = len(t)
    p = _dp(t, lazy)
    p.remove_flyers(dc.SOR_K, dc.SOR_SIGMA)
    got = _survivors(p, n)
    np.testing.assert_array_equal(got, _mask("sor/%s/mask" % case, n))
    np.testing.assert_array_equal(got, osor.sor_table(t, dc.SOR_K, dc.SOR_SIGMA)["mask"])
    assert np.float32(p.last_sor["threshold"]).tobytes() == GOLD["sor/%s/threshold" % case].tobytes()
    assert p.data.dtype == t.dtype                     # the surviving rows keep their own dtypes
    q = _dp(dc.f4le_equivalent(t), lazy)
    q.remove_flyers(dc.SOR_K, dc.SOR_SIGMA)
    np.testing.assert_array_equal(_survivors(q, n), got)
    assert np.float32(q.last_sor["threshold"]).tobytes() == np.float32(p.last_sor["threshold"]).tobytes()


@pytest.mark.parametrize("case", ["f4be", "f2", "f8r", "mixed_x8r"])
def test_sor_mean_distances_are_the_dtype_preserving_oracles(gsx, case):
    lib = _mod("_lib")
    t = dc.table(case)
    res = lib.sor_filter(lib.host_gather_xyz(t), dc.SOR_K, dc.SOR_SIGMA)
    np.testing.assert_array_equal(res["mean_dists"], osor.sor_table(t, dc.SOR_K, dc.SOR_SIGMA)["mean_dists"])


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("case", sorted(dc.ACCEPT["density"]))
def test_apply_density_filter_is_the_reference(gsx, case, lazy):
    t = dc.table(case)
    n = len(t)
    p = _dp(t, lazy)
    p.apply_density_filter(**dc.DENSITY_KW)
    got = _survivors(p, n)
    np.testing.assert_array_equal(got, _mask("density/%s/mask" % case, n))
    np.testing.assert_array_equal(got, oden.density_filter_table(t, **dc.DENSITY_KW)["mask"])
    q = _dp(dc.f4le_equivalent(t), lazy)
    q.apply_density_filter(**dc.DENSITY_KW)
    np.testing.assert_array_equal(_survivors(q, n), got)


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("case", dc.LARGE_CASES)
def test_large_tables_through_the_pinned_gather(gsx, case, lazy):
    """>= 65 536 rows: _xyz_rows / DeviceChain gather into the arena's page-locked buffer"""
    t = dc.table(case, dc.N_LARGE, seed=2)
    n = len(t)
    p = _dp(t, lazy)
    p.remove_flyers(dc.SOR_K, dc.SOR_SIGMA)
    np.testing.assert_array_equal(_survivors(p, n), _mask("large/sor/%s/mask" % case, n))
    if case in dc.ACCEPT["density"]:
        p = _dp(t, lazy)
        p.apply_density_filter(**dc.DENSITY_KW)
        np.testing.assert_array_equal(_survivors(p, n), _mask("large/density/%s/mask" % case, n))
    else:
        with pytest.raises(TypeError):
            _dp(t, lazy).apply_density_filter(**dc.DENSITY_KW)


@pytest.mark.parametrize("case", dc.CASES)
def test_lazy_row_filters_colours_and_box_are_the_reference(gsx, case):
    n = dc.N
    t = dc.table(case)
    p = _dp(t, True)
    p.apply_alpha_filter(dc.ALPHA_MIN)
    np.testing.assert_array_equal(_survivors(p, n), _mask("alpha/%s/mask" % case, n))
    p = _dp(t, True)
    p.crop_by_bbox(*dc.BOX)
    np.testing.assert_array_equal(_survivors(p, n), _mask("crop/%s/mask" % case, n))
    for lazy in (False, True):
        p = _dp(t, lazy)
        p.add_rgb_from_sh()
        rgb = np.column_stack([p.data[c] for c in ("red", "green", "blue")])
        assert hashlib.sha256(rgb.tobytes()).digest() == GOLD["rgb/" + case].tobytes(), lazy


@pytest.mark.parametrize("case", ["mixed_x8", "mixed_x8r"])
def test_a_refusal_leaves_the_lazy_chain_alone(gsx, case):
    """the alpha filter starts the device chain on a table with a float32 opacity whatever its x/y/z; SOR / density refused
    afterwards leave it as it was, and the box is taken from the table's own values where float32 does not hold them"""
    dpm = _mod("processing.data_processor")
    t = dc.table(case)
    n = len(t)
    p = _dp(t, True)
    p.apply_alpha_filter(dc.ALPHA_MIN)
    left = p._chain.n
    if case not in dc.ACCEPT["sor"]:
        with pytest.raises(TypeError):
            p.remove_flyers(dc.SOR_K, dc.SOR_SIGMA)
    with pytest.raises(TypeError):
        p.apply_density_filter(**dc.DENSITY_KW)
    assert p._chain is not None and p._chain.n == left and p._data is t
    msgs = []
    saved = dpm.status_print
    dpm.status_print = lambda *a, **kw: msgs.append(" ".join(map(str, a)))
    try:
        p.apply_auto_bbox()
    finally:
        dpm.status_print = saved
    kept = p.data
    np.testing.assert_array_equal(dc.masks_from_rows(kept, n), _mask("alpha/%s/mask" % case, n))
    lo = [np.min(kept[c]) for c in dc.XYZ]
    hi = [np.max(kept[c]) for c in dc.XYZ]
    assert msgs[-1] == (f"Auto-BBox Applied: [{lo[0]:.4f}, {lo[1]:.4f}, {lo[2]:.4f}] to "
                        f"[{hi[0]:.4f}, {hi[1]:.4f}, {hi[2]:.4f}]")


def test_filter_sor_gpu_casts_as_the_reference_does(gsx):
    """the reference's Taichi path casts its (N, 3) input to float32 (gpu_ops.py:200): so does this one"""
    t = dc.adv_sor_table()
    xyz = np.column_stack([t[c] for c in dc.XYZ])
    go = _mod("processing.gpu_ops")
    got = go.filter_sor_gpu(xyz, dc.ADV_SOR["k"], dc.ADV_SOR["sigma"])
    np.testing.assert_array_equal(got, go.filter_sor_gpu(xyz.astype(np.float32), dc.ADV_SOR["k"], dc.ADV_SOR["sigma"]))
    np.testing.assert_array_equal(got, osor.sor(xyz.astype(np.float32), dc.ADV_SOR["k"], dc.ADV_SOR["sigma"])["mask"])
    assert (got != _mask("adv_sor/mask", len(t))).any()      # (the table's own float64 answer is another one)


@pytest.mark.parametrize("case", sorted(dc.ACCEPT["writer"]))
def test_compressed_ply_is_the_reference(gsx, case):
    t = dc.table(case)
    chunk, vertex, sh, _ = _mod("formats.compressed_ply_writer").encode(t)
    for name, el in (("chunk", chunk), ("vertex", vertex), ("sh", sh)):
        b = b"" if el is None else np.ascontiguousarray(el).tobytes()
        assert hashlib.sha256(b).digest() == GOLD["cply/%s/%s" % (case, name)].tobytes(), name


@pytest.mark.parametrize("resident", [True, False])
@pytest.mark.parametrize("case", sorted(dc.ACCEPT["writer"] - {"f4le"}))
def test_sog_equals_the_little_endian_float32_table(gsx, case, resident):
    """SOG's codebooks are fitted without a fixed seed in the reference; the contract here: a table the writer takes gives the
    bytes its little-endian float32 twin gives, on both cores"""
    sw = _mod("formats.sog_writer")
    t = dc.table(case)
    np.random.seed(4)
    a = sw.encode(t, 8, device_resident=resident)
    np.random.seed(4)
    b = sw.encode(dc.f4le_equivalent(t), 8, device_resident=resident)
    assert sorted(a["textures"]) == sorted(b["textures"])
    for name in a["textures"]:
        np.testing.assert_array_equal(a["textures"][name], b["textures"][name], err_msg=name)
    for key in ("scale_codebook", "color_codebook", "shn_codebook", "shn_centroid_index", "mins", "maxs"):
        np.testing.assert_array_equal(np.asarray(a[key]), np.asarray(b[key]), err_msg=key)
    assert a["bands"] == b["bands"] == 3


@pytest.mark.parametrize("case", ["strided", "subset"])
def test_spz_and_ksplat_take_views_of_little_endian_tables(gsx, case, tmp_path):
    t = dc.table(case)
    twin = dc.f4le_equivalent(t)
    for mod, fn, ext in (("formats.spz_writer", "write_spz", "spz"), ("formats.ksplat_writer", "write_ksplat", "ksplat")):
        w = getattr(_mod(mod), fn)
        w(t, str(tmp_path / ("a." + ext)))
        w(twin, str(tmp_path / ("b." + ext)))
        assert (tmp_path / ("a." + ext)).read_bytes() == (tmp_path / ("b." + ext)).read_bytes(), mod
