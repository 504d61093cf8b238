"""-m "not gpu": gsx_table_profile_host, the host twin of the table-profile kernel and the product path for a table that is not
resident -- against numpy's `np.any(col != 0)`, `np.min` and `np.max` on every case of tests/profile_cases.py, with one thread
and with seven, the layouts it refuses, and the paths of host_table_profile that go round it (an empty table, fields that are
not '<f4', rows wider than 512 bytes)."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import profile_cases as pc  # noqa: E402

CASES = pc.cases()


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgsconverter_amd._lib")


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_host_profile_is_numpys(lib, case):
    want = pc.expected(case.table)
    one = lib.host_table_profile(case.table, threads=1)
    seven = lib.host_table_profile(case.table, threads=7)
    auto = lib.host_table_profile(case.table)
    assert pc.same(one, want), (one, want)
    for other in (seven, auto):
        assert pc.same(other, want), (other, want)
        assert other["rest_nonzero"] == one["rest_nonzero"] and other["nan_axes"] == one["nan_axes"]
        for a in range(3):
            if not (want["nan_axes"] >> a) & 1:                     # the same bits, a zero's sign included
                assert np.float32(other["lo"][a]).tobytes() == np.float32(one["lo"][a]).tobytes()
                assert np.float32(other["hi"][a]).tobytes() == np.float32(one["hi"][a]).tobytes()


def test_cases_cover_what_they_claim():
    by = {c.name: c for c in CASES}
    assert {c.table.dtype.itemsize for c in CASES} >= set(pc.ROW_BYTES)
    assert {len(c.table) for c in CASES} >= set(pc.NS)
    want = pc.expected(by["denormal_nan_negzero"].table)
    assert want["rest_nonzero"] == (1 << 3) | (1 << 17) | (1 << 30)      # denormals and the NaN count, -0.0 does not
    want = pc.expected(by["inf_x_nan_y"].table)
    assert want["lo"][0] == -np.inf and want["hi"][0] == np.inf and want["nan_axes"] == 0b010
    assert pc.expected(by["single_last_rb512_n1000"].table)["rest_nonzero"] == (1 << 44) | 1
    assert pc.expected(by["axes_none_rest45"].table)["lo"] == (np.inf,) * 3


def test_refused_layouts(lib):
    rows = np.zeros(4 * 513, np.uint8)
    for name, lay in pc.refused_layouts(lib):
        res = lib.TableProfile()
        rc = lib.load().gsx_table_profile_host(rows.ctypes.data, 4, C.byref(lay), 1, C.byref(res))
        assert rc != 0, name
        assert "gsx_table_profile_host" in lib.last_error() and "byte" in lib.last_error(), lib.last_error()
    lay, _ = lib.profile_layout(pc.table_dtype(248, 45))
    res = lib.TableProfile()
    assert lib.load().gsx_table_profile_host(rows.ctypes.data, 0, C.byref(lay), 1, C.byref(res)) != 0     # n >= 1
    assert lib.load().gsx_table_profile_host(None, 4, C.byref(lay), 1, C.byref(res)) != 0


def test_struct_sizes_match_the_header(lib):
    assert C.sizeof(lib.ProfileLayout) == 8 + 4 * 48 and C.sizeof(lib.TableProfile) == 48


def test_tables_the_pass_does_not_take(lib):
    """an empty table, a field of another type, rows over 512 bytes, a strided view: the reference's numpy expressions"""
    assert lib.host_table_profile(np.zeros(0, pc.table_dtype(248, 45)))["n"] == 0
    rng = np.random.default_rng(5)
    dt = np.dtype([("x", "<f8"), ("y", "<f4"), ("z", ">f4"), ("f_rest_0", "<f4"), ("f_rest_1", "<f8"), ("f_rest_2", "<f2")])
    t = np.zeros(100, dt)
    for nm in ("x", "y", "z"):
        t[nm] = rng.normal(size=100)
    t["f_rest_1"][99] = 1e-300
    layout, foreign = lib.profile_layout(dt)
    assert foreign == ["x", "z", "f_rest_1", "f_rest_2"] and layout.xyz_offset[0] == -1 and layout.xyz_offset[1] == 8
    got = lib.host_table_profile(t)
    assert got["rest_nonzero"] == 0b010 and got["n"] == 100
    for a, nm in enumerate(pc.AXES):
        assert got["lo"][a] == float(np.min(t[nm])) and got["hi"][a] == float(np.max(t[nm]))
    wide = pc.blank(50, np.dtype({"names": ["x", "y", "z", "f_rest_0"], "formats": ["<f4"] * 4, "offsets": [0, 4, 8, 600], "itemsize": 604}), 9)
    wide["f_rest_0"][49] = 3.0
    assert pc.same(lib.host_table_profile(wide), pc.expected(wide))
    strided = pc.blank(64, pc.table_dtype(68, 9), 11)[::2]
    assert pc.same(lib.host_table_profile(strided), pc.expected(strided))
