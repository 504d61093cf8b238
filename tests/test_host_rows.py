"""-m "not gpu": the threaded host row operations of the C ABI (gsx_host_gather_f32, gsx_host_compact_rows)
against the numpy expressions of the reference they replace (data_processor.py:38,139 column_stack;
:114,149 vertices[mask]).  Byte-exact."""
import importlib

import numpy as np
import pytest

gsx = importlib.import_module("3dgsconverter_amd")
L = gsx._lib


def _table(n, with_rgb=False, seed=0):
    names = ["x", "y", "z", "nx", "ny", "nz"] + ["f_dc_%d" % i for i in range(3)] + ["f_rest_%d" % i for i in range(45)] \
        + ["opacity"] + ["scale_%d" % i for i in range(3)] + ["rot_%d" % i for i in range(4)]
    fields = [(nm, "<f4") for nm in names]
    if with_rgb:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]  # 251-byte rows: nothing is aligned
    dt = np.dtype(fields)
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 255, size=(n, dt.itemsize), dtype=np.uint8)
    raw[:, 3::4] &= 0x3F  # keep the float fields finite (exponent < 255)
    return raw.reshape(-1).view(dt)


@pytest.mark.parametrize("n", [0, 1, 7, 1000, 300_001])
@pytest.mark.parametrize("with_rgb", [False, True])
def test_gather_equals_column_stack(n, with_rgb):
    v = _table(n, with_rgb, seed=n)
    got = L.host_gather_xyz(v)
    ref = np.column_stack((v["x"], v["y"], v["z"]))
    assert got.dtype == np.float32 and got.shape == (n, 3) and got.flags.c_contiguous
    assert got.tobytes() == ref.tobytes()


def test_gather_other_layouts_go_through_numpy():
    v = _table(1000)[::2]  # not contiguous
    assert L.host_gather_xyz(v).tobytes() == np.column_stack((v["x"], v["y"], v["z"])).tobytes()
    dt = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8")])
    w = np.zeros(10, dt)
    w["x"] = np.arange(10)
    assert L.host_gather_xyz(w).dtype == np.float32 and (L.host_gather_xyz(w)[:, 0] == np.arange(10)).all()


@pytest.mark.parametrize("n,p", [(0, 0.5), (1, 1.0), (1, 0.0), (1000, 0.5), (300_001, 0.85), (300_001, 0.0), (300_001, 1.0),
                                 (2_000_003, 0.03)])
@pytest.mark.parametrize("with_rgb", [False, True])
def test_compaction_equals_boolean_indexing(n, p, with_rgb):
    v = _table(min(n, 300_001), with_rgb, seed=n)
    if n > len(v):
        v = np.resize(v, n)
    mask = np.random.default_rng(n + 1).random(n) < p
    got = L.host_compact_rows(v, mask)
    ref = v[mask]
    assert got.dtype == v.dtype and got.shape == ref.shape
    assert got.tobytes() == ref.tobytes()
    assert got.base is None or got.base is not v  # a new array, like numpy's


def test_compaction_runs_and_plain_dtypes():
    a = np.arange(100_000, dtype=np.int64)
    mask = np.zeros(len(a), bool)
    mask[10:5000] = True
    mask[-3:] = True
    mask[50_000] = True
    np.testing.assert_array_equal(L.host_compact_rows(a, mask), a[mask])
    b = np.arange(12, dtype=np.float32).reshape(4, 3)  # not 1-D: numpy semantics
    np.testing.assert_array_equal(L.host_compact_rows(b, np.array([1, 0, 1, 1], bool)), b[np.array([1, 0, 1, 1], bool)])


def test_c_abi_rejects_bad_arguments():
    lib = L.load()
    import ctypes as C
    n_out = C.c_int64()
    rows = np.zeros(16, np.uint8)
    mask = np.ones(4, np.uint8)
    out = np.zeros(8, np.uint8)
    assert lib.gsx_host_compact_rows(rows.ctypes.data, 4, 4, mask.ctypes.data, out.ctypes.data, 2, C.byref(n_out)) != 0
    assert b"do not fit" in lib.gsx_last_error()
    offs = (C.c_int64 * 1)(2)
    assert lib.gsx_host_gather_f32(rows.ctypes.data, 4, 4, offs, 1, out.ctypes.data) != 0
    assert b"outside the row" in lib.gsx_last_error()


def test_alpha_and_bbox_filters_match_the_reference_expressions():
    """DataProcessor.apply_alpha_filter / crop_by_bbox (reference data_processor.py:184-231): same masks,
    threaded compaction"""
    dp = importlib.import_module("3dgsconverter_amd.processing")
    v = _table(50_000, seed=3)
    rng = np.random.default_rng(4)
    v["opacity"] = rng.normal(0, 3, len(v)).astype(np.float32)
    for nm in "xyz":
        v[nm] = rng.normal(0, 2, len(v)).astype(np.float32)
    for limit in (1, 13, 128, 254):
        a = np.clip(limit / 255.0, 1e-6, 1.0 - 1e-6)
        ref = v[v["opacity"] >= np.log(a / (1.0 - a))]
        p = dp.DataProcessor(v)
        out = p.apply_alpha_filter(limit)
        assert out is p.data and out.tobytes() == ref.tobytes()
    p = dp.DataProcessor(v)
    assert p.apply_alpha_filter(0) is None and p.data is v
    p.apply_alpha_filter(255)
    assert len(p.data) == 0 and p.data.dtype == v.dtype
    box = (-1.0, -2.0, -0.5, 1.5, 2.0, 3.0)
    ref = v[(v["x"] >= box[0]) & (v["x"] <= box[3]) & (v["y"] >= box[1]) & (v["y"] <= box[4]) &
            (v["z"] >= box[2]) & (v["z"] <= box[5])]
    p = dp.DataProcessor(v)
    assert p.crop_by_bbox(*box).tobytes() == ref.tobytes() and 0 < len(ref) < len(v)
    w = np.zeros(5, np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4")]))
    p = dp.DataProcessor(w)
    assert p.apply_alpha_filter(10) is None and p.data is w  # no opacity channel: skipped with a warning


def test_zero_columns_and_append_columns_equal_numpy(gsx):
    """the host halves of cap_sh_degree (data_processor.py:310-313) and add_rgb_from_sh (:262-274): same bytes as numpy's
    field-by-field version, on the reference's 248-byte table, a table with trailing u1 fields, and tiny / empty inputs"""
    L = gsx._lib
    from oracle import datasets
    for n in (0, 1, 7, 50_001):
        a = datasets.sog_scene(n, 1) if n else np.zeros(0, dtype=datasets.splat_dtype(3))
        b = a.copy()
        names = ["f_rest_%d" % i for i in range(9, 45)] + ["not_a_field"]
        L.host_zero_columns(a, names)
        for nm in names[:-1]:
            b[nm] = 0.0
        assert a.tobytes() == b.tobytes()
        cols = np.random.default_rng(n).integers(0, 256, (n, 3)).astype(np.uint8)
        for base in (a, L.host_append_u8_columns(a, ("u", "v", "w"), cols)):      # second round: itemsize 251 -> 254
            w = L.host_append_u8_columns(base, ("red", "green", "blue"), cols)
            want = np.empty(n, dtype=base.dtype.descr + [("red", "u1"), ("green", "u1"), ("blue", "u1")])
            for nm in base.dtype.names:
                want[nm] = base[nm]
            want["red"], want["green"], want["blue"] = cols[:, 0], cols[:, 1], cols[:, 2]
            assert w.dtype == want.dtype and w.tobytes() == want.tobytes()
    # scattered (non-adjacent) columns and a read-only view fall back to numpy's own assignment
    a = datasets.sog_scene(100, 2)
    b = a.copy()
    L.host_zero_columns(a, ["x", "f_rest_3", "rot_3"])
    b["x"] = 0.0
    b["f_rest_3"] = 0.0
    b["rot_3"] = 0.0
    assert a.tobytes() == b.tobytes()


def test_lazy_cap_sh_degree_belongs_to_the_table_it_was_called_on():
    """a deferred cap_sh_degree followed by `processor.data = other` must zero the ORIGINAL table (the
    reference zeroes it at once, data_processor.py:313) and leave `other` alone"""
    import importlib
    dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    dt = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4")] + [("f_rest_%d" % i, "f4") for i in range(45)])
    a, b = np.ones(50, dtype=dt), np.ones(30, dtype=dt)
    for name in dt.names:
        a[name], b[name] = 1.0, 2.0
    proc = dp.DataProcessor(a, lazy=True)
    assert proc.cap_sh_degree(1) is None and float(a["f_rest_9"].sum()) == 50.0      # deferred: nothing written yet
    proc.data = b
    assert float(a["f_rest_9"].sum()) == 0.0 and float(a["f_rest_44"].sum()) == 0.0 and float(a["f_rest_8"].sum()) == 50.0
    assert proc.data is b and float(b["f_rest_9"].sum()) == 60.0                     # the new table is untouched


def test_lazy_cap_sh_degree_with_a_pending_compaction_leaves_the_callers_array_alone():
    """filters pending in the chain + a deferred cap_sh_degree + `processor.data = other`: the reference had
    replaced self.data with the filtered COPY before it zeroed anything, so the caller's original array stays untouched"""
    import importlib
    dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    dt = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4")] + [("f_rest_%d" % i, "f4") for i in range(45)])
    a, b = np.ones(50, dtype=dt), np.ones(30, dtype=dt)
    for name in dt.names:
        a[name], b[name] = 1.0, 2.0

    class Chain:   # what a DeviceChain looks like after a filter removed rows (no GPU needed for the setter's decision)
        n0, n, closed = 50, 20, False

        def close(self):
            self.closed = True

    proc = dp.DataProcessor(a, lazy=True)
    proc._chain = ch = Chain()
    assert proc.cap_sh_degree(1) is None
    proc.data = b
    assert ch.closed and float(a["f_rest_9"].sum()) == 50.0 and float(a["f_rest_44"].sum()) == 50.0
    assert proc.data is b and float(b["f_rest_9"].sum()) == 60.0


def test_take_rows_by_the_survivor_list_is_boolean_indexing():
    """round 5: gsx_host_take_rows (the device chain's ascending survivor list applied to the host table without a boolean
    mask in between) == rows[mask] byte for byte; empty list, every row, a ragged structured dtype, and a list that is not
    ascending is refused"""
    import importlib
    L = importlib.import_module("3dgsconverter_amd")._lib
    rng = np.random.default_rng(9)
    dt = np.dtype([("x", "f4"), ("k", "i8"), ("b", "u1", (3,)), ("y", "f4")])
    t = np.zeros(123457, dtype=dt)
    t["x"], t["k"], t["y"] = rng.random(len(t)), np.arange(len(t)), rng.random(len(t))
    t["b"] = rng.integers(0, 255, (len(t), 3))
    for frac in (0.0, 0.03, 0.8, 1.0):
        mask = rng.random(len(t)) < frac
        idx = np.flatnonzero(mask).astype(np.uint32)
        got = L.host_take_rows(t, idx)
        assert got.dtype == t.dtype and got.tobytes() == t[mask].tobytes()
    with pytest.raises(L.GsxError):
        L.host_take_rows(t, np.array([7, 7], dtype=np.uint32))
    with pytest.raises(L.GsxError):
        L.host_take_rows(t, np.array([1, len(t)], dtype=np.uint32))


def test_take_rows_and_append_columns_in_one_pass():
    """round 6: gsx_host_take_rows_append == the reference's two steps -- `vertices[mask]` (data_processor.py:114,149), then the
    widened copy of add_rgb_from_sh (:262-274) with the colours of the surviving rows -- byte for byte; no survivors, every row,
    bad index lists refused"""
    rng = np.random.default_rng(12)
    for n in (1, 9, 100_003):
        t = _table(n, False, seed=n)
        cols = rng.integers(0, 256, (n, 3), dtype=np.uint8)
        for frac in (0.0, 0.4, 1.0):
            mask = rng.random(n) < frac
            idx = np.flatnonzero(mask).astype(np.uint32)
            got = L.host_take_rows_append_u8(t, idx, ("red", "green", "blue"), cols)
            kept = t[mask]
            want = np.empty(len(kept), dtype=np.dtype(t.dtype.descr + [("red", "u1"), ("green", "u1"), ("blue", "u1")]))
            for nm in t.dtype.names:
                want[nm] = kept[nm]
            for i, nm in enumerate(("red", "green", "blue")):
                want[nm] = cols[mask, i]
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    with pytest.raises(L.GsxError):
        L.host_take_rows_append_u8(t, np.array([5, 5], dtype=np.uint32), ("red", "green", "blue"), cols)
    with pytest.raises(L.GsxError):
        L.host_take_rows_append_u8(t, np.array([0, n], dtype=np.uint32), ("red", "green", "blue"), cols)


def test_take_rows_shape_is_compaction_then_sh_cap_then_colours():
    """round 6: gsx_host_take_rows_shape == `vertices[mask]` (data_processor.py:114,149), `data[f_rest_i] = 0.0` for the capped columns
    (:310-313) and the widened copy with the survivors' colours (:262-274), in one pass -- with and without colours, with and
    without zeroed columns; a table the C routine does not take (strided view) goes through the separate steps"""
    rng = np.random.default_rng(21)
    n = 60_001
    t = _table(n, False, seed=5)
    cols = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    zero_sets = ([], ["f_rest_%d" % i for i in range(9, 45)], ["f_rest_3", "f_rest_4", "f_rest_40", "opacity"])
    for frac in (0.0, 0.5, 1.0):
        mask = rng.random(n) < frac
        idx = np.flatnonzero(mask).astype(np.uint32)
        for zero in zero_sets:
            for with_rgb in (False, True):
                got = L.host_take_rows_shape(t, idx, ("red", "green", "blue") if with_rgb else (), cols if with_rgb else None, zero)
                kept = t[mask]
                for nm in zero:
                    kept[nm] = 0.0
                if with_rgb:
                    want = np.empty(len(kept), dtype=np.dtype(t.dtype.descr + [("red", "u1"), ("green", "u1"), ("blue", "u1")]))
                    for nm in t.dtype.names:
                        want[nm] = kept[nm]
                    for i, nm in enumerate(("red", "green", "blue")):
                        want[nm] = cols[mask, i]
                else:
                    want = kept
                assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (frac, len(zero), with_rgb)
    view = t[::2]
    idx = np.arange(0, len(view), 3, dtype=np.uint32)
    got = L.host_take_rows_shape(view, idx, (), None, ["f_rest_7"])
    want = view[idx]
    want["f_rest_7"] = 0.0
    assert got.tobytes() == want.tobytes()


def test_row_filters_and_sh_cap_against_the_reference_class_on_random_sequences():
    """random sequences of crop_by_bbox / apply_alpha_filter / cap_sh_degree / apply_auto_bbox (the methods of the eager
    drop-in class that need no device) against what the REFERENCE's own class made of the same tables
    (tests/golden/row_filters_ref.json, oracle/make_golden_rows.py) -- bounds as Python floats, ints, numpy float32 /
    float64 scalars, coordinates with NaN and +-inf, thresholds at both ends.  Round 6 moved these methods onto contiguous
    copies of the columns (one threaded gather): the expressions must keep numpy's promotion rules.  Same bytes, same
    printed box."""
    import json
    import os
    from oracle import make_golden_rows as mgr
    with open(os.path.join(os.path.dirname(__file__), "golden", "row_filters_ref.json")) as f:
        gold = json.load(f)
    dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    all_cases = mgr.cases()
    assert len(all_cases) == gold["_meta"]["cases"]
    for case, t, steps in all_cases:
        got, want = mgr.run(dp.DataProcessor, t, steps), gold[str(case)]
        assert got["dtype"] == want["dtype"] and got["sha256"] == want["sha256"], (case, steps)
        assert got["log"] == want["log"], (case, steps, got["log"], want["log"])
