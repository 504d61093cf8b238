"""-m gpu: the lazy DataProcessor on a table whose rows are in HBM (``resident=``) against the same processor without them:
the same ``.data`` bytes and dtype, the same printed lines, and ``processor.resident`` holds the rows of ``.data``.  Scenes of a
few thousand rows (tests/resident_cases.py: clusters, a haze the density filter removes, flyers for SOR).  A table the resident
path does not take (a float64 x) runs on the host and raises what it raises without the keyword."""
import contextlib
import importlib
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resident_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")
utils = importlib.import_module("3dgsconverter_amd.utils")


@pytest.fixture(scope="module")
def lib():
    lib = importlib.import_module("3dgsconverter_amd._lib")
    lib.require_hip()
    return lib


@pytest.fixture(scope="module")
def table():
    return rc.scene(6000, np.random.default_rng(0x636861696e))


FULL = (("crop_by_bbox", (-8.0, -8.0, -8.0, 8.0, 8.0, 8.0)), ("apply_alpha_filter", (40,)), ("apply_density_filter", (1.0, 0.32)),
        ("remove_flyers", (12, 1.5)), ("apply_auto_bbox", ()), ("add_rgb_from_sh", ()))
SEQUENCES = {
    "all_filters_then_rgb": FULL,
    "cap_sh_0": (("cap_sh_degree", (0,)),) + FULL,
    "cap_sh_1": (("cap_sh_degree", (1,)),) + FULL,
    "cap_sh_2_alone": (("cap_sh_degree", (2,)),),
    "cap_sh_2_then_filters": (("cap_sh_degree", (2,)), ("apply_alpha_filter", (40,)), ("remove_flyers", (12, 1.5))),
    "rgb_alone": (("add_rgb_from_sh", ()),),
    "rgb_then_a_filter": (("add_rgb_from_sh", ()), ("apply_alpha_filter", (40,)), ("add_rgb_from_sh", ())),
    "removes_everything": (("crop_by_bbox", (100.0, 100.0, 100.0, 101.0, 101.0, 101.0)), ("apply_auto_bbox", ())),
    "removes_everything_at_once": (("apply_alpha_filter", (255,)),),
    "removes_nothing": (("crop_by_bbox", (-1e9, -1e9, -1e9, 1e9, 1e9, 1e9)),),
    "no_call_at_all": (),
}


def run(make, steps):
    """-> (the processor, its .data, the printed lines, the exception's (type, text) or None)"""
    buf, exc = io.StringIO(), None
    saved, utils.DEBUG = utils.DEBUG, True               # (the [DEBUG] lines too)
    p = make()
    try:
        with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
            for name, args in steps:
                getattr(p, name)(*args)
            data = p.data
    except Exception as e:      # noqa: BLE001
        exc, data = (type(e).__name__, str(e)), None
    finally:
        utils.DEBUG = saved
    return p, data, buf.getvalue().split("\n"), exc


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_resident_rows_give_the_host_paths_table_and_lines(lib, table, name):
    steps = SEQUENCES[name]
    before = lib.ResidentRows.open_count
    host_p, want, want_lines, want_exc = run(lambda: dp.ChainedDataProcessor(table.copy()), steps)
    assert want_exc is None and host_p.resident is None
    src = table.copy()
    p, got, lines, exc = run(lambda: dp.ChainedDataProcessor(src, resident=lib.ResidentRows.from_host(src)), steps)
    try:
        assert exc is None
        assert got.dtype == want.dtype and len(got) == len(want)
        assert got.tobytes() == want.tobytes()
        assert lines == want_lines
        rr = p.resident
        if name == "removes_everything_at_once":        # `self.data = self.data[:0]` (data_processor.py:201): a host table from there on
            assert rr is None
        else:
            assert rr is not None and rr.n == len(got) and rr.dtype == got.dtype
            assert rr.download().tobytes() == got.tobytes()
            assert "take" in p.resident_ms
        if name in ("removes_nothing", "no_call_at_all"):
            assert got is src                             # the caller's table, and its rows
        if name == "removes_everything":
            assert len(got) == 0
        if name == "all_filters_then_rgb":
            assert 0 < len(got) < len(table) and got.dtype.names[-3:] == ("red", "green", "blue")
            assert {"gather", "take", "download"} <= set(p.resident_ms)
    finally:
        p.close()
        p.close()
    assert lib.ResidentRows.open_count == before


def test_every_filter_of_the_full_sequence_removes_rows(table):
    _, _, lines, _ = run(lambda: dp.ChainedDataProcessor(table.copy()), FULL)
    kept = [int(ln.lower().split("retained ")[1].split(" ")[0]) for ln in lines if "retained " in ln.lower()]
    assert len(kept) == 4 and kept[0] < len(table) and all(b < a for a, b in zip(kept, kept[1:])), lines


def test_a_table_with_a_float64_x_takes_the_host_path(lib, table):
    wide = np.zeros(len(table), np.dtype([(nm, "<f8" if nm == "x" else table.dtype[nm]) for nm in table.dtype.names]))
    for nm in table.dtype.names:
        wide[nm] = table[nm]
    wide["x"] += 1e-9                                      # values float32 does not hold
    before = lib.ResidentRows.open_count
    for steps in ((("apply_alpha_filter", (40,)), ("add_rgb_from_sh", ())), (("remove_flyers", (12, 1.5)),),
                  (("apply_density_filter", (1.0, 0.32)),)):
        _, want, want_lines, want_exc = run(lambda: dp.ChainedDataProcessor(wide.copy()), steps)
        src = wide.copy()
        rr = lib.ResidentRows.from_host(src)
        p, got, lines, exc = run(lambda: dp.ChainedDataProcessor(src, resident=rr), steps)
        assert rr.closed and p._rr is None                 # refused at once, and closed
        assert exc == want_exc and lines == want_lines
        if want_exc is None:
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
            assert p.resident is None
        else:
            assert want_exc[0] == "TypeError"
        p.close()
    assert lib.ResidentRows.open_count == before


def test_colours_that_do_not_fit_the_widened_row_come_back_to_the_host_path(lib):
    """510-byte rows are resident-eligible, 513 with red / green / blue are over RESIDENT_MAX_ROW_BYTES: the take is refused at
    ``.data``, the colours computed on the device come to the host, the resident rows are closed and the host path compacts"""
    dt = np.dtype([(nm, "<f4") for nm in ["x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity"] + ["f_rest_%d" % i for i in range(45)]]
                  + [("more_%d" % i, "<f4") for i in range(75)] + [("tail", "u1", (2,))])
    assert dt.itemsize == 510 and lib.resident_eligible(dt, 33, dt, 33)
    rng = np.random.default_rng(0x353130)
    table = np.zeros(33, dt)
    for nm in dt.names[:-1]:
        table[nm] = rng.standard_normal(33).astype(np.float32)
    table["opacity"] = np.linspace(-6, 6, 33, dtype=np.float32)[rng.permutation(33)]
    table["tail"] = rng.integers(0, 256, (33, 2), dtype=np.uint8)
    steps = (("apply_alpha_filter", (40,)), ("add_rgb_from_sh", ()))
    before = lib.ResidentRows.open_count
    host_p, want, want_lines, want_exc = run(lambda: dp.ChainedDataProcessor(table.copy()), steps)
    assert want_exc is None and 0 < len(want) < 33 and want.dtype.itemsize == 513
    src = table.copy()
    p, got, lines, exc = run(lambda: dp.ChainedDataProcessor(src, resident=lib.ResidentRows.from_host(src)), steps)
    try:
        assert exc is None
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
        assert lines == want_lines
        assert p.resident is None
    finally:
        p.close()
        host_p.close()
    assert lib.ResidentRows.open_count == before


def test_rows_of_another_table_are_refused(lib, table):
    other = lib.ResidentRows.from_host(table[:100].copy())
    p = dp.ChainedDataProcessor(table.copy(), resident=other)
    assert other.closed and p._rr is None
    eager = lib.ResidentRows.from_host(table.copy())
    p = dp.DataProcessor(table.copy(), lazy=False, resident=eager)
    assert eager.closed and p.resident is None
