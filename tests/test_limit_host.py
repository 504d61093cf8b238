"""-m "not gpu": the splat budget's host side, no device touched -- gsx_limit_select_host (the select's digit walk and tie rule,
csrc/limit_select.h, run serially) against the numpy definition of tests/limit_numpy.py for every key case, size, budget and
a survivor list; the definition's two properties; the command line's flag; and limit_splats' refusals before any device work."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limit_cases as lc  # noqa: E402
import limit_numpy as ln  # noqa: E402
import ply_read_numpy as pn  # noqa: E402
import transform_cases as tc  # noqa: E402

lib = importlib.import_module("3dgsconverter_amd._lib")


@pytest.fixture(scope="module")
def cli():
    return importlib.import_module("3dgsconverter_amd.cli")


@pytest.fixture()
def no_reads(monkeypatch):
    """any load of a source fails the test"""
    conv = importlib.import_module("3dgsconverter_amd.converter")

    def refuse(self, path, stage_ms=None):
        raise AssertionError("the command line read %s" % path)
    monkeypatch.setattr(conv.SourceHandler, "read", refuse)


# ------------------------------------------------------------------------------------------------------------ the select

@pytest.mark.parametrize("n", lc.SIZES)
def test_host_select_is_the_definition(n):
    bad, runs = [], 0
    for name, keys in lc.key_cases(n).items():
        for N in lc.budgets(name, n):
            mask, info = lib.limit_select_host(keys, N)
            runs += 1
            assert mask.dtype == np.bool_ and mask.shape == (n,)
            T, ties, kept = ln.info(keys, N)
            if (int(mask.sum()) != min(N, n) or not np.array_equal(mask, ln.mask(keys, N))
                    or (info["threshold_key"], info["ties_kept"], info["kept"]) != (T, ties, kept)):
                bad.append((name, N, info, (T, ties, kept)))
    assert runs >= 7 * 3 or n < 3
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("n", lc.SIZES)
def test_host_select_reads_keys_through_a_survivor_list(n):
    """row j of the selected rows carries keys[orig[j]]: the definition on keys[orig]"""
    n0 = n + n // 2 + 3
    bad = []
    for name, keys in lc.key_cases(n0, seed=1).items():
        orig = lc.survivor_list(n0, n)
        sub = keys[orig]
        for N in lc.budgets("", n):
            mask, info = lib.limit_select_host(keys, N, orig=orig)
            if not np.array_equal(mask, ln.mask(sub, N)) or (info["threshold_key"], info["ties_kept"], info["kept"]) != ln.info(sub, N):
                bad.append((name, N, info))
    assert not bad, (len(bad), bad[:5])


def test_tie_block_cuts_inside_the_block():
    """the case the budgets of limit_cases are built for: the last row kept is row 2047, 2048, 2049 of the 21 equal keys"""
    keys = lc.key_cases(5000)["tie_block"]
    assert (keys[lc.TIE_FIRST:lc.TIE_LAST + 1] == lc.TIE_KEY).all() and np.count_nonzero(keys == lc.TIE_KEY) == 21
    assert np.count_nonzero(keys < lc.TIE_KEY) == lc.TIE_BELOW
    for last in (2047, 2048, 2049):
        N = lc.TIE_BELOW + last - lc.TIE_FIRST + 1
        assert N in lc.budgets("tie_block", 5000)
        mask, info = lib.limit_select_host(keys, N)
        block = mask[lc.TIE_FIRST:lc.TIE_LAST + 1]
        assert block[:last - lc.TIE_FIRST + 1].all() and not block[last - lc.TIE_FIRST + 1:].any()
        assert info["threshold_key"] == lc.TIE_KEY and info["ties_kept"] == last - lc.TIE_FIRST + 1 and info["kept"] == N


def test_host_select_refusals_and_no_rows():
    keys = np.arange(8, dtype=np.uint32)
    L = lib.load()
    import ctypes as C
    info = (C.c_uint32 * 3)(7, 7, 7)
    mask = np.full(8, 9, np.uint8)
    assert L.gsx_limit_select_host(keys.ctypes.data, None, 0, 3, mask.ctypes.data, info) == 0       # no rows: nothing written
    assert list(info) == [0, 0, 0] and (mask == 9).all()
    for args in ((None, None, 8, 3, mask.ctypes.data, info), (keys.ctypes.data, None, 8, 3, None, info), (keys.ctypes.data, None, -1, 3, mask.ctypes.data, info),
                 (keys.ctypes.data, None, 8, 0, mask.ctypes.data, info), (keys.ctypes.data, None, 8, -5, mask.ctypes.data, info),
                 (keys.ctypes.data, None, 8, 3, mask.ctypes.data, None), (keys.ctypes.data, None, 1 << 32, 3, mask.ctypes.data, info)):
        assert L.gsx_limit_select_host(*args) != 0, args[2:4]
        assert "gsx_limit_select_host" in lib.last_error()
    assert (mask == 9).all()
    mask, info = lib.limit_select_host(keys, 100)                                                    # a budget above n keeps every row
    assert mask.all() and info["kept"] == 8 and info["threshold_key"] == 7 and info["ties_kept"] == 1
    for bad in (0, -1, 2.5, True, "3", None):
        with pytest.raises(ValueError, match="at least 1"):
            lib.limit_count(bad)
    assert lib.limit_count(np.int64(4)) == 4


def test_threshold_is_the_metric_of_the_last_row_kept():
    t = lc.table(248, 1000)
    keys = ln.keys(t)
    m = ln.metric(t)
    for N in (1, 400, 970, 1000):
        mask, info = lib.limit_select_host(keys, N)
        last = np.argsort(keys, kind="stable")[N - 1]
        assert info["threshold_key"] == keys[last] and isinstance(info["threshold"], np.float32)
        if np.isnan(m[last]):
            assert np.isnan(info["threshold"])
        else:
            assert info["threshold"] == m[last] == -ln.sort_unkey(keys[last])


# ------------------------------------------------------------------------------------------------------------ the definition

def test_edge_table_holds_what_it_is_for():
    t = lc.table(248, 1000)
    m, k = ln.metric(t), ln.keys(t)
    tiny = np.finfo(np.float32).tiny
    assert np.isnan(m).sum() >= 3 and np.isposinf(m).sum() >= 1 and (m == 0).sum() >= 3 and ((m > 0) & (m < tiny)).sum() >= 2
    assert (k[np.isnan(m)] == lc.KEY_NAN).all() and (k[np.isposinf(m)] == lc.KEY_POS_INF_METRIC).all() and (k[m == 0] == 0x80000000).all()
    assert len(np.unique(k)) < len(k)                                   # equal keys among different rows: the tie rule matters
    order = np.argsort(k, kind="stable")
    assert np.isposinf(m[order[0]]) and np.isnan(m[order[-1]])          # an infinite metric is kept first, a NaN removed first


@pytest.mark.parametrize("n", (257, 5000))
def test_nesting(n):
    """(b): limit(N1) then limit(N2 <= N1) equals limit(N2)"""
    for name, keys in lc.key_cases(n).items():
        for N1 in (n - 1, n // 2, 3):
            first = np.nonzero(lib.limit_select_host(keys, N1)[0])[0].astype(np.uint32)
            for N2 in (N1, N1 // 2 + 1, 1):
                second = lib.limit_select_host(keys, N2, orig=first)[0]
                assert np.array_equal(first[second], ln.kept(keys, N2)), (name, N1, N2)


@pytest.mark.parametrize("n", (257, 5000))
def test_kept_rows_are_a_prefix_of_the_stable_order(n):
    """(a) at key level: the kept rows in stable key order are the first N of the full stable order -- what makes a budgeted
    .splat file the head of the unbudgeted one"""
    for name, keys in lc.key_cases(n).items():
        full = np.argsort(keys, kind="stable")
        for N in lc.budgets(name, n):
            rows = np.nonzero(lib.limit_select_host(keys, N)[0])[0]
            assert np.array_equal(rows[np.argsort(keys[rows], kind="stable")], full[:N]), (name, N)


def test_definition_is_the_splat_writers_metric():
    """with this process's numpy passing the exp probe, the definition's key is the key of the .splat writer's own metric"""
    if not lib.np_exp_probe():
        pytest.skip("this numpy's float32 exp is not the one csrc/np_exp.h reproduces: the writer's host metric differs by design")
    t = lc.table(248, 1000)
    with np.errstate(all="ignore"):
        want = ln.sort_key(-lib.splat_metric_host(t))
    assert np.array_equal(ln.keys(t), want)


# ------------------------------------------------------------------------------------------------------------ the processor

def test_limit_splats_refuses_before_any_device_work(monkeypatch, capsys):
    dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    monkeypatch.setattr(lib, "require_hip", lambda: (_ for _ in ()).throw(AssertionError("device work")))
    table = tc.table(248, 10)
    for lazy in (False, True):
        p = dp.DataProcessor(table.copy(), lazy=lazy)
        for bad in (0, -3, 2.5, "4", None, True):
            with pytest.raises(ValueError, match="at least 1"):
                p.limit_splats(bad)
        wide = dp.DataProcessor(table.astype(np.dtype([(nm, "<f8" if nm == "opacity" else "<f4") for nm in table.dtype.names])), lazy=lazy)
        with pytest.raises(TypeError, match="field 'opacity' is <f8"):
            wide.limit_splats(5)
        swapped = dp.DataProcessor(table.astype(np.dtype([(nm, ">f4" if nm == "scale_2" else "<f4") for nm in table.dtype.names])), lazy=lazy)
        with pytest.raises(TypeError, match="field 'scale_2' is >f4"):
            swapped.limit_splats(5)
        capsys.readouterr()
        bare = dp.DataProcessor(np.ascontiguousarray(table[[nm for nm in table.dtype.names if nm != "scale_1"]]), lazy=lazy)
        before = bare.data.tobytes()
        out = bare.limit_splats(5)
        assert capsys.readouterr().out.strip() == "Warning: Splat limit needs scale_0..2 and opacity. Limit skipped."
        assert ((out is None) if lazy else (out is bare.data)) and bare.data.tobytes() == before
        for N in (10, 11, 10 ** 9):                                     # a budget the table meets already: no device work
            out = p.limit_splats(N)
            assert capsys.readouterr().out.strip() == f"Splat Limit (max {N}): 10 splats, nothing to remove."
            assert ((out is None) if lazy else (out is p.data)) and p.data.tobytes() == table.tobytes()
        empty = dp.DataProcessor(table[:0].copy(), lazy=lazy)
        empty.limit_splats(1)
        assert capsys.readouterr().out.strip() == "Splat Limit (max 1): 0 splats, nothing to remove." and len(empty.data) == 0
    with pytest.raises(AssertionError, match="device work"):            # ... and a budget below the row count does reach the device
        dp.DataProcessor(table.copy(), lazy=True).limit_splats(5)
    with pytest.raises(TypeError, match="structured array"):
        dp.DataProcessor([1, 2, 3]).limit_splats(2)


# ------------------------------------------------------------------------------------------------------------ the command line

def _scene(path):
    t = pn.build(10, pn.canonical_fields(3), np.random.default_rng(3))
    pn.write_ply(str(path), [("vertex", t)])
    return str(path)


def test_flag_parses(cli):
    a = cli.build_parser().parse_args(["-i", "a.ply", "-f", "spz", "--max_splats", "1500000"])
    assert a.max_splats == 1500000
    assert cli.build_parser().parse_args(["-i", "a.ply", "-f", "spz"]).max_splats is None
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["-i", "a.ply", "-f", "spz", "--max_splats", "1.5"])


@pytest.mark.parametrize("value", [0, -3])
def test_budget_error_returns_before_a_read(cli, no_reads, capsys, tmp_path, value):
    assert cli.main(["-i", _scene(tmp_path / "a.ply"), "-f", "spz", "--max_splats=%d" % value]) is None
    assert capsys.readouterr().out.strip().split("\n") == [f"Error: --max_splats must be at least 1. Got {value}."]


def test_a_budget_is_no_no_op(cli, capsys, tmp_path, monkeypatch):
    """.ply -> .ply 3dgs with only --max_splats is not stopped by the same-extension rule, and the budget reaches run()"""
    src = _scene(tmp_path / "a.ply")
    seen = {}
    monkeypatch.setattr(cli, "report_info", lambda *a, **k: None)
    monkeypatch.setattr(cli.Converter, "run", lambda self, **kw: seen.update(kw))
    cli.main(["-i", src, "-f", "3dgs", "--max_splats", "5"])
    out = capsys.readouterr().out
    assert "Operation aborted" not in out and "no filters are active" not in out
    assert seen["max_splats"] == 5
    seen.clear()
    cli.main(["-i", src, "-f", "spz"])                  # without the flag run() is told so
    assert seen["max_splats"] is None
    cli.main(["-i", src, "-f", "3dgs"])                 # ... and the same-extension run without a filter is still stopped
    assert "Operation aborted to prevent redundant processing." in capsys.readouterr().out
