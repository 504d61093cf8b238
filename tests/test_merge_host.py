"""-m "not gpu": the merge's host side, no device touched -- merge.merged_dtype and merge.remap_runs on mixes of the readers'
layouts, every refusal with its type and message, gsx_rows_remap_host (the statement of the kernel's contract) against the numpy
definition of tests/merge_numpy.py byte for byte with guard bytes around the written rows, every refusal of the entry point, and
the command line's pairing and validation messages."""
import importlib
import itertools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_cases as mc  # noqa: E402
import merge_numpy as mn  # noqa: E402
import ply_read_numpy as pn  # noqa: E402

merge = importlib.import_module("3dgsconverter_amd.merge")
lib = importlib.import_module("3dgsconverter_amd._lib")
GUARD = mc.GUARD


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


# ------------------------------------------------------------------------------------------------------------ the plan

MIXES = [names for r in (1, 2, 3) for names in itertools.combinations(mc.LAYOUTS, r)]


@pytest.mark.parametrize("names", MIXES, ids="+".join)
def test_merged_dtype_and_runs(names):
    dtypes = [mc.LAYOUTS[nm] for nm in names]
    got, notes = merge.merged_dtype(dtypes)
    want = mn.merged_dtype(dtypes)
    assert got == want and got.itemsize == 4 * (17 + mn.n_rest(want)) + (3 if "red" in want.names else 0) <= 251
    assert ("red" in got.names) == all(nm.startswith("spz") or nm == "cc" for nm in names)
    losers = []
    for k, dt in enumerate(dtypes):
        runs = merge.remap_runs(dt, got)
        assert mc.runs_cover_once(runs, dt.itemsize, got.itemsize), (names[k], runs)
        if dt == got:
            assert runs == [(0, 0, got.itemsize)]       # a source of the union's own dtype is one run of the whole row
        from_byte = {d + i: (s + i if s >= 0 else -1) for s, d, nb in runs for i in range(nb)}
        for nm, src in mn.name_map(dt, got).items():                # the runs are the name map, byte by byte
            at = got.fields[nm][1]
            want_bytes = [-1] * got[nm].itemsize if src is None else [dt.fields[src][1] + i for i in range(got[nm].itemsize)]
            assert [from_byte[at + i] for i in range(got[nm].itemsize)] == want_bytes, (names[k], nm)
        lost = [nm for nm in dt.names if nm not in got.names]
        if lost:
            losers.append(f"Merge: source {k} loses {len(lost)} field{'s' if len(lost) != 1 else ''} the union does not have: {', '.join(lost)}")
    assert notes == losers


def test_widening_indices():
    """9 -> 24, 9 -> 45 and 24 -> 45: channel c, coefficient k keeps its place in its channel"""
    for src, dst in ((1, 2), (1, 3), (2, 3)):
        s, d = mc.spz_dtype(src), mc.spz_dtype(dst)
        m, R = mn.n_rest(s) // 3, mn.n_rest(d) // 3
        runs = merge.remap_runs(s, d)
        from_byte = {dd + i: (ss + i if ss >= 0 else -1) for ss, dd, nb in runs for i in range(nb)}
        for c in range(3):
            for k in range(R):
                at = d.fields["f_rest_%d" % (c * R + k)][1]
                assert from_byte[at] == (s.fields["f_rest_%d" % (c * m + k)][1] if k < m else -1), (src, dst, c, k)
    # ... and the definition agrees on values: coefficient k of channel c lands in f_rest_(c R/3 + k)
    t = mc.table(mc.spz_dtype(1), 4)
    out = mn.merge_tables([t], mc.spz_dtype(3))
    assert out["f_rest_15"].tobytes() == t["f_rest_3"].tobytes() and out["f_rest_32"].tobytes() == t["f_rest_8"].tobytes()
    assert not out["f_rest_3"].view(np.uint32).any() and not out["f_rest_44"].view(np.uint32).any()


def test_notes_and_labels():
    got, notes = merge.merged_dtype([mc.LAYOUTS["std"], mc.LAYOUTS["cc"], mc.LAYOUTS["spz1"]], labels=["'a.ply'", "'b.ply'", "'c.spz'"])
    assert got == mc.standard_dtype()
    extras = ["scalar_label", "red", "green", "blue"] + ["scalar_extra_%d" % i for i in range(9)] + ["flag_%d" % i for i in range(5)]
    assert notes == ["Merge: 'b.ply' loses 18 fields the union does not have: " + ", ".join(extras),
                     "Merge: 'c.spz' loses 3 fields the union does not have: red, green, blue"]
    assert merge.merged_dtype([mc.LAYOUTS["spz1"], mc.LAYOUTS["spz0"]]) == (mc.spz_dtype(1), [])


def _without(dt, *drop):
    return np.dtype([(nm, dt[nm]) for nm in dt.names if nm not in drop])


def _retyped(dt, name, typ):
    return np.dtype([(nm, typ if nm == name else dt[nm]) for nm in dt.names])


def test_plan_refusals():
    std = mc.standard_dtype()
    for name in ("x", "f_dc_1", "opacity", "scale_2", "rot_0"):
        with pytest.raises(ValueError, match=f"merge: source 1 has no field '{name}'"):
            merge.merged_dtype([std, _without(std, name)])
    with pytest.raises(ValueError, match="merge: 'b.spz' has no field 'y'"):          # the FIRST missing one, and the label
        merge.merged_dtype([std, _without(std, "y", "rot_3")], labels=["'a.ply'", "'b.spz'"])
    for name, typ in (("z", "<f8"), ("nx", "<f2"), ("f_rest_7", ">f4"), ("rot_2", "<i4")):
        with pytest.raises(TypeError, match=f"merge: field '{name}' of source 0 is {np.dtype(typ).str}, and the merge copies '<f4' fields only"):
            merge.merged_dtype([_retyped(std, name, typ), std])
    partial = "f_rest fields of source 1 cannot be merged: whole bands of three colour channels are needed \\(0, 9, 24 or 45 fields named f_rest_0 ...\\)"
    for dt, count in ((_without(std, "f_rest_44"), 44), (_without(std, "f_rest_0"), 44), (_without(std, *["f_rest_%d" % i for i in range(12, 45)]), 12)):
        with pytest.raises(ValueError, match=f"merge: {count} " + partial):
            merge.merged_dtype([std, dt])
    # colours of another type are no colours: they are dropped, not refused
    got, notes = merge.merged_dtype([mc.spz_dtype(0), _retyped(mc.spz_dtype(0), "green", "<u2")])
    assert "red" not in got.names and len(notes) == 2
    with pytest.raises(ValueError, match="no source"):
        merge.merged_dtype([])
    with pytest.raises(ValueError, match="45 f_rest fields do not fit a union of 9"):
        merge.remap_runs(std, mc.spz_dtype(1))
    with pytest.raises(TypeError, match="field 'x' is <f8 in the source and <f4 in the union"):
        merge.remap_runs(_retyped(std, "x", "<f8"), std)


# ------------------------------------------------------------------------------------------------------------ gsx_rows_remap_host

def _remap_guarded(src_table, dst_dtype, dst_row0, dst_rows, src_first=0, dst_first=0):
    """gsx_rows_remap_host of `src_table` into rows [dst_row0, ...) of a guard-filled destination -> (its bytes, the row area)"""
    runs, n_runs = lib.remap_runs_array(merge.remap_runs(src_table.dtype, dst_dtype))
    si, so = src_table.dtype.itemsize, np.dtype(dst_dtype).itemsize
    src = mc.aligned_bytes(src_first + src_table.nbytes + 16, 0)
    src[src_first:src_first + src_table.nbytes] = src_table.view(np.uint8)
    dst = mc.aligned_bytes(dst_first + dst_rows * so + 16, 0)
    rc = lib.load().gsx_rows_remap_host(src.ctypes.data, src_first, si, len(src_table), runs, n_runs, dst.ctypes.data, dst_first, so, dst_row0, dst_rows)
    assert rc == 0, lib.last_error()
    return dst, dst[dst_first:dst_first + dst_rows * so]


@pytest.mark.parametrize("dst_stride", sorted(mc.DESTINATIONS))
@pytest.mark.parametrize("name", [nm for nm in mc.LAYOUTS])
def test_remap_host_is_the_definition(name, dst_stride):
    src_dtype, dst_dtype = mc.LAYOUTS[name], mc.DESTINATIONS[dst_stride]
    for n, dst_row0, first in ((0, 2, (0, 0)), (1, 0, (5, 3)), (129, 3, (0, 15)), (5000, 1, (15, 0)), (129, 0, (0, 0))):
        table = mc.table(src_dtype, n)
        rows = n + dst_row0 + 2
        whole, area = _remap_guarded(table, dst_dtype, dst_row0, rows, *first)
        want = np.full(rows * dst_stride, GUARD, np.uint8)
        want[dst_row0 * dst_stride:(dst_row0 + n) * dst_stride] = mn.merge_tables([table], dst_dtype).view(np.uint8)
        assert area.tobytes() == want.tobytes(), (name, n, dst_row0)
        assert (whole[:first[1]] == GUARD).all() and (whole[first[1] + rows * dst_stride:] == GUARD).all(), "bytes outside the table were written"


def test_remap_host_wrapper_and_unaligned_tables():
    """_lib.rows_remap_host takes tables wherever numpy put them (a view that starts at an odd byte too)"""
    a, b = mc.table(mc.LAYOUTS["spz1"], 40), mc.table(mc.LAYOUTS["cc"], 25)
    union = mn.merged_dtype([a.dtype, b.dtype])
    raw = np.full(65 * union.itemsize + 7, GUARD, np.uint8)
    out = raw[7:].view(union)
    odd = np.empty(a.nbytes + 3, np.uint8)
    odd[3:] = a.view(np.uint8)
    assert lib.rows_remap_host(odd[3:].view(a.dtype), merge.remap_runs(a.dtype, union), out, 0) is out
    lib.rows_remap_host(b, merge.remap_runs(b.dtype, union), out, 40)
    assert out.tobytes() == mn.merge_tables([a, b]).tobytes() and (raw[:7] == GUARD).all()
    with pytest.raises(ValueError, match="1-D C-contiguous"):
        lib.rows_remap_host(a[::2], merge.remap_runs(a.dtype, union), out, 0)
    with pytest.raises(lib.GsxError, match="gsx_rows_remap_host"):
        lib.rows_remap_host(b, merge.remap_runs(b.dtype, union), out, 41)
    big = np.dtype(a.dtype.descr + [("pad", "u1", 600)])            # rows over 512 bytes: the numpy field copy
    t = np.zeros(5, big)
    for nm in a.dtype.names:
        t[nm] = a[nm][:5]
    assert merge.remap_fields(t, np.zeros(9, union), 2)[2:7].tobytes() == mn.merge_tables([a[:5]], union).tobytes()


def test_remap_host_refusals_write_nothing():
    si, so = 107, 251
    src, dst = mc.aligned_bytes(20 * si + 32), mc.aligned_bytes(20 * so + 32)
    runs, n_runs = lib.remap_runs_array(merge.remap_runs(mc.spz_dtype(1), mc.spz_dtype(3)))
    L = lib.load()
    cases = mc.bad_remap_arguments(src.ctypes.data, dst.ctypes.data, runs)
    assert len(cases) >= 25
    for what, args in cases:
        assert L.gsx_rows_remap_host(*args) != 0, what
        assert lib.last_error().startswith("gsx_rows_remap_host: "), (what, lib.last_error())
    assert (dst == GUARD).all(), "a refused call wrote the destination"
    assert L.gsx_rows_remap_host(src.ctypes.data, 0, si, 0, runs, n_runs, dst.ctypes.data, 0, so, 20, 20) == 0     # n = 0: nothing to do
    assert (dst == GUARD).all()
    by_name = dict(cases)
    for what, said in (("a byte covered twice", "run 1 overlaps another at output byte 7"), ("a byte not covered", "output byte 8 belongs to no run")):
        assert L.gsx_rows_remap_host(*by_name[what]) != 0 and said in lib.last_error(), (what, lib.last_error())


# ------------------------------------------------------------------------------------------------------------ the command line

def _scene(path):
    t = pn.build(10, pn.canonical_fields(3), np.random.default_rng(3))
    pn.write_ply(str(path), [("vertex", t)])
    return str(path)


def test_merge_flags_parse(cli):
    a = cli.build_parser().parse_args(["-i", "a.ply", "-f", "spz", "--merge", "b.spz", "--merge", "c.splat", "--merge_rotate", "0", "90", "0",
                                       "--merge_rotate", "1", "2", "3", "--merge_scale", "2", "--merge_translate", "1", "0", "-0.5"])
    assert a.merge == ["b.spz", "c.splat"] and a.merge_rotate == [[0.0, 90.0, 0.0], [1.0, 2.0, 3.0]]
    assert a.merge_scale == [2.0] and a.merge_translate == [[1.0, 0.0, -0.5]]
    a = cli.build_parser().parse_args(["-i", "a.ply", "-f", "spz"])
    assert a.merge is None and a.merge_rotate is None and a.merge_scale is None and a.merge_translate is None


@pytest.mark.parametrize("flag,values", [("--merge_rotate", ["0", "90", "0"]), ("--merge_scale", ["2"]), ("--merge_translate", ["1", "2", "3"])])
@pytest.mark.parametrize("given,files", [(1, 2), (3, 2), (1, 0)])
def test_merge_pairing_error_returns_before_a_read(cli, no_reads, capsys, tmp_path, flag, values, given, files):
    a, b = _scene(tmp_path / "a.ply"), _scene(tmp_path / "b.ply")
    argv = ["-i", a, "-f", "spz"] + ["--merge", b] * files + ([flag] + values) * given
    assert cli.main(argv) is None
    assert capsys.readouterr().out.strip().split("\n") == [
        f"Error: {flag} was given {given} times for {files} --merge files (once per file, or not at all)."]


@pytest.mark.parametrize("value", ["0", "-2", "nan", "inf"])
def test_merge_scale_error_returns_before_a_read(cli, no_reads, capsys, tmp_path, value):
    a, b = _scene(tmp_path / "a.ply"), _scene(tmp_path / "b.ply")
    assert cli.main(["-i", a, "-f", "spz", "--merge", b, "--merge", b, "--merge_scale", "1.5", "--merge_scale=" + value]) is None
    assert capsys.readouterr().out.strip().split("\n") == [f"Error: --merge_scale must be a finite number greater than 0. Got {float(value)}."]


def test_missing_merge_file_is_reported_before_a_read(cli, no_reads, capsys, tmp_path):
    a, b = _scene(tmp_path / "a.ply"), _scene(tmp_path / "b.ply")
    gone = str(tmp_path / "nothing.spz")
    assert cli.main(["-i", a, "-f", "spz", "--merge", b, "--merge", gone]) is None
    assert capsys.readouterr().out.strip().split("\n") == [f"Error: --merge file '{gone}' does not exist."]


def test_merge_is_no_no_op_and_reaches_run(cli, capsys, tmp_path, monkeypatch):
    """.ply -> .ply 3dgs with only --merge is not stopped by the same-extension rule; run() receives the files and, per file, its
    own transform; without --merge it receives neither keyword"""
    a, b = _scene(tmp_path / "a.ply"), _scene(tmp_path / "b.ply")
    seen = {}
    monkeypatch.setattr(cli, "report_info", lambda *a, **k: None)
    monkeypatch.setattr(cli.Converter, "run", lambda self, **kw: seen.update(kw))
    cli.main(["-i", a, "-f", "3dgs", "--merge", b, "--merge", a, "--merge_translate", "1", "0", "0", "--merge_translate", "0", "1", "0"])
    out = capsys.readouterr().out
    assert "Operation aborted" not in out and "no filters are active" not in out
    assert seen["merge"] == [b, a]
    assert seen["merge_transforms"] == [{"rotate": None, "scale": None, "translate": [1.0, 0.0, 0.0]},
                                        {"rotate": None, "scale": None, "translate": [0.0, 1.0, 0.0]}]
    seen.clear()
    cli.main(["-i", a, "-f", "3dgs", "--merge", b])
    assert seen["merge"] == [b] and seen["merge_transforms"] is None
    seen.clear()
    cli.main(["-i", a, "-f", "spz"])
    assert seen and "merge" not in seen and "merge_transforms" not in seen
    cli.main(["-i", a, "-f", "3dgs"])               # ... and without --merge the no-op rule still holds
    assert "Operation aborted to prevent redundant processing." in capsys.readouterr().out


def test_info_is_unaffected_by_merge_flags(cli, capsys, tmp_path, monkeypatch):
    a = _scene(tmp_path / "a.ply")
    seen = []
    monkeypatch.setattr(cli, "report_info", lambda path, *r: seen.append(path))
    cli.main(["-i", a, "--info", "--merge", str(tmp_path / "nothing.spz"), "--merge_scale", "2", "--merge_scale", "3"])
    assert seen == [a] and capsys.readouterr().out == ""


def test_run_refuses_a_wrong_transform_count_and_an_unknown_file(conv, tmp_path, monkeypatch):
    a = _scene(tmp_path / "a.ply")
    junk = tmp_path / "junk.bin"
    junk.write_bytes(b"\0" * 64)
    table = mc.table(mc.standard_dtype(), 4)

    def read(self, path, stage_ms=None):
        self.profile = {"rest_nonzero": 0}
        return table
    monkeypatch.setattr(conv.SourceHandler, "read", read)
    c = conv.Converter(a, str(tmp_path / "o.spz"), "spz", resident=False)
    with pytest.raises(ValueError, match=re.escape("Could not detect source format of merge source '%s'" % junk)):
        c.run(merge=[str(junk)])
    with pytest.raises(ValueError, match="merge_transforms: one entry per merge source"):
        c.run(merge=[a], merge_transforms=[None, None])
