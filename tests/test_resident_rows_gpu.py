"""-m gpu: a reader's rows kept in HBM (csrc/resident_rows.hip, _lib.ResidentRows, the readers' ``keep=``).

gsx_rows_columns_f32_dev against numpy's field views of the same random bytes and gsx_rows_take_dev against its host twin
_lib.host_take_rows_shape, byte for byte, at every stride, row count and first byte of tests/resident_cases.py; the colours of
resident rows -- columns, gsx_rgb_from_sh_list_dev, gsx_dev_patch_u8 -- against DataProcessor._compute_rgb_from_sh on the host
table, with planted values numpy's own power decides; every reader's ``keep=``; and the lifetime of what was kept."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cply_read_numpy as cn  # noqa: E402
import ksplat_read_numpy as kn  # noqa: E402
import parquet_numpy as qn  # noqa: E402
import ply_read_numpy as pn  # noqa: E402
import profile_cases as pc  # noqa: E402
import resident_cases as rc  # noqa: E402
import sog_read_numpy as gn  # noqa: E402
import splat_read_numpy as sn  # noqa: E402
import spz_read_numpy as zn  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 0xA5


@pytest.fixture(scope="module")
def lib():
    lib = importlib.import_module("3dgsconverter_amd._lib")
    lib.require_hip()
    return lib


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


def _upload_rows(ctx, raw, first_byte):
    """the rows' bytes from byte `first_byte` of a device buffer, 0xff before them and in the 16 bytes behind them"""
    buf = np.full(first_byte + raw.size + 16, 0xff, np.uint8)
    buf[first_byte:first_byte + raw.size] = raw.reshape(-1)
    return ctx.alloc(buf.nbytes).upload(buf)


def _guarded(ctx, nbytes):
    """a device buffer of `nbytes` bytes and 64 guard bytes behind them, all GUARD"""
    return ctx.alloc(nbytes + 64).upload(np.full(nbytes + 64, GUARD, np.uint8))


def _take_back(d, nbytes):
    """-> the first `nbytes` bytes; the guard behind them must be untouched (nothing is written past the output, so no slack
    behind it is ever needed, and none is read here)"""
    got = d.download(np.uint8, nbytes + 64)
    assert (got[nbytes:] == GUARD).all(), "bytes behind the output were written"
    return got[:nbytes]


# ------------------------------------------------------------------------------------------------------------ columns

@pytest.mark.parametrize("stride", rc.STRIDES)
def test_columns_are_numpys_field_views(lib, ctx, stride):
    rng = np.random.default_rng(stride)
    bad = []
    for n in rc.COUNTS:
        raw = rc.raw_rows(n, stride, rng)
        for first_byte in rc.FIRST_BYTES:
            d = _upload_rows(ctx, raw, first_byte)
            try:
                for m in (1, 3, 4):
                    offs = rc.column_offsets(stride, m)
                    want = np.stack([rc.field_view(raw, o) for o in offs], axis=1)
                    d_out = _guarded(ctx, 4 * n * m)
                    try:
                        arr = (C.c_int32 * m)(*offs)
                        lib.check(lib.load().gsx_rows_columns_f32_dev(ctx.handle, d.ptr, first_byte, stride, n, arr, m, d_out.ptr), "columns")
                        ctx.synchronize()
                        got = _take_back(d_out, 4 * n * m).view(np.uint32).reshape(n, m)
                    finally:
                        d_out.free()
                    if not np.array_equal(got, want):
                        bad.append((n, first_byte, m, offs))
            finally:
                d.free()
    assert not bad, bad[:5]


def test_columns_refusals(lib, ctx):
    d = ctx.alloc(4096)
    try:
        L = lib.load()
        one = (C.c_int32 * 4)(0, 4, 8, 12)
        for args in ((d.ptr, 0, 0, 4, one, 1), (d.ptr, 0, 513, 4, one, 1), (d.ptr, 16, 16, 4, one, 1), (d.ptr + 4, 0, 16, 4, one, 1),
                     (d.ptr, 0, 16, 4, one, 0), (d.ptr, 0, 16, 4, one, 5), (d.ptr, 0, 12, 4, one, 4), (d.ptr, 0, 16, -1, one, 1)):
            assert L.gsx_rows_columns_f32_dev(ctx.handle, *args, d.ptr + 2048) != 0, args[1:4]
            assert "gsx_rows_columns_f32_dev" in lib.last_error()
        assert L.gsx_rows_columns_f32_dev(ctx.handle, d.ptr, 0, 16, 4, one, 1, d.ptr + 2052) != 0      # the output's alignment
    finally:
        d.free()


# ------------------------------------------------------------------------------------------------------------ take

@pytest.mark.parametrize("stride", rc.STRIDES)
def test_take_is_the_host_twins_bytes(lib, ctx, stride):
    rng = np.random.default_rng(1000 + stride)
    bad, launches = [], 0
    for n in rc.COUNTS:
        for first_byte, phase in ((0, 0), (5, min(3, stride - 1) if stride % 4 else 1)):
            dt = rc.packed_dtype(stride, phase)
            table = rc.raw_rows(n, stride, rng).reshape(-1).view(dt)
            colours = rng.integers(0, 256, (n, 3), dtype=np.uint8)
            d = _upload_rows(ctx, table.view(np.uint8), first_byte)
            d_extra = ctx.alloc(3 * n + 16).upload(colours)
            d_idx = ctx.alloc(4 * n + 16)
            try:
                for e in (0, 3):
                    for name, idx in rc.index_lists(n, rc.take_tile_rows(stride + e)).items():
                        for nz in (0, 21, 45):
                            zero = rc.zero_names(dt, nz, rng)
                            full = np.arange(n, dtype=np.uint32) if idx is None else idx
                            want = lib.host_take_rows_shape(table, full, ("red", "green", "blue") if e else (), colours if e else None, zero)
                            assert want.dtype.itemsize == stride + e
                            if idx is not None and len(idx):
                                d_idx.upload(idx)
                            d_out = _guarded(ctx, want.nbytes)
                            try:
                                lib.rows_take_dev(ctx, d.ptr, first_byte, stride, n, None if idx is None else d_idx.ptr, len(full),
                                                  [dt.fields[nm][1] for nm in zero], d_extra.ptr if e else None, e, d_out.ptr)
                                got = _take_back(d_out, want.nbytes)
                            finally:
                                d_out.free()
                            launches += 1
                            if got.tobytes() != want.tobytes():
                                bad.append((n, first_byte, e, name, nz))
            finally:
                for b in (d, d_extra, d_idx):
                    b.free()
    assert launches == len(rc.COUNTS) * 2 * 2 * 8 * 3
    assert not bad, (len(bad), bad[:8])


def test_take_refuses_a_list_that_is_not_ascending_or_leaves_the_table(lib, ctx):
    table = rc.raw_rows(300, 68, np.random.default_rng(5))
    d = _upload_rows(ctx, table, 0)
    d_idx, d_out = ctx.alloc(4 * 300), ctx.alloc(68 * 300 + 64)
    try:
        for idx in ([3, 3], [5, 4], [0, 300], [299, 4000000000]):
            d_idx.upload(np.array(idx, np.uint32))
            with pytest.raises(lib.GsxError, match="not strictly ascending inside"):
                lib.rows_take_dev(ctx, d.ptr, 0, 68, 300, d_idx.ptr, len(idx), [], None, 0, d_out.ptr)
        L = lib.load()
        none = (C.c_int32 * 1)(0)
        assert L.gsx_rows_take_dev(ctx.handle, d.ptr, 0, 68, 300, None, 301, none, 0, None, 0, d_out.ptr, 68) != 0      # more rows out than in
        assert L.gsx_rows_take_dev(ctx.handle, d.ptr, 0, 68, 300, None, 300, none, 0, None, 0, d_out.ptr, 71) != 0      # stride_out != stride_in + e
        assert L.gsx_rows_take_dev(ctx.handle, d.ptr, 0, 68, 300, None, 300, none, 0, None, 5, d_out.ptr, 73) != 0      # e > 4
        assert L.gsx_rows_take_dev(ctx.handle, d.ptr, 0, 68, 300, None, 300, (C.c_int32 * 1)(66), 1, None, 0, d_out.ptr, 68) != 0
        lib.rows_take_dev(ctx, d.ptr, 0, 68, 300, None, 300, [], None, 0, d_out.ptr)                                      # the context still works
        assert d_out.download(np.uint8, 68 * 300).tobytes() == table.tobytes()
    finally:
        for b in (d, d_idx, d_out):
            b.free()


# ------------------------------------------------------------------------------------------------------------ colours

def test_resident_colours_are_the_host_paths(lib, ctx):
    dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    table = rc.colour_table(np.random.default_rng(0xc0105))
    n = len(table)
    assert len(rc.near_integer_f_dc()) >= 8
    want = dp.DataProcessor._compute_rgb_from_sh(table)
    np.testing.assert_array_equal(want, rc.numpy_rgb(np.stack([table["f_dc_%d" % c] for c in range(3)], axis=1)))
    rr = lib.ResidentRows.from_host(table, first_byte=7)
    bufs = [ctx.alloc(12 * n + 16), ctx.alloc(3 * n + 16), ctx.alloc(4 * (3 * n // 64 + 4096)), ctx.alloc(16)]
    try:
        patched = lib.resident_rgb_dev(ctx, rr, ["f_dc_%d" % c for c in range(3)], *bufs)
        got = bufs[1].download(np.uint8, 3 * n).reshape(n, 3)
        words = bufs[0].download(np.uint32, 3 * n).reshape(n, 3)
    finally:
        for b in bufs:
            b.free()
        rr.close()
    assert patched is not None and patched >= 1                       # the patch path ran
    np.testing.assert_array_equal(words, np.stack([table["f_dc_%d" % c].view(np.uint32) for c in range(3)], axis=1))   # NaN payloads, -0.0
    np.testing.assert_array_equal(got, want)


def test_patch_entry(lib, ctx):
    base = np.arange(1000, dtype=np.uint32).astype(np.uint8)
    d = ctx.alloc(1000 + 16).upload(base)
    try:
        idx, val = np.array([0, 999, 17, 500], np.uint32), np.array([9, 8, 7, 6], np.uint8)
        lib.dev_patch_u8(ctx, d.ptr, 1000, idx, val)
        want = base.copy()
        want[idx] = val
        np.testing.assert_array_equal(d.download(np.uint8, 1000), want)
        lib.dev_patch_u8(ctx, d.ptr, 1000, idx[:0], val[:0])
        with pytest.raises(lib.GsxError, match="gsx_dev_patch_u8"):
            lib.dev_patch_u8(ctx, d.ptr, 1000, np.array([1000], np.uint32), np.array([1], np.uint8))
        np.testing.assert_array_equal(d.download(np.uint8, 1000), want)
    finally:
        d.free()


# ------------------------------------------------------------------------------------------------------------ the readers' keep=

def _formats(name):
    return importlib.import_module("3dgsconverter_amd.formats." + name)


def _jobs(tmp, rng):
    """{name: (reader, path)}: a small file per reader from the numpy builders; two files for the readers the lifetime test uses"""
    plyr = _formats("ply_reader")
    fields = [(f, "f8" if f in ("x", "y", "z") else t) for f, t in pn.canonical_fields(3)]
    pn.write_ply(str(tmp / "transcoded.ply"), [("vertex", pn.build(300, fields, rng))])
    pn.write_ply(str(tmp / "canonical.ply"), [("vertex", pn.build(300, pn.canonical_fields(3), rng))])
    pn.write_ply(str(tmp / "cc.ply"), [("vertex", pn.build(300, pn.cc_fields(2), rng))])
    pn.write_ply(str(tmp / "empty.ply"), [("vertex", pn.build(0, fields, rng))])
    jobs = {
        "ply_3dgs_transcoded": (plyr.read_ply_3dgs, str(tmp / "transcoded.ply")),
        "ply_3dgs_canonical": (plyr.read_ply_3dgs, str(tmp / "canonical.ply")),
        "ply_3dgs_empty": (plyr.read_ply_3dgs, str(tmp / "empty.ply")),
        "ply_cc": (plyr.read_ply_cc, str(tmp / "cc.ply")),
        "compressed_ply": (_formats("compressed_ply_reader").read_compressed_ply, cn.scene_file(str(tmp / "a.cply.ply"), 600, 3, 5)),
        "compressed_ply_tail": (_formats("compressed_ply_reader").read_compressed_ply, cn.scene_file(str(tmp / "tail.ply"), 700, 3, 5, chunks=2)),
        "ksplat": (_formats("ksplat_reader").read_ksplat, kn.random_file(str(tmp / "a.ksplat"), 1, 2, 300, 7)),
        "spz": (_formats("spz_reader").read_spz, zn.build_file(str(tmp / "a.spz"), 3, 3, 300, rng, gzip_level=6)),
        "spz_other": (_formats("spz_reader").read_spz, zn.build_file(str(tmp / "b.spz"), 3, 3, 431, rng, gzip_level=6)),
        "splat": (_formats("splat_reader").read_splat, sn.build_file(str(tmp / "a.splat"), 300, rng)),
        "splat_empty": (_formats("splat_reader").read_splat, sn.build_file(str(tmp / "empty.splat"), 0, rng)),
    }
    try:
        from PIL import features
        if features.check("webp"):
            jobs["sog"] = (_formats("sog_reader").read_sog, gn.build_file(str(tmp / "a.sog"), 300, 2, 70, rng))
    except ImportError:
        pass
    try:
        import pandas  # noqa: F401
        import pyarrow  # noqa: F401
        table = np.zeros(300, qn.canonical_fields(with_rgb=True))
        for f, t in qn.canonical_fields():
            table[f] = (rng.standard_normal(300) * 3).astype(t)
        qn.write_file(table, str(tmp / "a.parquet"))
        jobs["parquet"] = (_formats("parquet_reader").read_parquet, str(tmp / "a.parquet"))
    except ImportError:
        pass
    return jobs


@pytest.fixture(scope="module")
def jobs(lib, tmp_path_factory):
    return _jobs(tmp_path_factory.mktemp("resident_readers"), np.random.default_rng(0x6b656570))


KEPT = ("ply_3dgs_transcoded", "ply_cc", "compressed_ply", "compressed_ply_tail", "ksplat", "spz", "splat", "sog", "parquet")
NOT_KEPT = ("ply_3dgs_canonical", "ply_3dgs_empty", "splat_empty")


def _first(r):
    return r[0] if isinstance(r, tuple) else r


@pytest.mark.parametrize("name", KEPT + NOT_KEPT)
def test_reader_keep(lib, jobs, name):
    if name not in jobs:
        pytest.skip("pyarrow is missing" if name == "parquet" else "Pillow lacks WebP")
    read, path = jobs[name]
    before = lib.ResidentRows.open_count
    plain_prof, prof, keep = {}, {}, {"stale": 1}
    plain = _first(read(path, profile=plain_prof))
    table = _first(read(path, profile=prof, keep=keep))
    try:
        assert plain.dtype == table.dtype and plain.tobytes() == table.tobytes()
        assert prof == plain_prof or pc.same(prof, plain_prof)                   # the profile is unchanged
        if name in NOT_KEPT:
            assert keep == {} and lib.ResidentRows.open_count == before
            return
        assert sorted(keep) == ["rows"] and lib.ResidentRows.open_count == before + 1
        rr = keep["rows"]
        assert (rr.n, rr.dtype, rr.first_byte, rr.device) == (len(table), table.dtype, 0, 0) and rr.ptr % 16 == 0
        assert rr.download().tobytes() == table.tobytes()
        assert pc.same(lib.table_profile_dev(rr._ctx, rr.ptr, 0, rr.n, rr.dtype), pc.expected(table))   # the slack behind the rows is there
    finally:
        if "rows" in keep:
            keep["rows"].close()
    assert lib.ResidentRows.open_count == before
    only_keep = {}
    again = _first(read(path, keep=only_keep))                                    # keep= without profile=
    assert again.tobytes() == table.tobytes() and ("rows" in only_keep) == (name in KEPT)
    if only_keep:
        assert only_keep["rows"].download().tobytes() == table.tobytes()
        only_keep["rows"].close()
    assert lib.ResidentRows.open_count == before


def test_kept_rows_outlive_the_next_read_and_the_arenas(lib, jobs):
    read = jobs["spz"][0]
    before = lib.ResidentRows.open_count
    keep_a, keep_b = {}, {}
    a = read(jobs["spz"][1], keep=keep_a)
    b = read(jobs["spz_other"][1], keep=keep_b)                                   # the same lease group's buffers, written again
    lib.release_arenas()
    try:
        assert len(a) != len(b)
        assert keep_a["rows"].download().tobytes() == a.tobytes()
        assert keep_b["rows"].download().tobytes() == b.tobytes()
    finally:
        for k in (keep_a, keep_b):
            k["rows"].close()
            k["rows"].close()                                                     # twice is harmless
    assert lib.ResidentRows.open_count == before and keep_a["rows"].closed
    with pytest.raises(ValueError, match="closed"):
        keep_a["rows"].download()
    c = read(jobs["spz"][1])                                                      # the arenas come back
    assert c.tobytes() == a.tobytes()
