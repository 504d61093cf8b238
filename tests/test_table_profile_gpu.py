"""-m gpu: gsx_table_profile_dev, one pass over resident rows -- the struct of the host twin and numpy's answer on every case
of tests/profile_cases.py, with row 0 at byte 0 and at byte 7 of the device buffer; the layouts it refuses; and the readers'
``profile=`` keyword: every reader returns the table it returns without the keyword, bit for bit, marks a "profile" stage, and
fills the dict with numpy's answer on that table (the compressed-PLY reader on a file whose vertex count exceeds 256 x chunks)."""
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
import sog_read_numpy as gn  # noqa: E402
import splat_read_numpy as sn  # noqa: E402
import spz_read_numpy as zn  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = pc.cases()


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


def _resident(ctx, table, first_byte):
    """the table's bytes from byte `first_byte` of a device buffer, 0xff before them and in the 16 bytes behind them (a NaN
    pattern wherever a stray read would land)"""
    raw = np.full(first_byte + table.nbytes + 16, 0xff, np.uint8)
    raw[first_byte:first_byte + table.nbytes] = np.ascontiguousarray(table).view(np.uint8).reshape(-1)
    return ctx.alloc(raw.nbytes).upload(raw)


@pytest.mark.parametrize("first_byte", pc.FIRST_BYTES)
def test_device_profile_is_the_host_twins_and_numpys(lib, ctx, first_byte):
    bad = []
    for case in CASES:
        d = _resident(ctx, case.table, first_byte)
        try:
            got = lib.table_profile_dev(ctx, d, first_byte, len(case.table), case.table.dtype)
        finally:
            d.free()
        want, host = pc.expected(case.table), lib.host_table_profile(case.table, threads=1)
        ok = pc.same(got, want) and got["rest_nonzero"] == host["rest_nonzero"] and got["nan_axes"] == host["nan_axes"]
        for a in range(3):                                     # the same struct as the host twin: a zero's sign included
            if ok and not (want["nan_axes"] >> a) & 1:
                ok = (np.float32(got["lo"][a]).tobytes() == np.float32(host["lo"][a]).tobytes()
                      and np.float32(got["hi"][a]).tobytes() == np.float32(host["hi"][a]).tobytes())
        if not ok:
            bad.append((case.name, got, want, host))
    assert not bad, bad[:3]


def test_refused_arguments(lib, ctx):
    d = ctx.alloc(4 * 513 + 32)
    try:
        for name, lay in pc.refused_layouts(lib):
            res = lib.TableProfile()
            assert lib.load().gsx_table_profile_dev(ctx.handle, d.ptr, 0, 4, C.byref(lay), C.byref(res)) != 0, name
            assert "gsx_table_profile_dev" in lib.last_error() and "byte" in lib.last_error(), lib.last_error()
        lay, _ = lib.profile_layout(pc.table_dtype(248, 45))
        res = lib.TableProfile()
        for ptr, first, n in ((d.ptr, 0, 0), (d.ptr, 16, 4), (d.ptr, -1, 4), (d.ptr + 4, 0, 4), (None, 0, 4)):
            assert lib.load().gsx_table_profile_dev(ctx.handle, ptr, first, n, C.byref(lay), C.byref(res)) != 0, (first, n)
    finally:
        d.free()


# ------------------------------------------------------------------------------------------------------------ the readers

def _formats(name):
    return importlib.import_module("3dgsconverter_amd.formats." + name)


def _ply_files(tmp, rng):
    """a 3DGS file whose rows need the transcode (double coordinates), one the reader takes as it is, a CloudCompare file"""
    fields = [(f, "f8" if f in ("x", "y", "z") else t) for f, t in pn.canonical_fields(3)]
    t = pn.build(300, fields, rng)
    for i in range(9, 45):
        t["f_rest_%d" % i] = 0.0                                          # a degree-1 scene in 45 columns
    t["f_rest_44"][299] = np.float32(np.nan)
    pn.write_ply(str(tmp / "transcoded.ply"), [("vertex", t)])
    c = pn.build(300, pn.canonical_fields(3), rng)
    c["x"][17] = np.inf
    pn.write_ply(str(tmp / "canonical.ply"), [("vertex", c)])
    cc = pn.build(300, pn.cc_fields(2), rng)
    pn.write_ply(str(tmp / "cc.ply"), [("vertex", cc)])
    return str(tmp / "transcoded.ply"), str(tmp / "canonical.ply"), str(tmp / "cc.ply")


@pytest.fixture(scope="module")
def reader_runs(lib, tmp_path_factory):
    """{name: (rows without the keyword, rows with it, the dict, the stage clocks with it, the stage clocks without it)}"""
    tmp = tmp_path_factory.mktemp("profile_readers")
    rng = np.random.default_rng(0x70726f66)
    plyr = _formats("ply_reader")
    transcoded, canonical, cc = _ply_files(tmp, rng)
    jobs = {
        "ply_3dgs_transcoded": (plyr.read_ply_3dgs, transcoded),
        "ply_3dgs_canonical": (plyr.read_ply_3dgs, canonical),
        "ply_cc": (plyr.read_ply_cc, cc),
        "compressed_ply_tail": (_formats("compressed_ply_reader").read_compressed_ply, cn.scene_file(str(tmp / "tail.ply"), 700, 3, 5, chunks=2)),
        "compressed_ply_no_chunks": (_formats("compressed_ply_reader").read_compressed_ply, cn.scene_file(str(tmp / "none.ply"), 40, 1, 6, chunks=0)),
        "ksplat": (_formats("ksplat_reader").read_ksplat, kn.random_file(str(tmp / "a.ksplat"), 1, 2, 300, 7)),
        "spz": (_formats("spz_reader").read_spz, zn.build_file(str(tmp / "a.spz"), 3, 3, 300, rng, gzip_level=6)),
        "splat": (_formats("splat_reader").read_splat, sn.build_file(str(tmp / "a.splat"), 300, rng)),
    }
    try:
        from PIL import features
        webp = bool(features.check("webp"))
    except ImportError:
        webp = False
    if webp:
        jobs["sog"] = (_formats("sog_reader").read_sog, gn.build_file(str(tmp / "a.sog"), 300, 2, 70, rng))
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
    out = {}
    for name, (read, path) in jobs.items():
        plain_ms, prof_ms, prof = {}, {}, {"stale": 1}
        plain = read(path, stage_ms=plain_ms)
        with_prof = read(path, stage_ms=prof_ms, profile=prof)
        first = lambda r: r[0] if isinstance(r, tuple) else r   # noqa: E731
        out[name] = (first(plain), first(with_prof), prof, prof_ms, plain_ms)
    return out


ALWAYS = ("ply_3dgs_transcoded", "ply_3dgs_canonical", "ply_cc", "compressed_ply_tail", "compressed_ply_no_chunks", "ksplat", "spz", "splat")
HOST_PROFILED = ("ply_3dgs_canonical", "compressed_ply_no_chunks")   # no resident rows: the host twin fills the dict


@pytest.mark.parametrize("name", ALWAYS + ("sog", "parquet"))
def test_reader_profile(reader_runs, name):
    if name not in reader_runs:
        pytest.skip("pyarrow is missing" if name == "parquet" else "Pillow lacks WebP")
    plain, with_prof, prof, prof_ms, plain_ms = reader_runs[name]
    assert plain.dtype == with_prof.dtype and plain.tobytes() == with_prof.tobytes()
    assert "stale" not in prof and sorted(prof) == ["hi", "lo", "n", "nan_axes", "rest_nonzero"]
    assert pc.same(prof, pc.expected(with_prof)), (prof, pc.expected(with_prof))
    assert "profile" not in plain_ms
    assert ("profile" in prof_ms) == (name not in HOST_PROFILED)
    assert set(prof_ms) - {"profile"} == set(plain_ms)


def test_the_reader_cases_are_what_they_claim(reader_runs):
    tail = reader_runs["compressed_ply_tail"][1]
    assert len(tail) == 700 and not tail[512:].tobytes().strip(b"\0") and tail[:512].tobytes().strip(b"\0")
    prof = reader_runs["ply_3dgs_transcoded"][2]
    assert prof["rest_nonzero"] == (1 << 9) - 1 | 1 << 44                  # the NaN in f_rest_44 counts
    assert reader_runs["ply_3dgs_canonical"][2]["hi"][0] == np.inf
