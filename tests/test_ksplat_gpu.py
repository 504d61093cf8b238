"""-m gpu: the .ksplat writer on the MI355X (csrc/ksplat.hip through formats/ksplat_writer.py) -- every golden file of the reference
byte for byte, numpy's exp and float16 cast on the device, the rows and buckets left to numpy, ragged sizes, odd bucket sizes and
row layouts against the restatement, 1M rows, two writers at once, and the failed-probe path."""
import hashlib
import importlib
import json
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ksplat_numpy  # noqa: E402
import layout_refusals as refusals  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ksplat_ref.npz")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return g, json.loads(bytes(g["spec"]).decode())


@pytest.fixture(scope="module")
def writer():
    return importlib.import_module("3dgsconverter_amd.formats.ksplat_writer")


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgsconverter_amd._lib")


def _table(g, spec, name):
    return g["edges__table"] if spec[name]["kind"] == "edges" else ksplat_numpy.case_table(spec[name])


def _same(got: bytes, g, name):
    if name + "__sha256" in g:
        return hashlib.sha256(got).digest() == g[name + "__sha256"].tobytes()
    return got == g[name].tobytes()


def test_every_golden_case_byte_for_byte(gsx, gold, writer, tmp_path):
    g, spec = gold
    done = 0
    for name, rec in spec.items():
        if "error" in rec:
            continue
        path = tmp_path / (name + ".ksplat")
        writer.write_ksplat(_table(g, spec, name), str(path), rec["level"], **rec.get("kw", {}))
        got = path.read_bytes()
        assert len(got) == rec["bytes"] and _same(got, g, name), name
        done += 1
    assert done >= 50


def _device_math(lib, x):
    ctx = lib.Context(0)
    try:
        d_x, d_e, d_h = ctx.alloc(4 * len(x) + 16), ctx.alloc(4 * len(x) + 16), ctx.alloc(2 * len(x) + 16)
        d_x.upload(x)
        lib.check(ctx.lib.gsx_ksplat_math_dev(ctx.handle, d_x.ptr, len(x), d_e.ptr, d_h.ptr), "gsx_ksplat_math_dev")
        e, h = d_e.download(np.uint32, len(x)), d_h.download(np.uint16, len(x))
        for b in (d_x, d_e, d_h):
            b.free()
        return e, h
    finally:
        ctx.close()


def test_device_exp_and_f16_cast_are_numpys(gsx, lib):
    """2^24 strided bit patterns (every exponent, both signs) plus the probe vector and the hard cases"""
    x = (np.arange(1 << 24, dtype=np.uint64) * 255 + 3).astype(np.uint32).view(np.float32)
    hard = np.array([65504, 65519.996, 65520, -65520, 6.1e-5, 6e-8, 2.98e-8, 2.9802326e-08, 5.96e-8, 1e-40, -0.0, 0.0, np.inf, -np.inf,
                     ksplat_numpy.EXP_HARD, 88.72283935546875, -103.972084045410156], np.float32)
    x = np.concatenate([x, lib.np_exp_probe_vector(), hard])
    e, h = _device_math(lib, x)
    with np.errstate(all="ignore"):
        we, wh = np.exp(x).view(np.uint32), x.astype(np.float16).view(np.uint16)
    assert np.array_equal(e, we), np.nonzero(e != we)[0][:8]
    ok = ~np.isnan(x)                     # the writer never casts a NaN on the device (those rows are listed)
    assert np.array_equal(h[ok], wh[ok]), np.nonzero((h != wh) & ok)[0][:8]


def test_crafted_nan_rows_and_buckets_reach_the_host(gsx, gold, writer):
    g, _ = gold
    t = g["edges__table"]
    for level, kw in ((0, {}), (1, dict(bucket_size=7)), (2, {}), (7, dict(bucket_size=7))):
        listed = {}
        out, _ = writer.encode(t, level, listed=listed, **kw)
        assert len(listed["rows"]) > 0, level
        if level:
            assert len(listed["buckets"]) > 0, level
        assert out.tobytes() == ksplat_numpy.file_bytes(t, level, **kw), level
    listed = {}
    writer.encode(t, 1, listed=listed, bucket_size=7)
    assert {2, 3, 4, 5} <= set(listed["buckets"].tolist())        # rows 14-20 mixed zeros, 21-34 one sign, 35-48 NaN and +-inf
    with np.errstate(all="ignore"):
        assert np.isnan(t["opacity"][listed["rows"]]).sum() > 0


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4097])
def test_ragged_sizes_buckets_and_layouts_against_the_restatement(gsx, writer, n):
    for level, kw, tkw in ((0, {}, {}), (1, dict(bucket_size=7), dict(rgb=True)), (2, dict(bucket_size=1), {}), (1, dict(bucket_size=257), {}),
                           (2, dict(bucket_size=1000, block_size=0.37), dict(rgb=True, sh_upto=9)), (3, dict(bucket_size=97), dict(n_rest=24)),
                           (1, dict(bucket_size=5000), dict(n_rest=0))):
        t = ksplat_numpy.random_table(n, 1000 + n, **tkw)
        out, _ = writer.encode(t, level, **kw)
        assert out.tobytes() == ksplat_numpy.file_bytes(t, level, **kw), (n, level, kw, tkw)


def test_wide_rows_and_odd_offsets(gsx, writer):
    """rows beyond 512 bytes (only the read fields go up), and fields at odd byte offsets inside odd-sized rows"""
    base = ksplat_numpy.random_table(3000, 5)
    wide = np.zeros(3000, base.dtype.descr + [("pad", "V400")])
    for f in base.dtype.names:
        wide[f] = base[f]
    for level in (0, 1, 2):
        out, _ = writer.encode(wide, level, bucket_size=99)
        assert out.tobytes() == ksplat_numpy.file_bytes(base, level, bucket_size=99)
    odd = np.zeros(3000, [("tag", "u1")] + base.dtype.descr + [("z2", "u1"), ("z3", "u1")])
    for f in base.dtype.names:
        odd[f] = base[f]
    assert odd.dtype.itemsize % 4 == 3 and odd.dtype.fields["x"][1] == 1
    for level in (0, 1, 2):
        out, _ = writer.encode(odd, level, bucket_size=13)
        assert out.tobytes() == ksplat_numpy.file_bytes(base, level, bucket_size=13)


def test_one_million_rows_against_the_restatement(gsx, writer, tmp_path):
    t = ksplat_numpy.random_table(1_000_000, 77, rgb=True)
    t["opacity"][::1001] = np.nan
    t["x"][7::50001] = np.nan
    t["rot_1"][9::70001] = np.nan
    for level in (0, 1, 2):
        stage = {}
        path = tmp_path / "m.ksplat"
        writer.write_ksplat(t, str(path), level, stage_ms=stage)
        assert path.read_bytes() == ksplat_numpy.file_bytes(t, level), level
        assert {"upload", "sh_detect", "pack", "download", "file_write"} <= set(stage)


def test_two_threads_write_different_tables_at_once(gsx, writer, tmp_path):
    tables = [ksplat_numpy.random_table(600_000, 31), ksplat_numpy.random_table(400_001, 32, rgb=True, sh_upto=9)]
    levels = [1, 2]
    want = [ksplat_numpy.file_bytes(t, lv) for t, lv in zip(tables, levels)]
    errors = []
    start = threading.Barrier(2)

    def run(i):
        try:
            start.wait()
            for k in range(3):
                p = tmp_path / ("t%d_%d.ksplat" % (i, k))
                writer.write_ksplat(tables[i], str(p), levels[i])
                if p.read_bytes() != want[i]:
                    errors.append((i, k))
        except Exception as e:          # noqa: BLE001
            errors.append((i, repr(e)))
    th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors


def test_failed_probe_takes_exp_from_numpy_or_raises(gsx, writer, lib, monkeypatch):
    t = ksplat_numpy.edge_table()

    def off_by_one_ulp(x):
        with np.errstate(all="ignore"):
            return np.nextafter(np.exp(x), np.float32(np.inf))
    monkeypatch.setattr(lib, "np_exp_host", off_by_one_ulp)
    monkeypatch.setattr(lib, "_np_exp_checked", None)
    monkeypatch.delenv("GSX_STRICT_NUMPY", raising=False)
    for level in (0, 1):
        listed = {}
        with pytest.warns(RuntimeWarning, match="exp"):
            out, _ = writer.encode(t, level, listed=listed)
            monkeypatch.setattr(lib, "_np_exp_checked", None)
        assert listed["exp_host"] is True
        assert out.tobytes() == ksplat_numpy.file_bytes(t, level), level
    monkeypatch.setenv("GSX_STRICT_NUMPY", "1")
    with pytest.raises(lib.GsxError, match="exp"):
        writer.encode(t, 0)
    monkeypatch.setattr(lib, "_np_exp_checked", None)


def _ksplat_refusals():
    R = refusals
    centres, pack = "gsx_ksplat_centres_dev", "gsx_ksplat_pack_dev"
    cases = []
    for entry, args in ((centres, ()), (pack, (0,))):          # x .. opacity are required, no f_rest
        cases += [(entry,) + c for c in R.common_cases(entry, args, R.OPACITY)]
        cases += [(entry, "no_f_rest", R.absent(*range(R.F_REST, R.FIELDS)), args, None)]
    for sh_count in (9, 24):                                   # ... and f_rest_0 .. f_rest_{sh_count-1}
        cases += [(pack, "sh%d_without_f_rest_0" % sh_count, R.absent(R.F_REST), (sh_count,), pack + ": field %d is required" % R.F_REST),
                  (pack, "sh%d_without_its_last" % sh_count, R.absent(R.F_REST + sh_count - 1), (sh_count,),
                   pack + ": field %d is required" % (R.F_REST + sh_count - 1)),
                  (pack, "sh%d_without_the_next" % sh_count, R.absent(*range(R.F_REST + sh_count, R.FIELDS)), (sh_count,), None)]
    return cases


@pytest.mark.parametrize("case", _ksplat_refusals(), ids=lambda c: c[0] + "-" + c[1])
def test_layout_refusals(gsx, lib, case):
    """the entry points' layout checks, message for message (all return before any launch)"""
    refusals.check(lib, case[0], *case[2:])
