"""-m gpu: the .splat writer on the MI355X (csrc/splat.hip through formats/splat_writer.py) -- every golden file of the reference
byte for byte, the device's key order against numpy's stable argsort over 2^24 bit patterns, ragged sizes and odd row layouts
against the restatement, 1M rows, two writers at once, and the failed-probe path."""
import hashlib
import importlib
import json
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import splat_numpy  # noqa: E402
import layout_refusals as refusals  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "splat_ref.npz")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return g, json.loads(bytes(g["spec"]).decode())


@pytest.fixture(scope="module")
def writer():
    return importlib.import_module("3dgsconverter_amd.formats.splat_writer")


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgsconverter_amd._lib")


def _table(g, spec, name):
    return g["edges__table"] if spec[name]["kind"] == "edges" else splat_numpy.case_table(spec[name])


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
        path = tmp_path / (name + ".splat")
        writer.write_splat(_table(g, spec, name), str(path))
        got = path.read_bytes()
        assert len(got) == rec["bytes"] and _same(got, g, name), name
        done += 1
    assert done >= 25


def _device_order(lib, metric):
    n = len(metric)
    ctx = lib.Context(0)
    try:
        d_m, d_k, d_o = ctx.alloc(4 * n + 16), ctx.alloc(4 * n + 16), ctx.alloc(4 * n + 16)
        d_m.upload(metric)
        lib.check(ctx.lib.gsx_splat_keys_dev(ctx.handle, d_m.ptr, n, d_k.ptr), "gsx_splat_keys_dev")
        lib.check(ctx.lib.gsx_splat_order_dev(ctx.handle, d_k.ptr, n, d_o.ptr), "gsx_splat_order_dev")
        order = d_o.download(np.uint32, n)
        for b in (d_m, d_k, d_o):
            b.free()
        return order
    finally:
        ctx.close()


def test_key_order_is_numpys_stable_argsort(gsx, lib):
    """2^24 strided float32 bit patterns (every exponent, both signs, NaNs of any payload, subnormals) plus +-0, +-inf and NaN
    runs: the device's order equals np.argsort(-metric, kind="stable")"""
    x = (np.arange(1 << 24, dtype=np.uint64) * 255 + 3).astype(np.uint32).view(np.float32)
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x00000001,
                        0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x3F800000], np.uint32).view(np.float32)
    x = np.concatenate([x, np.tile(special, 4096), x[:4096]])       # long runs of equal keys, and repeats of earlier values
    want = np.argsort(-x, kind="stable")
    got = _device_order(lib, x)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 257, 1000, 4097])
def test_ragged_sizes_and_layouts_against_the_restatement(gsx, writer, n):
    for make in (lambda: splat_numpy.random_table(n, 1000 + n), lambda: splat_numpy.random_table(n, 2000 + n, rgb=True),
                 lambda: splat_numpy.minimal_table(n, 3000 + n), lambda: splat_numpy.shuffled_table(n, 4000 + n),
                 lambda: splat_numpy.rgb_table(n, 5000 + n), lambda: splat_numpy.ties_table(n, 6000 + n, "quant"),
                 lambda: splat_numpy.ties_table(n, 7000 + n, "zeros_nans")):
        t = make()
        assert writer.encode(t).tobytes() == splat_numpy.file_bytes(t), (n, t.dtype)


def test_wide_rows_and_non_contiguous_tables(gsx, writer):
    """rows beyond 512 bytes (only the read fields go up), and a strided view of a table"""
    base = splat_numpy.random_table(3000, 5)
    wide = np.zeros(3000, base.dtype.descr + [("pad", "V400")])
    for f in base.dtype.names:
        wide[f] = base[f]
    assert writer.encode(wide).tobytes() == splat_numpy.file_bytes(base)
    assert writer.encode(base[::3]).tobytes() == splat_numpy.file_bytes(np.ascontiguousarray(base[::3]))


def test_sort_first_variant_gives_the_same_file(gsx, gold, lib):
    g, _ = gold
    t = g["edges__table"]
    want = splat_numpy.file_bytes(t)
    assert lib.splat_pack_table(t, variant="gather").tobytes() == want
    r = splat_numpy.rgb_table(5000, 9)
    assert lib.splat_pack_table(r, rgb=True, variant="gather").tobytes() == splat_numpy.file_bytes(r)


def test_one_million_rows_against_the_restatement(gsx, writer, tmp_path):
    t = splat_numpy.random_table(1_000_000, 77, rgb=True)
    t["opacity"][::1001] = np.nan
    t["scale_0"][5::3001] = -200.0
    t["rot_1"][9::70001] = np.nan
    t["f_dc_2"][11::50001] = np.inf
    stage = {}
    path = tmp_path / "m.splat"
    writer.write_splat(t, str(path), stage_ms=stage)
    assert path.read_bytes() == splat_numpy.file_bytes(t)
    assert {"upload", "key_pack", "sort", "permute", "download", "file_write"} <= set(stage)


def test_two_threads_write_different_tables_at_once(gsx, writer, tmp_path):
    tables = [splat_numpy.random_table(600_000, 31), splat_numpy.rgb_table(400_001, 32)]
    want = [splat_numpy.file_bytes(t) for t in tables]
    errors = []
    start = threading.Barrier(2)

    def run(i):
        try:
            start.wait()
            for k in range(3):
                p = tmp_path / ("t%d_%d.splat" % (i, k))
                writer.write_splat(tables[i], str(p))
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
    t = splat_numpy.edge_table()

    def off_by_one_ulp(x):
        with np.errstate(all="ignore"):
            return np.nextafter(np.exp(x), np.float32(np.inf))
    monkeypatch.setattr(lib, "np_exp_host", off_by_one_ulp)
    monkeypatch.setattr(lib, "_np_exp_checked", None)
    monkeypatch.delenv("GSX_STRICT_NUMPY", raising=False)
    for table in (t, splat_numpy.ties_table(3001, 3, "quant")):
        listed = {}
        with pytest.warns(RuntimeWarning, match="exp"):
            out = writer.encode(table, listed=listed)
        monkeypatch.setattr(lib, "_np_exp_checked", None)
        assert listed["exp_host"] is True
        assert out.tobytes() == splat_numpy.file_bytes(table)
    monkeypatch.setenv("GSX_STRICT_NUMPY", "1")
    with pytest.raises(lib.GsxError, match="exp"):
        writer.encode(t)
    monkeypatch.setattr(lib, "_np_exp_checked", None)


def _splat_refusals():
    R = refusals
    pack = "gsx_splat_pack_dev"
    dc, rgb = (-1, -1, -1), (236, 237, 238)                    # colour from f_dc_0..2, or from three bytes behind the fields
    cases = [(pack,) + c for c in R.common_cases(pack, dc, R.OPACITY)]
    cases += [(pack, "f_dc_0_absent", R.absent(R.F_DC), dc, pack + ": field 10 is required"),
              (pack, "f_dc_2_absent", R.absent(R.F_DC + 2), dc, pack + ": field 12 is required"),
              (pack, "no_f_rest", R.absent(*range(R.F_REST, R.FIELDS)), dc, None),
              (pack, "rgb_no_f_dc_no_f_rest", dict(R.absent(*range(R.F_DC, R.OPACITY), *range(R.F_REST, R.FIELDS)), row_bytes=239), rgb, None),
              (pack, "rgb_scale_2_absent", dict(R.absent(R.SCALE_2), row_bytes=239), rgb, pack + ": field 9 is required"),
              (pack, "rgb_opacity_absent", dict(R.absent(R.OPACITY), row_bytes=239), rgb, pack + ": field 13 is required"),
              (pack, "rgb_field_over_the_end", dict(f10=236, row_bytes=239), rgb, pack + ": field 10 at byte offset 236 of a 239-byte row"),
              (pack, "red_without_green", dict(row_bytes=239), (236, -1, 238), pack + ": red, green and blue offsets go together"),
              (pack, "red_without_blue", dict(row_bytes=239), (236, 237, -1), pack + ": red, green and blue offsets go together"),
              (pack, "green_without_red", dict(row_bytes=239), (-1, 237, 238), None),
              (pack, "blue_at_row_bytes", dict(row_bytes=238), rgb, pack + ": colour byte 2 at offset 238 of a 238-byte row"),
              (pack, "red_at_row_bytes", dict(row_bytes=239), (239, 237, 238), pack + ": colour byte 0 at offset 239 of a 239-byte row")]
    return cases


@pytest.mark.parametrize("case", _splat_refusals(), ids=lambda c: c[0] + "-" + c[1])
def test_layout_refusals(gsx, lib, case):
    """the entry point's layout checks, message for message (all return before any launch)"""
    refusals.check(lib, case[0], *case[2:])
