"""-m gpu: the SPZ writer on the MI355X (csrc/spz.hip through formats/spz_writer.py) -- every golden case of the reference
byte for byte, the gzip container, the rows left to numpy, a 1M-row table against the restatement, and two writers at once."""
import gzip
import hashlib
import importlib
import json
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spz_numpy  # noqa: E402
import layout_refusals as refusals  # noqa: E402
import rest_scan_cases as rsc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "spz_ref.npz")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return g, json.loads(bytes(g["spec"]).decode())


@pytest.fixture(scope="module")
def writer():
    return importlib.import_module("3dgsconverter_amd.formats.spz_writer")


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgsconverter_amd._lib")


def _table(g, spec, name):
    return g["edges__table"] if name == "edges" else spz_numpy.case_table(spec[name])


def _same(got: bytes, g, name):
    if name + "__sha256" in g:
        return hashlib.sha256(got).digest() == g[name + "__sha256"].tobytes()
    return got == g[name].tobytes()


def test_every_golden_case_byte_for_byte(gsx, gold, writer, tmp_path):
    g, spec = gold
    done = 0
    for name, rec in spec.items():
        t = _table(g, spec, name)
        path = tmp_path / (name + ".spz")
        if "error" in rec:
            with pytest.raises(ValueError) as e:
                writer.write_spz(t, str(path), compression_level=0)
            assert str(e.value) == rec["error"] and not path.exists(), name
            continue
        writer.write_spz(t, str(path), compression_level=0)
        got = gzip.decompress(path.read_bytes())
        assert got[12] == rec["degree"], name
        assert _same(got, g, name), name
        done += 1
    assert done >= 12


@pytest.mark.parametrize("level", [0, 1, 9])
def test_file_is_pythons_gzip_of_the_reference_payload(gsx, gold, writer, tmp_path, level):
    g, spec = gold
    for name in ("edges", "n1000", "low_degree"):
        path = tmp_path / ("%s_%d.spz" % (name, level))
        writer.write_spz(_table(g, spec, name), str(path), compression_level=level)
        data = path.read_bytes()
        mtime = int.from_bytes(data[4:8], "little")
        assert data == gzip.compress(g[name].tobytes(), level, mtime=mtime), (name, level)


def test_crafted_alpha_rows_are_left_to_numpy(gsx, gold, writer):
    g, _ = gold
    t = g["edges__table"]
    listed = {}
    out, _ = writer.encode(t, listed=listed)
    n = len(t)
    assert len(listed["alpha"]) > 0 and len(listed["rotation"]) > 0
    with np.errstate(all="ignore"):
        want = (1.0 / (1.0 + np.exp(-np.clip(t["opacity"], -20, 20))) * 255.0).astype(np.uint8)
    alpha = out[16 + 9 * n:16 + 10 * n]
    assert np.array_equal(alpha[listed["alpha"]], want[listed["alpha"]])
    assert np.array_equal(alpha, want)
    assert out.tobytes() == g["edges"].tobytes()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 1000, 4097])
def test_ragged_sizes_and_layouts_against_the_restatement(gsx, writer, n):
    for kw in ({}, dict(rgb=True), dict(opacity=False, dc=False), dict(n_rest=0)):
        t = spz_numpy.random_table(n, 1000 + n, **kw)
        out, _ = writer.encode(t)
        assert out.tobytes() == spz_numpy.payload(t), (n, kw)


def test_wide_rows_and_odd_offsets(gsx, writer):
    """rows beyond 512 bytes (only the read fields go up), and fields at odd byte offsets inside odd-sized rows"""
    base = spz_numpy.random_table(3000, 5)
    wide = np.zeros(3000, base.dtype.descr + [("pad", "V400")])
    for f in base.dtype.names:
        wide[f] = base[f]
    out, _ = writer.encode(wide)
    assert out.tobytes() == spz_numpy.payload(base)
    odd = np.zeros(3000, [("tag", "u1")] + base.dtype.descr + [("z2", "u1"), ("z3", "u1")])
    for f in base.dtype.names:
        odd[f] = base[f]
    assert odd.dtype.itemsize % 4 == 3 and odd.dtype.fields["x"][1] == 1
    out, _ = writer.encode(odd)
    assert out.tobytes() == spz_numpy.payload(base)


def test_one_million_rows_against_the_restatement(gsx, writer, tmp_path):
    t = spz_numpy.random_table(1_000_000, 77, rgb=True)
    t["opacity"][::1001] = np.nan
    t["rot_1"][7::50001] = np.nan
    stage = {}
    path = tmp_path / "m.spz"
    writer.write_spz(t, str(path), stage_ms=stage, compression_level=1)
    assert gzip.decompress(path.read_bytes()) == spz_numpy.payload(t)
    assert {"upload", "sh_detect", "pack", "download", "gzip", "file_write"} <= set(stage)


def test_two_threads_write_different_tables_at_once(gsx, writer, tmp_path):
    tables = [spz_numpy.random_table(600_000, 31), spz_numpy.random_table(400_001, 32, rgb=True, sh_upto=24)]
    want = [spz_numpy.payload(t) for t in tables]
    errors = []
    start = threading.Barrier(2)

    def run(i):
        try:
            start.wait()
            for k in range(3):
                p = tmp_path / ("t%d_%d.spz" % (i, k))
                writer.write_spz(tables[i], str(p), compression_level=0)
                if gzip.decompress(p.read_bytes()) != want[i]:
                    errors.append((i, k))
        except Exception as e:          # noqa: BLE001
            errors.append((i, repr(e)))
    th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors


def _spz_refusals():
    R = refusals
    rest, pack = "gsx_spz_rest_nonzero_dev", "gsx_spz_pack_dev"
    cases = []
    for entry, args in ((rest, (0,)), (pack, (0,))):          # x .. scale_2 are required, nothing behind them
        cases += [(entry,) + c for c in R.common_cases(entry, args, R.SCALE_2)]
        cases += [(entry, "no_colour_no_opacity_no_sh", R.absent(*range(R.F_DC, R.FIELDS)), args, None),
                  (entry, "f_dc_0_without_f_dc_1", R.absent(R.F_DC + 1), args, entry + ": f_dc_0 without f_dc_1 / f_dc_2"),
                  (entry, "f_dc_0_without_f_dc_2", R.absent(R.F_DC + 2), args, entry + ": f_dc_0 without f_dc_1 / f_dc_2"),
                  (entry, "f_dc_1_without_f_dc_0", R.absent(R.F_DC), args, None)]
    cases += [(pack, "degree1_without_f_rest_16", R.absent(R.F_REST + 16), (1,), pack + ": f_rest_16 is absent"),
              (pack, "degree1_without_f_rest_3", R.absent(R.F_REST + 3), (1,), None),
              (pack, "degree3_without_f_rest_44", R.absent(R.F_REST + 44), (3,), pack + ": f_rest_44 is absent"),
              (rest, "scan_of_absent_f_rest_5", R.absent(R.F_REST + 5), (1 << 5,), rest + ": f_rest_5 is absent"),
              (rest, "scan_beside_absent_f_rest_5", R.absent(R.F_REST + 5), (1 << 4,), None)]
    return cases


@pytest.mark.parametrize("case", _spz_refusals(), ids=lambda c: c[0] + "-" + c[1])
def test_layout_refusals(gsx, lib, case):
    """the entry points' layout checks, message for message (all return before any launch)"""
    refusals.check(lib, case[0], *case[2:])


@pytest.mark.parametrize("row_bytes,n", rsc.CASES)
def test_rest_scan_is_numpys_any_nonzero_at_the_edge_values(gsx, lib, row_bytes, n):
    """gsx_spz_rest_nonzero_dev on rows of 248 bytes (tiles of 128) and of 261 (tiles of 64, every field at an odd offset), one
    row, one full tile and one row more: -0.0 in the last row sets no bit; the smallest denormal of either sign, a NaN and 1.0
    set exactly their field's bit; the fields that are not asked for hold 1.0 and never show"""
    t = rsc.table(row_bytes, n)
    lay = lib.spz_layout(t.dtype)
    ctx = lib.Context(0)
    d_rows = ctx.alloc(t.nbytes + 64)
    try:
        for i, want, word in rsc.plantings(t):
            d_rows.upload(t)
            got = lib.rest_nonzero_word(ctx.lib, ctx, d_rows, lay, n, rsc.ASKED)
            assert got == word, "f_rest_%d: got %#x, numpy %#x" % (i, got, word)
    finally:
        d_rows.free()
        ctx.close()
