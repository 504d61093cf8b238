"""-m gpu: the SPZ reader on the device -- every golden case against the reference's own rows (dtype, field order, every row's
bytes, NaN bits included), every byte / float16 / 10-bit pattern in every slot, ragged tiles at every section alignment,
250 077 degree-3 rows per version, a round trip through this project's writer, concurrent readers, and the install() binding."""
import importlib
import json
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spz_read_numpy as srn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "spz_read_ref.npz")
pytestmark = pytest.mark.gpu
TILE = 128                                   # csrc/spz_read.hip SPZR_TILE


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return g, json.loads(bytes(g["spec"]).decode())


@pytest.fixture(scope="module")
def reader():
    mod = importlib.import_module("3dgsconverter_amd.formats.spz_reader")
    importlib.import_module("3dgsconverter_amd._lib").require_hip()
    return mod


def _assert_bytes(name, rows, want):
    """both as packed rows; names the first differing row and field"""
    got = np.ascontiguousarray(rows).view(np.uint8).reshape(-1)
    want = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert got.shape == want.shape, "%s: %d bytes, %d expected" % (name, got.size, want.size)
    bad = np.nonzero(got != want)[0]
    if len(bad):
        rb = rows.dtype.itemsize
        row, col = bad[0] // rb, bad[0] % rb
        field = [f for f in rows.dtype.names if rows.dtype.fields[f][1] <= col][-1]
        raise AssertionError("%s: %d bytes differ, first at row %d field %s: %s != %s" % (
            name, len(bad), row, field, got[row * rb:][rows.dtype.fields[field][1]:][:4].tobytes().hex(),
            want[row * rb:][rows.dtype.fields[field][1]:][:4].tobytes().hex()))


def _against_restatement(reader, path, name):
    rows = reader.read_spz(path)
    want = srn.read(path)
    assert rows.dtype == want.dtype, name
    _assert_bytes(name, rows, want)
    return rows


def test_every_golden_case_is_the_references_rows(gold, reader, tmp_path):
    g, spec = gold
    checked = 0
    for name, rec in spec.items():
        if "error" in rec or name == "degree4":
            continue
        p = tmp_path / (name + ".spz")
        p.write_bytes(g[name + "__file"].tobytes())
        rows = reader.read_spz(str(p))
        assert list(rows.dtype.names) == rec["names"] and [rows.dtype[f].str for f in rows.dtype.names] == rec["dtype"], name
        assert rows.dtype.itemsize == rec["itemsize"] and len(rows) == rec["rows"], name
        if name + "__rows" in g:
            _assert_bytes(name, rows, g[name + "__rows"])
        else:
            if srn.sha(rows) != g[name + "__sha256"].tobytes():
                _assert_bytes(name, rows, srn.read(str(p)))             # (names the first differing field)
            assert srn.sha(rows) == g[name + "__sha256"].tobytes(), name
        checked += 1
    assert checked == 34


@pytest.mark.parametrize("version", [1, 2, 3])
def test_every_pattern_in_every_slot(reader, tmp_path, version):
    """65 536 rows: every byte value in every byte slot of every section; every float16 pattern as a version-1 position (NaNs of
    both kinds); every 10-bit component in each version-3 slot with each idx; 24-bit positions at +-1, +-(2^23 - 1), -2^23"""
    path = srn.pattern_file(str(tmp_path / ("pat%d.spz" % version)), version)
    rows = _against_restatement(reader, path, "patterns version %d" % version)
    assert len(rows) == 65536 and rows.dtype.itemsize == 251
    if version == 1:
        assert np.isnan(rows["x"]).sum() == 2 * 1023 and rows["x"].view(np.uint32)[0x7C01] == 0x7F802000   # a signalling NaN stays one
    else:
        assert {1 / 4096, -1 / 4096, (2 ** 23 - 1) / 4096, -(2 ** 23 - 1) / 4096, -2048.0} <= set(rows["x"][:24].tolist())
        for bits in (0, 127, 128):                                     # subnormal quotients kept; +-0 under an infinite divisor
            p = srn.pattern_file(str(tmp_path / ("pat%d_%d.spz" % (version, bits))), version, degree=0, frac_bits=bits)
            r = _against_restatement(reader, p, "patterns version %d, %d bits" % (version, bits))
            if bits == 127:
                assert 0 < abs(float(r["x"][0])) < 1.2e-38
            if bits == 128:
                assert not r["x"].any() and np.signbit(r["x"]).any() and not np.signbit(r["x"]).all()
    if version == 3:
        packed = np.frombuffer(srn.pattern_body(3), "<u4", 65536, 65536 * (9 + 1 + 3 + 3))
        for k in range(12):                                            # block k: all 1024 codes in slot k % 3 with idx k // 3
            block = packed[1024 * k:1024 * (k + 1)]
            assert set((block >> (10 * (2 - k % 3))) & 0x3FF) == set(range(1024)) and set(block >> 30) == {k // 3}


def test_every_n_from_1_to_33_sees_every_section_alignment(reader, tmp_path):
    rng = np.random.default_rng(11)
    for version, degree in ((3, 3), (2, 1), (1, 2)):
        for n in range(1, 34):
            path = srn.build_file(str(tmp_path / "a.spz"), version, degree, n, rng, gzip_level=None if n % 2 else 0)
            _against_restatement(reader, path, "n=%d version %d degree %d" % (n, version, degree))


@pytest.mark.parametrize("version", [1, 2, 3])
def test_ragged_tiles_for_every_version_and_degree(reader, tmp_path, version):
    rng = np.random.default_rng(77 + version)
    for degree in (0, 1, 2, 3):
        for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 5, 1000):
            for level in (None, 1):
                path = srn.build_file(str(tmp_path / "r.spz"), version, degree, n, rng, frac_bits=12 + degree, gzip_level=level)
                rows = _against_restatement(reader, path, "n=%d version %d degree %d gzip %s" % (n, version, degree, level))
                assert len(rows) == n and rows.dtype.itemsize == 71 + 12 * srn.SH_DIM[degree] and not rows["nx"].any()


@pytest.mark.parametrize("version", [1, 2, 3])
def test_250077_degree_3_rows_equal_the_restatement(reader, tmp_path, version):
    path = srn.build_file(str(tmp_path / "m.spz"), version, 3, 250_077, np.random.default_rng(100 + version))
    rows = reader.read_spz(path)
    want = srn.read(path)
    assert rows.dtype == want.dtype and srn.sha(rows) == srn.sha(want)


def test_round_trip_through_this_projects_writer(reader, tmp_path):
    writer = importlib.import_module("3dgsconverter_amd.formats.spz_writer")
    kr = importlib.import_module("3dgsconverter_amd.formats.ksplat_reader")
    rng = np.random.default_rng(3)
    for degree, n in ((3, 3000), (1, 777), (0, 129)):
        table = np.zeros(n, kr.define_dtype(3))
        for f in table.dtype.names:
            table[f] = (rng.standard_normal(n) * (3.0 if f in "xyz" else 0.7)).astype(np.float32)
        for i in range({3: 45, 1: 9, 0: 0}[degree], 45):          # the writer takes the degree from the last f_rest with content
            table["f_rest_%d" % i] = 0
        path = str(tmp_path / ("rt%d.spz" % degree))
        writer.write_spz(table, path, compression_level=degree)
        rows = _against_restatement(reader, path, "round trip degree %d" % degree)
        assert len(rows) == n and rows.dtype.itemsize == 71 + 12 * srn.SH_DIM[degree]
        for f in "xyz":                       # 12 fractional bits, rounded to nearest: within half a step
            assert np.abs(rows[f].astype(np.float64) - table[f].astype(np.float64)).max() <= 2.0 ** -13, f


def test_concurrent_readers_get_their_own_rows(reader, tmp_path):
    paths = [srn.build_file(str(tmp_path / ("c%d.spz" % i)), 1 + i % 3, 3 - i % 3, 40000 + 3000 * i, np.random.default_rng(i),
                            gzip_level=(0, None, 1, 0)[i]) for i in range(4)]
    want = [srn.read(p).tobytes() for p in paths]
    got, errors = {}, []

    def run(k):
        try:
            for rep in range(3):
                for i in range(len(paths)):
                    j = (i + k) % len(paths)
                    got[(k, rep, j)] = reader.read_spz(paths[j]).tobytes()
        except Exception as e:  # noqa: BLE001
            errors.append(e)
    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert len(got) == 2 * 3 * len(paths)
    for (k, rep, j), b in got.items():
        assert b == want[j], (k, rep, j)


def test_the_reference_bound_through_install_returns_the_same_rows(gsx, reader, tmp_path):
    from oracle import refload
    if not refload.available():
        pytest.skip("the reference is not mounted")
    refload.load()
    import gsconverter.formats.spz as rspz  # type: ignore
    path = srn.build_file(str(tmp_path / "i.spz"), 3, 2, 5000, np.random.default_rng(9), gzip_level=6)
    with np.errstate(all="ignore"):
        want = rspz.SpzFormat().read(path)
    gsx.install()
    try:
        assert rspz.SpzFormat.read.__wrapped__ is not None
        rows = rspz.SpzFormat().read(path)
    finally:
        gsx.uninstall()
    assert rows.dtype == want.dtype
    _assert_bytes("install()", rows, want)
