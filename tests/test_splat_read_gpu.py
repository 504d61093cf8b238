"""-m gpu: the .splat reader on the device -- every golden case against the reference's own rows (dtype, field order, every row's
bytes, NaN bits included), every pair of rotation bytes and every colour / alpha byte, numpy's float32 log on the probe
vector in every scale slot, every tile boundary with every ragged tail, 250 077 random-byte rows, a round trip through this
project's writer, concurrent readers, and the path taken when the probe of numpy's log fails."""
import hashlib
import importlib
import json
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import splat_read_numpy as sn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "splat_read_ref.npz")
pytestmark = pytest.mark.gpu
TILE = 128                                   # csrc/splat_read.hip SPLR_TILE


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return g, json.loads(bytes(g["spec"]).decode())


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgsconverter_amd._lib")


@pytest.fixture(scope="module")
def reader(lib):
    mod = importlib.import_module("3dgsconverter_amd.formats.splat_reader")
    lib.require_hip()
    return mod


@pytest.fixture(scope="module")
def pattern(tmp_path_factory):
    """the pattern file and the restatement's rows of it, shared (built once, left unchanged)"""
    path = sn.pattern_file(str(tmp_path_factory.mktemp("splat_pattern") / "pattern.splat"))
    return path, sn.read(path)


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
    rows = reader.read_splat(path)
    want = sn.read(path)
    assert rows.dtype == want.dtype, name
    _assert_bytes(name, rows, want)
    return rows


def test_every_golden_case_is_the_references_rows(gold, reader, pattern, tmp_path):
    g, spec = gold
    checked = 0
    for name, rec in spec.items():
        if name + "__file" in g:
            p = tmp_path / (name + ".splat")
            p.write_bytes(g[name + "__file"].tobytes())
            path = str(p)
        else:
            assert name == "pattern"
            path = pattern[0]
        with open(path, "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == rec["file_sha256"], name
        rows = reader.read_splat(path)
        assert list(rows.dtype.names) == rec["names"] and [rows.dtype[f].str for f in rows.dtype.names] == rec["dtype"], name
        assert rows.dtype.itemsize == rec["itemsize"] and len(rows) == rec["rows"], name
        if name + "__rows" in g:
            _assert_bytes(name, rows, g[name + "__rows"])
        else:
            if sn.sha(rows) != g[name + "__sha256"].tobytes():
                _assert_bytes(name, rows, sn.read(path))                 # (names the first differing field)
            assert sn.sha(rows) == g[name + "__sha256"].tobytes(), name
        checked += 1
    assert checked == 14


def test_every_rotation_pair_and_every_colour_byte(reader, pattern):
    """6 x 65 536 rows: all byte pairs in each pair of rotation slots with the other two at 128; all 256 values in each colour
    and alpha slot; positions that are raw bit patterns"""
    path, want = pattern
    rows = reader.read_splat(path)
    assert rows.dtype == want.dtype and len(rows) == 6 * 65536
    _assert_bytes("patterns", rows, want)
    recs = np.fromfile(path, sn.RECORD)
    for p, (a, b) in enumerate(sn.ROT_PAIRS):
        blk = recs["rot"][65536 * p:65536 * (p + 1)]
        assert len(np.unique(blk[:, a].astype(np.uint32) << 8 | blk[:, b])) == 65536
        others = [s for s in range(4) if s not in (a, b)]
        assert (blk[:, others] == 128).all()
    for s in range(4):
        assert len(np.unique(recs["colour"][:, s])) == 256
    assert np.isnan(rows["x"]).any() and np.array_equal(rows["x"].view(np.uint32), recs["pos"][:, 0])      # the file's bits
    all128 = (recs["rot"] == 128).all(axis=1)
    assert all128.sum() == 6 and not rows["rot_0"][all128].any()
    norm = np.sqrt(sum(rows["rot_%d" % i].astype(np.float64) ** 2 for i in range(4)))
    assert np.abs(norm[~all128] - 1).max() < 1e-6
    assert not rows["nx"].any() and not rows["red"].any() and not rows["green"].any() and not rows["blue"].any()


def test_numpys_log_on_the_probe_vector_in_every_scale_slot(reader, lib, tmp_path):
    v = lib.np_log_probe_vector()
    path = sn.scale_file(str(tmp_path / "scales.splat"), v)
    rows = _against_restatement(reader, path, "scale file")
    assert len(rows) == len(v)
    with np.errstate(all="ignore"):
        want = np.log(np.maximum(v, np.float32(1e-6))).view(np.uint32)
    assert np.array_equal(rows["scale_0"].view(np.uint32), want)
    assert np.array_equal(rows["scale_1"].view(np.uint32), np.roll(want, 1237))
    assert np.array_equal(rows["scale_2"].view(np.uint32), np.roll(want, 40001))
    # the device's log over the whole domain, not only what the reader's clamp lets through
    ctx = lib.Context(0)
    try:
        d_in, d_out = ctx.alloc(v.nbytes), ctx.alloc(v.nbytes)
        d_in.upload(v)
        lib.check(ctx.lib.gsx_np_log_math_dev(ctx.handle, d_in.ptr, len(v), d_out.ptr), "gsx_np_log_math_dev")
        got = d_out.download(np.uint32, len(v))
        d_in.free()
        d_out.free()
    finally:
        ctx.close()
    with np.errstate(all="ignore"):
        full = np.log(v).view(np.uint32)
    bad = np.nonzero(got != full)[0]
    assert not len(bad), [(hex(int(v.view(np.uint32)[i])), hex(int(got[i])), hex(int(full[i]))) for i in bad[:4]]


def test_tile_boundaries_with_every_ragged_tail(reader, tmp_path):
    rng = np.random.default_rng(11)
    for n in list(range(1, 34)) + [TILE - 1, TILE, TILE + 1, 2 * TILE + 5, 1000]:
        recs = sn.random_records(n, rng)
        want = sn.decode(recs, n)
        for trailing in range(32):
            path = sn.write_file(str(tmp_path / "t.splat"), recs, trailing)
            rows = reader.read_splat(path)
            assert rows.dtype == want.dtype, (n, trailing)
            _assert_bytes("n=%d, %d trailing bytes" % (n, trailing), rows, want)


def test_250077_random_byte_rows_equal_the_restatement(reader, tmp_path):
    path = sn.build_file(str(tmp_path / "m.splat"), 250_077, np.random.default_rng(100), trailing=9)
    rows = reader.read_splat(path)
    want = sn.read(path)
    assert rows.dtype == want.dtype and len(rows) == 250_077 and sn.sha(rows) == sn.sha(want)


def test_round_trip_through_this_projects_writer(reader, tmp_path):
    writer = importlib.import_module("3dgsconverter_amd.formats.splat_writer")
    kr = importlib.import_module("3dgsconverter_amd.formats.ksplat_reader")
    rng = np.random.default_rng(3)
    for n in (3000, 129):
        table = np.zeros(n, kr.define_dtype(0))
        for f in table.dtype.names:
            table[f] = (rng.standard_normal(n) * (3.0 if f in "xyz" else 0.7)).astype(np.float32)
        for a in range(3):
            table["scale_%d" % a] = rng.normal(-4.5, 1.5, n).astype(np.float32)
        path = str(tmp_path / ("rt%d.splat" % n))
        writer.write_splat(table, path)
        rows = _against_restatement(reader, path, "round trip of %d rows" % n)     # scale_i: the restatement on the written file
        assert len(rows) == n
        order = np.lexsort((table["z"].view(np.uint32), table["y"].view(np.uint32), table["x"].view(np.uint32)))
        back = np.lexsort((rows["z"].view(np.uint32), rows["y"].view(np.uint32), rows["x"].view(np.uint32)))
        for f in "xyz":                                                           # the writer sorts the rows: paired up by position
            assert np.array_equal(rows[f][back].view(np.uint32), table[f][order].view(np.uint32)), f


def test_concurrent_readers_get_their_own_rows(reader, tmp_path):
    paths = [sn.build_file(str(tmp_path / ("c%d.splat" % i)), 40000 + 3000 * i, np.random.default_rng(i), trailing=(0, 5, 31, 16)[i])
             for i in range(4)]
    want = [sn.read(p).tobytes() for p in paths]
    got, errors = {}, []

    def run(k):
        try:
            for rep in range(3):
                for i in range(len(paths)):
                    j = (i + k) % len(paths)
                    got[(k, rep, j)] = reader.read_splat(paths[j]).tobytes()
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


def test_a_failed_probe_takes_the_scales_from_numpy_and_returns_the_same_rows(reader, lib, tmp_path, monkeypatch):
    v = lib.np_log_probe_vector()
    path = sn.scale_file(str(tmp_path / "scales.splat"), v)
    assert lib.np_log_probe() is True
    on_device = reader.read_splat(path)
    monkeypatch.setattr(lib, "_np_log_checked", False)
    on_host = reader.read_splat(path)
    assert lib.np_log_probe() is False
    assert on_host.dtype == on_device.dtype
    _assert_bytes("probe failed", on_host, on_device)
    _assert_bytes("probe failed", on_host, sn.read(path))
    ragged = sn.build_file(str(tmp_path / "r.splat"), 261, np.random.default_rng(8), trailing=7)
    _assert_bytes("probe failed, ragged", reader.read_splat(ragged), sn.read(ragged))
