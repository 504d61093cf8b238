"""-m gpu: the .ksplat reader on the device -- every golden case against the reference's own rows (dtype, field order, metadata,
every row as uint32 words, NaN bits included), every u16 / float16 / byte pattern in every slot, ragged tiles and bucket
boundaries, 1M rows per level, a round trip through this project's writer, and concurrent readers."""
import importlib
import json
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ksplat_read_numpy as krn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ksplat_read_ref.npz")
pytestmark = pytest.mark.gpu
TILE = 128                                   # csrc/ksplat_read.hip KSR_TILE


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return g, json.loads(bytes(g["spec"]).decode())


@pytest.fixture(scope="module")
def reader():
    mod = importlib.import_module("3dgsconverter_amd.formats.ksplat_reader")
    importlib.import_module("3dgsconverter_amd._lib").require_hip()
    return mod


def _same_meta(a, b):
    return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)


def _assert_words(name, rows, want_words):
    got = np.ascontiguousarray(rows).view(np.uint32).reshape(-1)
    want = np.ascontiguousarray(want_words).view(np.uint32).reshape(-1)
    assert got.shape == want.shape, "%s: %d words, %d expected" % (name, got.size, want.size)
    bad = np.nonzero(got != want)[0]
    nf = len(rows.dtype.names)
    assert len(bad) == 0, "%s: %d words differ, first at row %d field %s: 0x%08x != 0x%08x" % (
        name, len(bad), bad[0] // nf, rows.dtype.names[bad[0] % nf], got[bad[0]], want[bad[0]])


def _against_restatement(reader, path, name):
    rows, meta = reader.read_ksplat(path)
    want, wmeta = krn.read(path)
    assert rows.dtype == want.dtype and _same_meta(meta, wmeta), name
    _assert_words(name, rows, want)
    return rows


def test_every_golden_case_is_the_references_rows(gold, reader, tmp_path):
    g, spec = gold
    checked = 0
    for name, rec in spec.items():
        if "error" in rec:
            continue
        p = tmp_path / (name + ".ksplat")
        p.write_bytes(g[name + "__file"].tobytes())
        rows, meta = reader.read_ksplat(str(p))
        assert list(rows.dtype.names) == rec["names"] and [rows.dtype[f].str for f in rows.dtype.names] == rec["dtype"], name
        assert _same_meta(meta, rec["metadata"]) and len(rows) == rec["rows"], name
        if name + "__rows" in g:
            _assert_words(name, rows, g[name + "__rows"])
        else:
            if krn.sha(rows) != g[name + "__sha256"].tobytes():
                _assert_words(name, rows, krn.read(str(p))[0])          # (names the first differing word)
            assert krn.sha(rows) == g[name + "__sha256"].tobytes(), name
        checked += 1
    assert checked == len([r for r in spec.values() if "error" not in r]) == 52


@pytest.mark.parametrize("level", [0, 1, 2])
def test_every_pattern_in_every_slot(reader, tmp_path, level):
    """all 65 536 u16 patterns as position, scale, rotation and level-1 sh (every float16, NaNs of both kinds), all 256 bytes
    as colour, opacity and level-2 sh; at level 0 float32 patterns over the whole exponent range, NaN payloads included"""
    path = krn.pattern_file(str(tmp_path / ("pat%d.ksplat" % level)), level)
    rows = _against_restatement(reader, path, "patterns level %d" % level)
    assert len(rows) == 65536
    if level == 1:
        assert np.isnan(rows["scale_0"]).sum() == 2 * 1023 and np.isnan(rows["f_rest_23"]).sum() == 2 * 1023
        assert rows["scale_1"].view(np.uint32)[0x7C01] == 0x7F802000    # numpy keeps a signalling NaN signalling
    if level == 0:
        assert np.isnan(rows["x"]).any()


def test_ragged_tiles_bucket_boundaries_and_sections(reader, tmp_path):
    rng = np.random.default_rng(77)
    S, k = krn.section, 0
    for n in (1, 3, 4, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 5, 1000):
        for level, degree in ((0, 1), (1, 2), (2, 1)):
            k += 1
            path = krn.build_file(str(tmp_path / ("r%d.ksplat" % k)), level, [S(level, degree, n, rng, bucket_size=TILE - 1 if n > TILE else 3)])
            _against_restatement(reader, path, "n=%d level %d" % (n, level))
    # buckets that end on, just before and just after a tile boundary; empty buckets in between; a partial list longer than the rows
    lens = [TILE - 3, 0, 3, 1, 0, 0, TILE - 1, 1, 2 * TILE, 5, 0, 9]
    path = krn.build_file(str(tmp_path / "pb.ksplat"), 1, [S(1, 1, sum(lens) + 2 * TILE, rng, bucket_size=TILE, full_buckets=2, partial=lens)])
    _against_restatement(reader, path, "partial buckets around tiles")
    lens = rng.integers(0, 40, 3000)
    path = krn.build_file(str(tmp_path / "pm.ksplat"), 2, [S(2, 2, int(lens.sum()) - 17, rng, bucket_size=64, full_buckets=0, partial=lens)])
    _against_restatement(reader, path, "3000 partial buckets")
    # three sections of different degrees, bucket sizes, block sizes and padding; odd row counts put tiles off 16-byte boundaries
    for level in (0, 1, 2, 5):
        path = krn.build_file(str(tmp_path / ("s3_%d.ksplat" % level)), level, [
            S(level, 1, 2 * TILE + 37, rng, bucket_size=50, max_splats=3 * TILE, block_size=0.37),
            S(level, 2, TILE + 1, rng, bucket_size=TILE + 1, max_splats=TILE + 2, scale_range=1000),
            S(level, 0, 3 * TILE - 1, rng, bucket_size=7, block_size=-2.0)])
        rows = _against_restatement(reader, path, "three sections level %d" % level)
        assert len(rows) == 6 * TILE + 37 and rows.dtype.itemsize == 164
        assert not rows["f_rest_9"][:2 * TILE + 37].any() and not rows["f_rest_0"][3 * TILE + 38:].any() and not rows["nx"].any()


@pytest.mark.parametrize("level", [0, 1, 2])
def test_one_million_rows_equal_the_restatement(reader, tmp_path, level):
    path = krn.random_file(str(tmp_path / "m.ksplat"), level, 2, 1_000_000 + 77, 100 + level, bucket_size=256, block_size=5.0)
    rows, meta = reader.read_ksplat(path)
    want, wmeta = krn.read(path)
    assert _same_meta(meta, wmeta) and rows.dtype == want.dtype and krn.sha(rows) == krn.sha(want)


def test_round_trip_through_this_projects_writer(reader, tmp_path):
    writer = importlib.import_module("3dgsconverter_amd.formats.ksplat_writer")
    rng = np.random.default_rng(3)
    for level, degree, n, bucket in ((0, 2, 3000, 256), (1, 1, 777, 100), (2, 2, 5000, 256), (1, 0, 256, 256)):
        table = np.zeros(n, krn.define_dtype(degree))
        for f in table.dtype.names:
            table[f] = (rng.standard_normal(n) * (3.0 if f in "xyz" else 0.7)).astype(np.float32)
        path = str(tmp_path / ("rt%d_%d.ksplat" % (level, degree)))
        writer.write_ksplat(table, path, level, bucket_size=bucket)
        rows = _against_restatement(reader, path, "round trip level %d degree %d" % (level, degree))
        assert len(rows) == n and rows.dtype == table.dtype
        if level == 0:                       # level 0 stores position, rotation and sh as they are
            for f in ("x", "y", "z", "rot_0", "rot_3", "f_rest_0", "f_rest_23"):
                assert np.array_equal(rows[f].view(np.uint32), table[f].view(np.uint32)), f


def test_concurrent_readers_get_their_own_rows(reader, tmp_path):
    paths = [krn.random_file(str(tmp_path / ("c%d.ksplat" % i)), i % 3, 2 - i % 3, 40000 + 3000 * i, i, bucket_size=100 + i) for i in range(4)]
    want = [krn.read(p)[0].tobytes() for p in paths]
    got, errors = {}, []

    def run(k):
        try:
            for rep in range(3):
                for i in range(len(paths)):
                    j = (i + k) % len(paths)
                    got[(k, rep, j)] = reader.read_ksplat(paths[j])[0].tobytes()
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
