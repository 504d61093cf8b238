"""-m gpu: the compressed-PLY reader on the device -- every golden case against the reference's own rows (dtype, field order,
every row bit for bit, NaN bits included, metadata), a round trip through this project's writer, concurrent readers, and a
1M-row file against the numpy restatement."""
import importlib
import json
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cply_read_numpy as crn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "cply_read_ref.npz")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return g, json.loads(bytes(g["spec"]).decode())


@pytest.fixture(scope="module")
def reader():
    mod = importlib.import_module("3dgsconverter_amd.formats.compressed_ply_reader")
    importlib.import_module("3dgsconverter_amd._lib").require_hip()
    return mod


def _file(g, name, tmp_path):
    p = tmp_path / (name + ".ply")
    p.write_bytes(g[name + "__file"].tobytes())
    return str(p)


def test_every_golden_case_is_the_references_rows(gold, reader, tmp_path):
    g, spec = gold
    checked = 0
    for name, rec in spec.items():
        if "error" in rec:
            continue
        rows, meta = reader.read_compressed_ply(_file(g, name, tmp_path))
        assert list(rows.dtype.names) == rec["names"] and [rows.dtype[f].str for f in rows.dtype.names] == rec["dtype"], name
        assert meta == rec["metadata"], name
        if name + "__rows" in g:
            want = g[name + "__rows"].view(np.uint32)
            got = np.ascontiguousarray(rows).view(np.uint32).reshape(-1)
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, "%s: %d words differ, first at row %d field %s: 0x%08x != 0x%08x" % (
                name, len(bad), bad[0] // (len(rows.dtype.names)), rows.dtype.names[bad[0] % len(rows.dtype.names)], got[bad[0]], want[bad[0]])
        else:
            assert crn.sha(rows) == g[name + "__sha256"].tobytes(), name
        checked += 1
    assert checked == 14


def test_round_trip_through_this_projects_writer(reader, tmp_path):
    from oracle import cply as ocply
    writer = importlib.import_module("3dgsconverter_amd.formats.compressed_ply_writer")
    for deg, n in ((3, 5000), (1, 777), (0, 256)):
        scene = ocply.cply_scene(n, deg, "clustered")
        path = str(tmp_path / ("rt%d.compressed.ply" % deg))
        writer.write_compressed_ply(scene, path)
        rows, meta = reader.read_compressed_ply(path)
        want, wmeta = crn.read(path)
        assert meta == wmeta and meta["count"] == n and meta["chunks"] == (n + 255) // 256
        assert rows.dtype == want.dtype and rows.tobytes() == want.tobytes()


def test_concurrent_readers_agree(reader, tmp_path):
    paths = [crn.scene_file(str(tmp_path / ("c%d.ply" % i)), 40000 + 3000 * i, 3 - i % 4, i) for i in range(4)]
    want = [crn.read(p)[0].tobytes() for p in paths]
    got = {}
    errors = []

    def run(k):
        try:
            for rep in range(3):
                for i in range(len(paths)):
                    j = (i + k) % len(paths)
                    got[(k, rep, j)] = reader.read_compressed_ply(paths[j])[0].tobytes()
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


def test_one_million_rows_equal_the_restatement(reader, tmp_path):
    path = crn.scene_file(str(tmp_path / "m.ply"), 1_000_000 + 77, 3, 11)
    rows, meta = reader.read_compressed_ply(path)
    want, wmeta = crn.read(path)
    assert meta == wmeta and crn.sha(rows) == crn.sha(want)
