"""-m gpu: the compressed-PLY reader on the device -- every golden case against the reference's own rows (dtype, field order,
every row bit for bit, NaN bits included, metadata), the wide golden cases (sh elements of 38 to 256 properties), every tile
geometry of csrc/cply_read.hip at ragged row counts, every n from 1 to 33, every pattern in every slot, layouts off the grid at
narrow tiles, a round trip through this project's writer, concurrent readers, and a 1M-row file against the numpy restatement.

The kernel's tile: tile_rows halves from 256 until the staged sh rows and the output rows fit 64 KiB.  With sh_stride == n_sh
(every file: the sh properties are uchar) that is 256 rows up to 37 sh properties, 128 up to 88, 64 up to 191 and 32 up to 256
(tile_rows below restates the table of DESIGN.md section 6e; it is not read out of the library)."""
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
GOLD_WIDE = os.path.join(ROOT, "tests", "golden", "cply_read_wide_ref.npz")
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


@pytest.fixture(scope="module")
def gold_wide():
    g = np.load(GOLD_WIDE)
    return g, json.loads(bytes(g["spec"]).decode())


def tile_rows(n_sh):
    return 256 if n_sh <= 37 else 128 if n_sh <= 88 else 64 if n_sh <= 191 else 32


def _assert_rows(what, rows, want):
    """every word of every row; names the first differing row and field"""
    assert rows.dtype == want.dtype and len(rows) == len(want), what
    nf = len(rows.dtype.names)
    got, exp = (np.ascontiguousarray(a).view(np.uint32).reshape(-1) for a in (rows, want))
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, "%s: %d words differ, first at row %d field %s: 0x%08x != 0x%08x" % (
        what, len(bad), bad[0] // nf, rows.dtype.names[bad[0] % nf], got[bad[0]], exp[bad[0]])


def _against_restatement(reader, path, what):
    rows, meta = reader.read_compressed_ply(path)
    want, wmeta = crn.read(path)
    assert meta == wmeta, what
    _assert_rows(what, rows, want)
    return rows


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


def test_every_wide_golden_case_is_the_references_rows(gold_wide, reader, tmp_path):
    g, spec = gold_wide
    checked = 0
    for name, rec in spec.items():
        assert "error" not in rec, name
        path = _file(g, name, tmp_path)
        if len(rec["names"]) - 17 > 256:                              # the reference reads it, the device path does not
            with pytest.raises(reader.UnsupportedPlyError, match="257 sh properties"):
                reader.read_compressed_ply(path)
            continue
        rows, meta = reader.read_compressed_ply(path)
        assert list(rows.dtype.names) == rec["names"] and [rows.dtype[f].str for f in rows.dtype.names] == rec["dtype"], name
        assert meta == rec["metadata"], name
        if name + "__rows" in g:
            _assert_rows(name, rows, np.frombuffer(g[name + "__rows"].tobytes(), rows.dtype))
        elif crn.sha(rows) != g[name + "__sha256"].tobytes():
            _assert_rows(name, rows, crn.read(path)[0])               # (names the first differing row and field)
            raise AssertionError(name + ": equal to the restatement, not to the reference's sha256")
        checked += 1
    assert checked == 5
    assert sorted(tile_rows(len(r["names"]) - 17) for r in spec.values() if len(r["names"]) <= 17 + 256) == [32, 32, 64, 64, 128]


# both sides of every switch of tile_rows (37 | 38, 88 | 89, 191 | 192) and their neighbours, the ends of the range; with 41, 92
# and 194 row_words = 17 + n_sh takes every value mod 4 at every tile_rows, and the odd widths start tiles at every offset mod 16.
# n_sh = 191 is the widest launch: 65 504 bytes of dynamic LDS and the kernel's 72 static ones (bnd) make 65 576 bytes, 40
# over 64 KiB.  gfx950 takes it: the MI355X, whose workgroups may hold up to 160 KiB of LDS, launched it and returned the
# restatement's rows (recorded in DESIGN.md section 6e).
RAGGED_SH = [0, 1, 2, 3, 36, 37, 38, 39, 41, 87, 88, 89, 90, 92, 190, 191, 192, 193, 194, 255, 256]


def test_the_ragged_widths_cover_every_row_size_mod_4_at_every_tile_shape():
    for T in (256, 128, 64, 32):                                       # (41, 92 and 194 are there for this)
        assert {(17 + m) % 4 for m in RAGGED_SH if tile_rows(m) == T} == {0, 1, 2, 3}, T
        assert {m % 2 for m in RAGGED_SH if tile_rows(m) == T} == {0, 1}, T


@pytest.mark.parametrize("n_sh", RAGGED_SH)
def test_every_tile_shape_at_ragged_row_counts(reader, tmp_path, n_sh):
    T = tile_rows(n_sh)
    counts = [1, 3, T - 1, T, T + 1, 255, 256, 257, 256 + T + 1, 2 * 256 + T - 1]
    for j, n in enumerate(counts):
        path = crn.scene_file(str(tmp_path / "t.ply"), n, 0, 1000 * n_sh + j, n_sh=n_sh)
        rows = _against_restatement(reader, path, "n_sh=%d n=%d" % (n_sh, n))
        assert len(rows) == n and len(rows.dtype.names) == 17 + n_sh


@pytest.mark.parametrize("n_sh", [100, 200])
def test_chunk_element_one_short_and_two_long_at_narrow_tiles(reader, tmp_path, n_sh):
    T = tile_rows(n_sh)
    assert T == {100: 64, 200: 32}[n_sh]
    n = 2 * 256 + T - 1
    for chunks in (2, 5):
        path = crn.scene_file(str(tmp_path / "c.ply"), n, 0, n_sh + chunks, chunks=chunks, n_sh=n_sh)
        rows = _against_restatement(reader, path, "n_sh=%d n=%d chunks=%d" % (n_sh, n, chunks))
        tail = np.ascontiguousarray(rows[512:]).view(np.uint32)
        assert tail.any() == (chunks == 5) and rows[511:512].view(np.uint32).any()   # rows past 256 x chunks stay zero


@pytest.mark.parametrize("n_sh", [45, 89, 255])
def test_every_n_from_1_to_33_sees_every_sh_window_alignment(reader, tmp_path, n_sh):
    """sh_stride is odd, so the last tile's window starts at any offset mod 16 and n * row_words ends on any word mod 4"""
    for n in range(1, 34):
        path = crn.scene_file(str(tmp_path / "a.ply"), n, 0, 50 * n_sh + n, n_sh=n_sh)
        _against_restatement(reader, path, "n_sh=%d n=%d" % (n_sh, n))


def test_every_pattern_in_every_slot(reader, tmp_path):
    """crn.pattern_file: 4096 rows in 16 chunks, every bound of every chunk a float32 of its own.  What exposes what:
      a swapped shift or mask: position x | z hold i and 7 i mod 2048, which differ in every row but 0 and 2048 (scale: 13 i and
        i); the 10-bit y holds 5 i (11 i) mod 1024, so rows 1024 ... 2047 would show an 11-bit mask there, and row 1 (5 / 1023
        against 5 / 2047) a swapped quotient table; position and scale differ in every slot from row 1 on, so a swapped word shows;
      colour and opacity: r g b alpha = i, 3 i, 5 i, 7 i mod 256 differ pairwise in rows 1 ... 255 (a swapped byte), and every
        byte value meets the opacity table in the last slot;
      a swapped bound or table: no two of the 288 bounds are equal, so any row of the chunk shows a min or max taken from
        another axis, group or chunk (row 256 is the first that shows chunk 0's bounds used for chunk 1);
      rotation: every `largest` with 0, 1, 511, 512, 1022, 1023 in each 10-bit slot: rows 0 ... 863, where the three codes
        differ in all but 6 of every 216 rows (a swapped slot), and `largest` moves the computed component through all four;
      sh: slot k holds ((2 k + 1) i + k) mod 256, every byte value in every slot, no two slots alike in row 0.
    The exhaustive rotation sweep stays in devtools/check_cply_quat.py."""
    ch, vt, sh = crn.pattern_tables()
    p, s, c, r = (vt[f] for f in ("packed_position", "packed_scale", "packed_color", "packed_rotation"))
    for w in (p, s):
        assert set(w >> 21) == set(w & 0x7FF) == set(range(2048)) and set((w >> 11) & 0x3FF) == set(range(1024))
    assert all(set((c >> k) & 0xFF) == set(range(256)) for k in (0, 8, 16, 24))
    combos = {(int(w) >> 30, (int(w) >> 20) & 0x3FF, (int(w) >> 10) & 0x3FF, int(w) & 0x3FF) for w in r}
    assert combos == {(L, a, b, d) for L in range(4) for a in crn.ROT_EDGE for b in crn.ROT_EDGE for d in crn.ROT_EDGE}
    assert all(set(sh[f]) == set(range(256)) for f in sh.dtype.names) and len(sh.dtype.names) == 45
    assert len(ch) == 16 and len(set(np.stack([ch[f] for f in crn.CHUNK_FIELDS]).reshape(-1).tolist())) == 16 * 18
    rows = _against_restatement(reader, crn.pattern_file(str(tmp_path / "pat.ply")), "patterns")
    assert len(rows) == 4096 and not np.isnan(np.ascontiguousarray(rows).view(np.float32)).any()


@pytest.mark.parametrize("n_sh", [100, 200])
def test_layouts_off_the_grid_at_narrow_tiles(reader, tmp_path, n_sh):
    """the `permuted` golden case's layout under 64- and 32-row tiles: a chunk row of 81 bytes (a double in front, a uchar
    behind, the bounds in reverse), a vertex row of 19 bytes with the words at 15, 10, 6 and 0, shuffled sh properties"""
    rng = np.random.default_rng(600 + n_sh)
    n, nc = 600, 3
    ch = np.zeros(nc, [("pad", "<f8")] + [(f, "<f4") for f in reversed(crn.CHUNK_FIELDS)] + [("tag", "u1")])
    vt = np.zeros(n, [("packed_color", "<u4"), ("extra", "<i2"), ("packed_scale", "<u4"), ("packed_rotation", "<u4"), ("w", "u1"),
                      ("packed_position", "<u4")])
    sh = np.zeros(n, [("f_rest_%d" % i, "u1") for i in rng.permutation(n_sh)])
    for a in (ch, vt, sh):                                            # random bytes everywhere, the other properties too
        a.view(np.uint8)[:] = rng.integers(0, 256, a.nbytes, dtype=np.uint8)
    for group in (0, 6, 12):
        for k in range(3):
            lo = (rng.standard_normal(nc) * 5).astype(np.float32)
            ch[crn.CHUNK_FIELDS[group + k]] = lo
            ch[crn.CHUNK_FIELDS[group + 3 + k]] = lo + np.abs(rng.standard_normal(nc) * 3).astype(np.float32)
    path = str(tmp_path / "off.ply")
    crn.write_ply(path, [("camera", np.zeros(2, [("a", "<i4"), ("b", "<f8")])), ("chunk", ch), ("vertex", vt), ("sh", sh)])
    h = reader.parse_header(path)
    lay = reader.layout_of(h)
    assert (lay.chunk_stride, lay.vertex_stride, lay.sh_stride, lay.n_sh) == (81, 19, n_sh, n_sh)
    assert list(lay.vertex_offset) == [15, 10, 6, 0] and lay.chunk_offset[0] == 8 + 4 * 17 and lay.chunk_offset[17] == 8
    assert [lay.sh_offset[i] for i in range(n_sh)] == list(range(n_sh)) and h.element("sh").names() != ["f_rest_%d" % i for i in range(n_sh)]
    rows = _against_restatement(reader, path, "off the grid, n_sh=%d" % n_sh)
    assert len(rows) == n and list(rows.dtype.names[17:]) == h.element("sh").names()


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
