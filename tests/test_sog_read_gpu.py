"""-m gpu: the SOG reader on the device -- every golden case against the reference's own rows (dtype, field order, every row's
bytes), every u16 code / byte pattern in every slot, ragged tiles at every output alignment, palettes on both sides of the
64-entry image row, textures larger than needed and of other modes, a label past the palette, a round trip through this
project's writer, concurrent readers, and the install() binding."""
import importlib
import json
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sog_read_numpy as srn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "sog_read_ref.npz")
pytestmark = pytest.mark.gpu
TILE = 128                                   # csrc/sog_read.hip SOGR_TILE
ROW_BYTES = (68, 104, 164, 248)


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return g, json.loads(bytes(g["spec"]).decode())


@pytest.fixture(scope="module")
def reader():
    mod = importlib.import_module("3dgsconverter_amd.formats.sog_reader")
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
    rows = reader.read_sog(path)
    want = srn.read(path)
    assert rows.dtype == want.dtype, name
    _assert_bytes(name, rows, want)
    return rows


def test_every_golden_case_is_the_references_rows(gold, reader, tmp_path):
    g, spec = gold
    checked = 0
    for name, rec in spec.items():
        if "error" in rec:
            continue
        p = tmp_path / (name + ".sog")
        p.write_bytes(g[name + "__file"].tobytes())
        rows = reader.read_sog(str(p))
        assert list(rows.dtype.names) == rec["names"] and [rows.dtype[f].str for f in rows.dtype.names] == rec["dtype"], name
        assert rows.dtype.itemsize == rec["itemsize"] and len(rows) == rec["rows"], name
        if name + "__rows" in g:
            _assert_bytes(name, rows, g[name + "__rows"])
        else:
            if srn.sha(rows) != g[name + "__sha256"].tobytes():
                _assert_bytes(name, rows, srn.read(str(p)))             # (names the first differing field)
            assert srn.sha(rows) == g[name + "__sha256"].tobytes(), name
        checked += 1
    assert checked == 26


@pytest.mark.parametrize("bands", [0, 1, 2, 3])
def test_every_pattern_in_every_slot(reader, tmp_path, bands):
    """65 536 rows: every u16 code on every position axis; every byte in every channel of scales, sh0 and quats; every alpha byte
    in quats (the wrap below 252); rotation triples whose sum of squares is above 1 and next to 1 on both sides (no byte triple
    sums to exactly 1 in float32: srn.edge_triples asserts it over all 2^24)"""
    t = srn.pattern_texels(bands)
    codes = t["means_l"][:, :3].astype(np.uint32) | (t["means_u"][:, :3].astype(np.uint32) << 8)
    assert all(len(np.unique(codes[:, a])) == 65536 for a in range(3))
    for name in ("scales", "sh0", "quats"):
        assert all(len(np.unique(t[name][:, a])) == 256 for a in range(4)), name
    path = srn.pattern_file(str(tmp_path / ("pat%d.sog" % bands)), bands)
    rows = _against_restatement(reader, path, "patterns, %d bands" % bands)
    assert len(rows) == 65536 and rows.dtype.itemsize == ROW_BYTES[bands] and not rows["nx"].any()
    quat = np.stack([rows["rot_%d" % k] for k in range(4)], axis=1)
    wrapped = t["quats"][:, 3] < 252
    assert wrapped.sum() > 30000 and not quat[wrapped].any() and quat[~wrapped].any(axis=1).all()
    s = np.sum(srn.quat_component_of(t["quats"][:60, :3]) ** 2, axis=1)
    assert (s > 1).sum() >= 8 and ((s < 1) & (s > 0.9999)).sum() >= 8 and (s > 2.9).any()
    for k in range(4):                                               # slot k of rows 15 k ... holds the recovered component
        assert rows["rot_%d" % k][15 * k] == 0 and rows["rot_%d" % k][15 * k + 11] == np.sqrt(np.maximum(np.float32(1) - s[15 * k + 11], 0))


@pytest.mark.parametrize("bands", [0, 1, 2, 3])
def test_row_counts_see_ragged_tiles_and_every_output_alignment(reader, tmp_path, bands):
    rng = np.random.default_rng(20 + bands)
    palette = 77
    full = srn.random_texels(1000, bands, palette, rng)
    meta = srn.meta_for(0, bands, palette, rng)
    for n in list(range(1, 34)) + [TILE - 1, TILE, TILE + 1, 2 * TILE + 5, 1000]:
        t = {k: (v if k == "shN_centroids" else v[:n]) for k, v in full.items()}
        meta["count"] = n
        path = srn.build_file(str(tmp_path / "r.sog"), n, bands, palette, rng, meta=meta, texels=t)
        rows = _against_restatement(reader, path, "n=%d, %d bands" % (n, bands))
        assert len(rows) == n and rows.dtype.itemsize == ROW_BYTES[bands]


@pytest.mark.parametrize("bands", [1, 2, 3])
def test_palette_sizes_cross_the_64_entry_image_row(reader, tmp_path, bands):
    rng = np.random.default_rng(40 + bands)
    for palette in (1, 63, 64, 65, 128, 300):
        n = 700
        t = srn.random_texels(n, bands, palette, rng)
        lab = t["shN_labels"][:, 0].astype(np.uint32) | (t["shN_labels"][:, 1].astype(np.uint32) << 8)
        assert lab.max() == palette - 1 and lab[-1] == palette - 1
        path = srn.build_file(str(tmp_path / "p.sog"), n, bands, palette, rng, texels=t)
        rows = _against_restatement(reader, path, "palette %d, %d bands" % (palette, bands))
        if palette > 64:                                             # a linear (writer's) reading would differ
            cpc = srn.COEFFS[bands] // 3
            hit = lab >= 64
            assert hit.any() and (srn.centroid_pixel(lab[hit], 0, 3 * cpc) != lab[hit] * cpc).all()
        assert len(rows) == n


def test_a_palette_of_65536_entries_and_label_65535(reader, tmp_path):
    rng = np.random.default_rng(50)
    n, bands, palette = 300, 1, 65536
    t = srn.random_texels(n, bands, palette, rng)
    lab = rng.integers(0, palette, n).astype(np.uint32)
    lab[0], lab[-1], lab[150] = 65535, 65535, 0
    t["shN_labels"] = srn.labels_texels(lab, rng)
    path = srn.build_file(str(tmp_path / "big.sog"), n, bands, palette, rng, texels=t)
    rows = _against_restatement(reader, path, "palette 65536")
    assert len(rows) == n


def test_textures_larger_than_needed_and_of_another_width(reader, tmp_path):
    rng = np.random.default_rng(60)
    for n, bands, palette, size in ((300, 2, 90, (40, 9)), (300, 3, 130, (7, 43)), (129, 0, 0, (129, 3)), (1000, 1, 20, (1, 1003))):
        path = srn.build_file(str(tmp_path / "l.sog"), n, bands, palette, rng, size=size)
        _against_restatement(reader, path, "n=%d in %dx%d" % (n, *size))
    n, bands, palette = 200, 2, 70                                   # a centroid image with more rows and another width than the writer's
    t = srn.random_texels(n, bands, palette, rng)
    w_c, h_c = srn.centroid_dims(bands, palette)
    t["shN_centroids"] = (srn.padded(t["shN_centroids"], 1000 * 5, fill=7), 1000, 5)
    assert 1000 * 5 > w_c * h_c
    _against_restatement(reader, srn.build_file(str(tmp_path / "c.sog"), n, bands, palette, rng, texels=t), "centroid image 1000x5")


def test_images_of_other_modes_go_through_convert_rgba(reader, tmp_path):
    rng = np.random.default_rng(70)
    every = {k: "RGB" for k in srn.TEXTURES}
    for modes in (every, {"scales": "L", "means_l": "L", "shN_centroids": "L"}, {"sh0": "RGB"}):
        path = srn.build_file(str(tmp_path / "m.sog"), 333, 3, 100, rng, modes=modes)
        rows = _against_restatement(reader, path, "modes %s" % sorted(modes))
        if "sh0" in modes:
            assert len(set(rows["opacity"].tolist())) == 1           # alpha 255 in every texel


def test_a_label_equal_to_the_palette_size_in_the_last_tile_raises_numpys_error(reader, tmp_path):
    rng = np.random.default_rng(80)
    n, bands, palette = 3 * TILE + 9, 2, 70
    t = srn.random_texels(n, bands, palette, rng)
    t["shN_labels"][-2, 0], t["shN_labels"][-2, 1] = palette, 0
    path = srn.build_file(str(tmp_path / "bad.sog"), n, bands, palette, rng, texels=t)
    with pytest.raises(IndexError) as want:
        srn.read(path)
    assert str(want.value) == "index 70 is out of bounds for axis 0 with size 70"
    rows = None
    with pytest.raises(IndexError) as e:
        rows = reader.read_sog(path)
    assert str(e.value) == str(want.value) and rows is None
    t["shN_labels"][-2, 0] = palette - 1                              # and the next read on the same session is clean
    _against_restatement(reader, srn.build_file(str(tmp_path / "good.sog"), n, bands, palette, rng, texels=t), "after the flag")


def test_round_trip_through_this_projects_writer(reader, tmp_path):
    """the file write_sog writes, read back, is what the restatement reads from it -- not the written data: above 64 palette
    entries the reference's reader looks elsewhere than its writer wrote"""
    writer = importlib.import_module("3dgsconverter_amd.formats.sog_writer")
    kr = importlib.import_module("3dgsconverter_amd.formats.ksplat_reader")
    rng = np.random.default_rng(3)
    for degree, n in ((0, 2999), (3, 3001)):
        table = np.zeros(n, kr.define_dtype(3))
        for f in table.dtype.names:
            table[f] = (rng.standard_normal(n) * (3.0 if f in "xyz" else 0.7)).astype(np.float32)
        for f in ("nx", "ny", "nz"):
            table[f] = 0
        for i in range({3: 45, 0: 0}[degree], 45):
            table["f_rest_%d" % i] = 0
        path = str(tmp_path / ("rt%d.sog" % degree))
        writer.write_sog(table, path)
        rows = _against_restatement(reader, path, "round trip degree %d" % degree)
        assert len(rows) == n and rows.dtype.itemsize == ROW_BYTES[degree]


def test_concurrent_readers_get_their_own_rows(reader, tmp_path):
    paths = [srn.build_file(str(tmp_path / ("c%d.sog" % i)), 4000 + 300 * i, 3 - i % 4, 100 + 60 * i, np.random.default_rng(i)) for i in range(4)]
    want = [srn.read(p).tobytes() for p in paths]
    got, errors = {}, []

    def run(k):
        try:
            for rep in range(3):
                for i in range(len(paths)):
                    j = (i + k) % len(paths)
                    got[(k, rep, j)] = reader.read_sog(paths[j]).tobytes()
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


_STANDIN = {
    "gsconverter/__init__.py": "",
    "gsconverter/processing/__init__.py": "from . import gpu_ops\nfrom .data_processor import DataProcessor\n",
    "gsconverter/processing/gpu_ops.py": "HAS_TAICHI = False\n",
    "gsconverter/processing/data_processor.py": "class DataProcessor:\n    def __init__(self, data):\n        self.data = data\n",
    "gsconverter/converter.py": "from .processing import DataProcessor\n",
    "gsconverter/formats/__init__.py": "",
    "gsconverter/formats/sog.py": ("from ..processing import gpu_ops\n\nclass SogFormat:\n    def read(self, path, **kw):\n        return ('own', path, kw)\n"
                                   "    def write(self, data, path, **kw):\n        return 'w'\n"),
}


def test_sog_read_bound_through_install_decodes_on_the_device(gsx, gold, reader, tmp_path, monkeypatch):
    """install() on a stand-in `gsconverter` package: its SogFormat().read returns the golden rows from the device, a refused
    file goes to the stand-in's own read, and uninstall() puts that read back"""
    g, spec = gold
    for rel, src in _STANDIN.items():
        (tmp_path / rel).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / rel).write_text(src)
    saved = {m: sys.modules.pop(m) for m in list(sys.modules) if m == "gsconverter" or m.startswith("gsconverter.")}
    mine = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    monkeypatch.setattr(mine, "_REFERENCE_CLASS", None)
    monkeypatch.syspath_prepend(str(tmp_path))
    try:
        import gsconverter.formats.sog as rsog
        own_read = rsog.SogFormat.read
        rng = np.random.default_rng(12)
        meta = srn.meta_for(12, 1, 7, rng)
        meta["shN"]["bands"] = 4
        refused = srn.write_bundle(str(tmp_path / "bands4.sog"), meta, srn.encode_textures(srn.random_texels(12, 1, 7, rng), 12, 1, 7))
        gsx.install()
        try:
            assert rsog.SogFormat.read.__wrapped__ is own_read
            for name in ("b3", "palette_65", "writer_layout", "smooth_b3"):
                p = tmp_path / (name + ".sog")
                p.write_bytes(g[name + "__file"].tobytes())
                rows = rsog.SogFormat().read(str(p))
                assert len(rows) == spec[name]["rows"] and list(rows.dtype.names) == spec[name]["names"], name
                if name + "__rows" in g:
                    _assert_bytes(name, rows, g[name + "__rows"])
                else:
                    assert srn.sha(rows) == g[name + "__sha256"].tobytes(), name
            assert rsog.SogFormat().read(refused, extra=1) == ("own", refused, {"extra": 1})
        finally:
            gsx.uninstall()
        assert rsog.SogFormat.read is own_read
    finally:
        for m in [m for m in sys.modules if m == "gsconverter" or m.startswith("gsconverter.")]:
            del sys.modules[m]
        sys.modules.update(saved)
