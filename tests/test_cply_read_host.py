"""-m "not gpu": the compressed-PLY reader's host side -- the header parser, what goes to the reference's own reader and what
is refused (257 sh properties and a short sh element among it), the reference's errors before any device work, the numpy
restatement against the reference's rows (tests/golden/cply_read_ref.npz, and cply_read_wide_ref.npz for sh elements of 38 to
257 properties), the host tables, and the install() binding of CompressedPlyFormat.read."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cply_read_numpy as crn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "cply_read_ref.npz")
GOLD_WIDE = os.path.join(ROOT, "tests", "golden", "cply_read_wide_ref.npz")


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return g, json.loads(bytes(g["spec"]).decode())


@pytest.fixture(scope="module")
def gold_wide():
    g = np.load(GOLD_WIDE)
    return g, json.loads(bytes(g["spec"]).decode())


@pytest.fixture(scope="module")
def reader():
    return importlib.import_module("3dgsconverter_amd.formats.compressed_ply_reader")


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgsconverter_amd._lib")


def _file(g, name, tmp_path):
    p = tmp_path / (name + ".ply")
    p.write_bytes(g[name + "__file"].tobytes())
    return str(p)


def _no_device(monkeypatch, lib):
    def boom(*a, **k):
        raise AssertionError("device work started")
    monkeypatch.setattr(lib, "cply_unpack_table", boom)


def test_header_offsets_strides_and_permuted_properties(gold, reader, tmp_path):
    g, _ = gold
    h = reader.parse_header(_file(g, "permuted", tmp_path))
    assert h.format == "binary_little_endian" and [e.name for e in h.elements] == ["camera", "chunk", "vertex", "sh"]
    cam, chunk, vertex, sh = h.elements
    assert cam.stride == 12 and chunk.stride == 8 + 72 + 1 and vertex.stride == 4 + 2 + 4 + 4 + 1 + 4
    assert chunk.offset["max_b"] == 8 and chunk.offset["min_x"] == 8 + 4 * 17 and chunk.offset["tag"] == 80
    assert vertex.offset == {"packed_color": 0, "extra": 4, "packed_scale": 6, "packed_rotation": 10, "w": 14, "packed_position": 15}
    assert chunk.body_offset == h.header_bytes + 2 * 12 and vertex.body_offset == chunk.body_offset + 4 * 81
    assert sh.body_offset == vertex.body_offset + 1000 * 19 and sh.stride == 45
    assert h.refusal() is None
    lay = reader.layout_of(h)
    assert lay.chunk_stride == 81 and list(lay.vertex_offset) == [15, 10, 6, 0] and lay.n_sh == 45
    assert [lay.sh_offset[i] for i in range(45)] == [sh.offset[n] for n in sh.names()]


@pytest.mark.parametrize("fmt", ["ascii", "binary_big_endian"])
def test_ascii_and_big_endian_go_to_the_reference_or_are_refused(reader, lib, tmp_path, monkeypatch, fmt):
    _no_device(monkeypatch, lib)
    path = str(tmp_path / "a.ply")
    ch = np.zeros(1, [(f, "<f4") for f in crn.CHUNK_FIELDS])
    vt = np.zeros(3, [(f, "<u4") for f in crn.VERTEX_FIELDS])
    if fmt == "ascii":
        with open(path, "w") as f:
            f.write("ply\nformat ascii 1.0\nelement chunk 1\n" + "".join("property float %s\n" % n for n in crn.CHUNK_FIELDS)
                    + "element vertex 0\nproperty uint packed_position\nend_header\n" + " ".join(["0"] * 18) + "\n")
    else:
        crn.write_ply(path, [("chunk", ch), ("vertex", vt)], fmt)
    with pytest.raises(reader.UnsupportedPlyError, match=fmt):
        reader.read_compressed_ply(path)
    assert reader.read_compressed_ply(path, fallback=lambda p: ("ref", p)) == ("ref", path)


def test_list_property_and_no_chunk_element_go_to_the_reference(reader, lib, tmp_path, monkeypatch):
    _no_device(monkeypatch, lib)
    path = str(tmp_path / "l.ply")
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement chunk 0\nproperty float min_x\nelement face 1\n"
                b"property list uchar int vertex_indices\nelement vertex 0\nproperty uint packed_position\nend_header\n"
                b"\x03" + np.arange(3, dtype="<i4").tobytes())
    with pytest.raises(reader.UnsupportedPlyError, match="list property 'vertex_indices'"):
        reader.read_compressed_ply(path)
    assert reader.read_compressed_ply(path, fallback=lambda p: "ref") == "ref"
    path2 = str(tmp_path / "plain.ply")
    crn.write_ply(path2, [("vertex", np.zeros(2, [("x", "<f4")]))])
    with pytest.raises(reader.UnsupportedPlyError, match="no 'chunk' element"):
        reader.read_compressed_ply(path2)
    assert reader.read_compressed_ply(path2, fallback=lambda p: "ref") == "ref"
    path3 = str(tmp_path / "t.ply")
    crn.write_ply(path3, [("chunk", np.zeros(1, [(f, "<f8") for f in crn.CHUNK_FIELDS])), ("vertex", np.zeros(1, [(f, "<u4") for f in crn.VERTEX_FIELDS]))])
    with pytest.raises(reader.UnsupportedPlyError, match="property 'min_x' of element 'chunk' is f8"):
        reader.read_compressed_ply(path3)


def test_missing_properties_raise_numpys_error_before_device_work(gold, reader, lib, tmp_path, monkeypatch):
    g, spec = gold
    _no_device(monkeypatch, lib)
    errors = [n for n, r in spec.items() if "error" in r]
    assert len(errors) == 3
    for name in errors:
        seen = []
        with pytest.raises(ValueError) as e:
            reader.read_compressed_ply(_file(g, name, tmp_path), on_metadata=seen.append)
        assert "ValueError: " + str(e.value) == spec[name]["error"]
        assert seen == [spec[name]["metadata"]]
    rows, meta = reader.read_compressed_ply(_file(g, "missing_but_empty", tmp_path))
    assert len(rows) == 0 and meta == spec["missing_but_empty"]["metadata"]


def test_missing_vertex_element_is_plyfiles_key_error(reader, lib, tmp_path, monkeypatch):
    _no_device(monkeypatch, lib)
    path = str(tmp_path / "nv.ply")
    crn.write_ply(path, [("chunk", np.zeros(1, [(f, "<f4") for f in crn.CHUNK_FIELDS]))])
    with pytest.raises(KeyError):
        reader.read_compressed_ply(path)


def test_restatement_equals_every_golden_case(gold, tmp_path):
    g, spec = gold
    checked = 0
    for name, rec in spec.items():
        if "error" in rec:
            continue
        rows, meta = crn.read(_file(g, name, tmp_path))
        assert list(rows.dtype.names) == rec["names"] and meta == rec["metadata"], name
        if name + "__rows" in g:
            assert rows.tobytes() == g[name + "__rows"].tobytes(), name
        else:
            assert crn.sha(rows) == g[name + "__sha256"].tobytes(), name
        checked += 1
    assert checked == 14
    assert spec["edge_bounds"]["nan_rows"] == 1


def test_restatement_equals_every_wide_golden_case(gold_wide, tmp_path):
    g, spec = gold_wide
    checked = 0
    for name, rec in spec.items():
        assert "error" not in rec, name
        rows, meta = crn.read(_file(g, name, tmp_path))
        assert list(rows.dtype.names) == rec["names"] and meta == rec["metadata"], name
        assert [rows.dtype[f].str for f in rows.dtype.names] == rec["dtype"], name
        if name + "__rows" in g:
            assert rows.tobytes() == g[name + "__rows"].tobytes(), name
        else:
            assert crn.sha(rows) == g[name + "__sha256"].tobytes(), name
        checked += 1
    assert checked == 6
    assert sorted(len(r["names"]) - 17 for r in spec.values()) == [38, 89, 100, 192, 256, 257]
    assert spec["edge_bounds_sh100"]["nan_rows"] == 1 and spec["edge_bounds_sh100"]["metadata"]["chunks"] == 5
    assert spec["sh89_permuted"]["names"][17:] != ["f_rest_%d" % i for i in range(89)]
    assert sorted(spec["sh89_permuted"]["names"][17:]) == sorted("f_rest_%d" % i for i in range(89))
    assert not any(n.startswith("f_rest_") for n in spec["sh192_other_names"]["names"])


def _refused(reader, path, match):
    """`path` is refused for `match`: UnsupportedPlyError without a fallback, the fallback's result with one"""
    assert match in reader.parse_header(path).refusal()
    with pytest.raises(reader.UnsupportedPlyError, match=match):
        reader.read_compressed_ply(path)
    assert reader.read_compressed_ply(path, fallback=lambda p: ("ref", p)) == ("ref", path)


def test_257_sh_properties_go_to_the_reference_or_are_refused(gold_wide, reader, lib, tmp_path, monkeypatch):
    g, spec = gold_wide
    _no_device(monkeypatch, lib)
    path = _file(g, "sh257_refused", tmp_path)
    assert len(spec["sh257_refused"]["names"]) == 17 + 257
    assert reader.parse_header(path).refusal() == "257 sh properties (the device path reads up to 256)"
    _refused(reader, path, "257 sh properties")


def _with_sh_rows(path, n, chunks, sh_rows):
    ch = np.zeros(chunks, [(f, "<f4") for f in crn.CHUNK_FIELDS])
    vt = np.zeros(n, [(f, "<u4") for f in crn.VERTEX_FIELDS])
    crn.write_ply(path, [("chunk", ch), ("vertex", vt), ("sh", np.zeros(sh_rows, [("f_rest_%d" % i, "u1") for i in range(9)]))])
    return path


@pytest.mark.parametrize("n,chunks,sh_rows", [(300, 2, 299), (700, 2, 511), (300, 1, 0)])
def test_short_sh_element_goes_to_the_reference_or_is_refused(reader, lib, tmp_path, monkeypatch, n, chunks, sh_rows):
    """fewer sh rows than min(vertex.count, 256 x chunk.count), the rows the kernel decodes"""
    _no_device(monkeypatch, lib)
    path = _with_sh_rows(str(tmp_path / "s.ply"), n, chunks, sh_rows)
    assert reader.parse_header(path).refusal() == "an sh element of %d rows for %d vertices" % (sh_rows, n)
    _refused(reader, path, "an sh element of %d rows for %d vertices" % (sh_rows, n))


def test_sh_element_shorter_than_the_vertices_but_not_than_the_decoded_rows_is_taken(reader, lib, tmp_path, monkeypatch):
    path = _with_sh_rows(str(tmp_path / "s.ply"), 700, 2, 512)
    h = reader.parse_header(path)
    assert h.refusal() is None
    seen = {}

    def unpack(path_, segments, layout, n_chunks, n_vertices, dtype, stage_ms=None):
        seen.update(segments=segments, n_chunks=n_chunks, n_vertices=n_vertices, n_sh=layout.n_sh)
        return np.zeros(n_vertices, dtype)
    monkeypatch.setattr(lib, "cply_unpack_table", unpack)
    rows, meta = reader.read_compressed_ply(path, fallback=lambda p: pytest.fail("handed to the fallback"))
    assert meta == {"count": 700, "sh_degree": 1, "chunks": 2} and len(rows) == 700
    sh = h.element("sh")
    assert seen["segments"]["sh"] == (sh.body_offset, 9 * 512) and seen["segments"]["vertex"][1] == 16 * 512
    assert (seen["n_chunks"], seen["n_vertices"], seen["n_sh"]) == (2, 700, 9)


def test_layout_of_a_256_property_sh_element(gold_wide, reader, tmp_path):
    g, spec = gold_wide
    h = reader.parse_header(_file(g, "sh256", tmp_path))
    assert h.refusal() is None
    lay = reader.layout_of(h)
    assert lay.n_sh == 256 and lay.sh_stride == 256
    assert [lay.sh_offset[i] for i in range(256)] == list(range(256))
    assert h.element("sh").names() == spec["sh256"]["names"][17:] == ["f_rest_%d" % i for i in range(256)]
    assert lay.chunk_stride == 72 and lay.vertex_stride == 16 and list(lay.vertex_offset) == [0, 4, 8, 12]


def test_host_tables_are_numpys_results(lib):
    t = lib.cply_read_tables()
    d = t[:8 * 4352].view(np.float64)
    f = t[8 * 4352:].view(np.float32)
    u = np.arange(2048, dtype=np.uint32)
    assert np.array_equal(d[:2048].view(np.uint64), (u / 2047).view(np.uint64))
    assert np.array_equal(d[2048:3072].view(np.uint64), (u[:1024] / 1023).view(np.uint64))
    assert np.array_equal(d[3072:3328].view(np.uint64), (u[:256] / 255.0).view(np.uint64))
    assert np.array_equal(d[3328:].view(np.uint64), ((u[:1024] / 1023.0 - 0.5) / 0.7071067811865476).view(np.uint64))
    a = np.clip(u[:256] / 255.0, 1e-6, 1.0 - 1e-6)
    assert np.array_equal(f[:256].view(np.uint32), np.log(a / (1.0 - a)).astype(np.float32).view(np.uint32))
    assert np.array_equal(f[256:], ((np.arange(256, dtype=np.uint8) / 256.0 - 0.5) * 8.0).astype(np.float32))


_STANDIN = {
    "gsconverter/__init__.py": "",
    "gsconverter/processing/__init__.py": "from . import gpu_ops\nfrom .data_processor import DataProcessor\n",
    "gsconverter/processing/gpu_ops.py": "HAS_TAICHI = False\n",
    "gsconverter/processing/data_processor.py": "class DataProcessor:\n    def __init__(self, data):\n        self.data = data\n",
    "gsconverter/converter.py": "from .processing import DataProcessor\n",
    "gsconverter/formats/__init__.py": "",
    "gsconverter/formats/compressed_ply.py": ("class CompressedPlyFormat:\n    def read(self, path, **kw):\n        self.metadata = 'own'\n"
                                              "        return ('own', path, kw)\n    def write(self, data, path, **kw):\n        return 'w'\n"),
}


def test_install_rebinds_cply_read_on_a_stand_in_and_uninstall_restores_it(gsx, reader, tmp_path, monkeypatch):
    for rel, src in _STANDIN.items():
        (tmp_path / rel).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / rel).write_text(src)
    saved = {m: sys.modules.pop(m) for m in list(sys.modules) if m == "gsconverter" or m.startswith("gsconverter.")}
    mine = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    monkeypatch.setattr(mine, "_REFERENCE_CLASS", None)
    monkeypatch.syspath_prepend(str(tmp_path))
    try:
        import gsconverter.formats.compressed_ply as rcp
        own = rcp.CompressedPlyFormat.read
        calls = []

        def fake(path, stage_ms=None, fallback=None, on_metadata=None):
            calls.append(path)
            if path.endswith(".fb"):
                return fallback(path)
            on_metadata({"count": 3})
            return "mine", {"count": 3}
        monkeypatch.setattr(reader, "read_compressed_ply", fake)
        monkeypatch.setattr(reader, "plyfile_available", lambda: True)
        try:
            gsx.install(cply_reader=False)
            assert rcp.CompressedPlyFormat.read is own
            gsx.uninstall()
            gsx.install()
            assert rcp.CompressedPlyFormat.read is not own
            fmt = rcp.CompressedPlyFormat()
            assert fmt.read("a.compressed.ply") == "mine" and fmt.metadata == {"count": 3}
            fmt2 = rcp.CompressedPlyFormat()
            assert fmt2.read("b.fb", extra=1) == ("own", "b.fb", {"extra": 1}) and fmt2.metadata == "own"
            assert calls == ["a.compressed.ply", "b.fb"]
        finally:
            gsx.uninstall()
        assert rcp.CompressedPlyFormat.read is own
    finally:
        for m in [m for m in sys.modules if m == "gsconverter" or m.startswith("gsconverter.")]:
            del sys.modules[m]
        sys.modules.update(saved)
