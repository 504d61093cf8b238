"""-m gpu: the ASCII bodies of the 3DGS / CloudCompare PLY readers on the device -- read_ply_3dgs / read_ply_cc with
ascii_body=True against the contract's oracle (tests/ply_text_numpy.py, which the host tests tie to the reference's own rows), bit
for bit: row counts around a wave, bodies that cross scan tiles and chunk windows, property counts 1 ... 66, every source type,
every separator and line end, camera elements on both sides, the hard set with its patched tokens, every binary golden case
rewritten as text, profile= and keep= against the binary twin, each structural refusal with its line, one converter run."""
import contextlib
import importlib
import io
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ply_read_numpy as pn  # noqa: E402
import ply_text_numpy as pt  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_BINARY = os.path.join(ROOT, "tests", "golden", "ply_read_ref.npz")
GOLD_TEXT = os.path.join(ROOT, "tests", "golden", "ply_text_ref.npz")
TILE = 4096                                            # csrc/ply_text.hip TXT_TILE
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgsconverter_amd._lib")


@pytest.fixture(scope="module")
def reader(lib):
    mod = importlib.import_module("3dgsconverter_amd.formats.ply_reader")
    lib.require_hip()
    return mod


def _read(reader, dialect):
    return reader.read_ply_3dgs if dialect == "3dgs" else reader.read_ply_cc


def _same(name, got, want):
    assert got.dtype == want.dtype, name
    a, b = np.ascontiguousarray(got).view(np.uint8).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert a.shape == b.shape, name
    bad = np.nonzero(a != b)[0]
    if len(bad):
        rb = got.dtype.itemsize
        row, col = bad[0] // rb, bad[0] % rb
        field = [f for f in got.dtype.names if got.dtype.fields[f][1] <= col][-1]
        raise AssertionError("%s: %d bytes differ, first at row %d field %s: %r != %r" % (name, len(bad), row, field, got[field][row], want[field][row]))


def _check(reader, name, path, dialects=("3dgs", "cc"), **kw):
    """both readers against the oracle -> the last read's stats"""
    st = {}
    for dialect in dialects:
        want, others = pt.read(path, dialect)
        st = {}
        rows, extras = _read(reader, dialect)(path, ascii_body=True, stats=st, **kw)
        _same("%s (%s)" % (name, dialect), rows, want)
        assert [e.name for e in extras] == [n for n, _ in others], name
        for e, (_, d) in zip(extras, others):
            assert e.data.dtype == d.dtype and e.data.tobytes() == d.tobytes(), (name, e.name)
    return st


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_row_counts_around_a_wave(reader, tmp_path, n):
    rng = np.random.default_rng(n)
    path = pt.write_arrays(str(tmp_path / "n.ply"), [("vertex", pn.build(n, pn.canonical_fields(3), rng))])
    st = _check(reader, "canonical %d" % n, path)
    assert st["tokens"] == 62 * n and st["host_tokens"] == 0 and st["chunks"] == 1
    path = pt.write_arrays(str(tmp_path / "x.ply"), [("vertex", pn.build(n, [("x", "f4")], rng))])       # one property a line
    assert _check(reader, "x alone %d" % n, path)["tokens"] == n


def _straddles(path, table, chunk_bytes):
    """does a token cross a scan tile's edge, a line a chunk window's edge, when the body is read in chunks of chunk_bytes?"""
    raw = open(path, "rb").read()
    body = raw[raw.index(b"end_header\n") + 11:]
    token_over_tile = line_over_window = False
    pos, windows = 0, 0
    while pos < len(body):
        win = body[pos:pos + chunk_bytes]
        cut = win.rfind(b"\n") + 1 if len(win) == chunk_bytes else len(win)
        line_over_window |= len(win) == chunk_bytes and cut < len(win)
        for edge in range(TILE, cut, TILE):
            token_over_tile |= win[edge - 1:edge].strip() != b"" and win[edge:edge + 1].strip() != b""
        pos, windows = pos + cut, windows + 1
    return token_over_tile, line_over_window, windows


def test_tiles_chunks_and_a_last_line_without_newline(reader, tmp_path):
    """59 properties, ~40 KB of text: ten scan tiles in one chunk, and five chunks of up to three tiles each with a small
    chunk_bytes; tokens over tile edges, lines over chunk windows, no newline at the end of the file"""
    rng = np.random.default_rng(5)
    fields = [f for f in pn.canonical_fields(3) if f[0] not in ("nx", "ny", "nz")]
    assert len(fields) == 59
    table = pn.build(70, fields, rng)
    path = pt.write_arrays(str(tmp_path / "t.ply"), [("vertex", table)], last_newline=False)
    over_tile, _, windows = _straddles(path, table, 1 << 30)
    assert over_tile and windows == 1 and os.path.getsize(path) > 3 * TILE
    assert _check(reader, "one chunk", path)["chunks"] == 1
    over_tile, over_window, windows = _straddles(path, table, 10000)
    assert over_tile and over_window and windows >= 3
    st = _check(reader, "five chunks", path, chunk_bytes=10000)
    assert st["chunks"] == windows and st["tokens"] == 70 * 59 and st["host_tokens"] == 0


def test_wide_rows_every_source_type_and_separators(reader, tmp_path):
    rng = np.random.default_rng(6)
    wide = pn.build(150, pn.canonical_fields(3) + [(c, "u1") for c in pn.COLOURS] + [("confidence", "f8")], rng)      # 62 + 3 + 1
    seps = lambda r, c: (" ", "\t", "   ", " \t\x0b\x0c ", "\r")[(r + c) % 5]     # noqa: E731
    for name, kw in (("plain", {}), ("crlf", dict(eol="\r\n")), ("crlf no end", dict(eol="\r\n", last_newline=False)),
                     ("blanks", dict(sep=seps, lead=lambda r: " \t"[: r % 3], trail=lambda r: "  \t"[: r % 4]))):
        path = pt.write_arrays(str(tmp_path / "w.ply"), [("vertex", wide)], **kw)
        assert _check(reader, name, path, chunk_bytes=30000)["host_tokens"] == 0
    mixed = [(f, pn.SOURCE_TYPES[k % 8]) for k, (f, _) in enumerate(pn.canonical_fields(3))]
    table = pn.build(130, mixed, rng)
    for k, (f, t) in enumerate(mixed):                   # the edge values of every type (a NaN's payload has no text)
        v = pn.edge_values(t, 130, seed=k)
        table[f] = np.where(np.isnan(v), 1, v) if t[0] == "f" else v
    path = pt.write_arrays(str(tmp_path / "m.ply"), [("vertex", table)], sep="\t")
    _check(reader, "every source type", path)
    cc = pn.build(90, pn.cc_fields(3), rng)
    camera = pn.build(3, [("fx", "f4"), ("fy", "f8"), ("id", "i4"), ("flag", "u1")], rng)
    path = pt.write_arrays(str(tmp_path / "c.ply"), [("camera", camera), ("vertex", cc), ("camera2", camera[:2])], eol="\r\n")
    _check(reader, "cameras on both sides", path, chunk_bytes=20000)
    path = pt.write_arrays(str(tmp_path / "z.ply"), [("vertex", cc[:0]), ("camera", camera)])
    rows, extras = reader.read_ply_cc(path, ascii_body=True)
    assert len(rows) == 0 and rows.dtype == pt.read(path, "cc")[0].dtype and extras[0].data.tobytes() == camera.tobytes()


def test_the_hard_set_is_patched_and_counted(reader, lib, tmp_path):
    toks = pt.hard_tokens()
    props = [("x", "f8"), ("y", "f4"), ("scalar_w", "f8")]
    rows = [[t, t, toks[-1 - k]] for k, t in enumerate(toks)]
    path = pt.write_text(str(tmp_path / "hard.ply"), [("vertex", props, rows)])
    st = _check(reader, "hard set", path)
    host = {}
    h = reader.parse_header(path)
    lib.ply_text_host(path, h.header_bytes, len(rows), props, stats=host)
    assert 0 < st["host_tokens"] == host["host_tokens"] < st["tokens"] // 2          # the device lists what its host twin lists
    few = _check(reader, "hard set in chunks", path, chunk_bytes=5000)
    assert few["chunks"] >= 3 and few["host_tokens"] == st["host_tokens"]
    # more listed tokens than the list holds (every token a subnormal): the host twin converts the chunk
    n = 6000
    sub = [["%de-320" % (k % 97 + 1), "1", "4.9e-324"] for k in range(n)]
    path = pt.write_text(str(tmp_path / "sub.ply"), [("vertex", props, sub)])
    st = _check(reader, "list overflow", path, dialects=("cc",), chunk_bytes=200_000)        # (room for 4291 listed tokens)
    assert st["host_tokens"] == 2 * n


def test_binary_golden_cases_rewritten_as_text(reader, tmp_path):
    g = np.load(GOLD_BINARY)
    spec = json.loads(bytes(g["spec"]).decode())
    done = 0
    for name, rec in spec.items():
        src = str(tmp_path / (name + ".ply"))
        open(src, "wb").write(g[name + "__file"].tobytes())
        if any("error" in r for r in rec["readers"].values()):
            continue
        elements = pn.parse(src)
        native = [(n, d.astype(d.dtype.newbyteorder("<"))) for n, d in elements]
        if not all(np.isfinite(d[f]).all() for _, d in native for f in d.dtype.names if d.dtype[f].kind == "f"):
            continue
        path = pt.write_arrays(str(tmp_path / (name + "_ascii.ply")), native)
        for dialect, r in rec["readers"].items():
            rows, extras = _read(reader, dialect)(path, ascii_body=True)
            assert list(rows.dtype.names) == r["names"] and [rows.dtype[f].str for f in rows.dtype.names] == r["dtype"], (name, dialect)
            assert rows.tobytes() == g["%s__%s__rows" % (name, dialect)].tobytes(), (name, dialect)
            assert [e.name for e in extras] == r["extra_elements"]
            done += 1
    assert done >= 20
    t = np.load(GOLD_TEXT)                               # ... and the ASCII golden file's own cases
    for name, rec in json.loads(bytes(t["spec"]).decode()).items():
        path = str(tmp_path / (name + "_t.ply"))
        open(path, "wb").write(t[name + "__file"].tobytes())
        for dialect, r in rec["readers"].items():
            st = {}
            rows, _ = _read(reader, dialect)(path, ascii_body=True, stats=st)
            assert rows.tobytes() == t["%s__%s__rows" % (name, dialect)].tobytes(), (name, dialect)
            assert name != "digits15" or st["host_tokens"] == 0
            assert name != "repr" or st["host_tokens"] <= st["tokens"] // 100


def test_profile_and_keep_equal_the_binary_twin(reader, lib, tmp_path):
    rng = np.random.default_rng(8)
    table = pn.build(300, pn.cc_fields(2), rng)
    binary = pn.write_ply(str(tmp_path / "b.ply"), [("vertex", table)])
    text = pt.write_arrays(str(tmp_path / "a.ply"), [("vertex", table)])
    for dialect in ("3dgs", "cc"):
        got = {}
        for kind, path, kw in (("binary", binary, {}), ("text", text, {"ascii_body": True, "chunk_bytes": 40000})):
            profile, keep = {}, {}
            rows, _ = _read(reader, dialect)(path, profile=profile, keep=keep, **kw)
            rr = keep.get("rows")
            assert rr is not None
            try:
                resident = rr.download() if hasattr(rr, "download") else None
            finally:
                rr.close()
            got[kind] = (rows, profile, resident)
        _same(dialect, got["text"][0], got["binary"][0])
        assert got["text"][1] == got["binary"][1] and got["text"][1]
        if got["binary"][2] is not None:
            assert np.asarray(got["text"][2]).tobytes() == np.asarray(got["binary"][2]).tobytes()
    assert lib.ResidentRows.open_count == 0


@pytest.mark.parametrize("kind", ["short", "long", "blank", "early_end"])
def test_structural_refusals_name_the_line(reader, tmp_path, kind):
    rng = np.random.default_rng(9)
    n = 120
    props, rows = pt.tokens_of(pn.build(n, pn.canonical_fields(3), rng))             # ~550 bytes a line: line 100 is in tile 13
    for at, chunk_bytes in ((0, None), (3, None), (100, None), (100, 9000), (n - 1, 9000)):
        broken = [list(r) for r in rows]
        if kind == "short":
            broken[at] = broken[at][:-1]
        elif kind == "long":
            broken[at] = broken[at] + ["1"]
        elif kind == "blank":
            broken[at] = []
        else:
            broken = broken[:at]
        path = pt.write_text(str(tmp_path / "bad.ply"), [("vertex", props, broken)])
        if kind == "early_end":
            raw = open(path, "rb").read().replace(b"element vertex %d\n" % at, b"element vertex %d\n" % n)
            open(path, "wb").write(raw)
        with pytest.raises(pt.Refused) as want:
            pt.parse(path)
        assert want.value.line == at + 1
        with pytest.raises(reader.UnsupportedPlyError) as e:
            reader.read_ply_3dgs(path, ascii_body=True, chunk_bytes=chunk_bytes)
        assert "element 'vertex'" in str(e.value) and re.search(r"line %d\b" % (at + 1), str(e.value)), (kind, at, str(e.value))
        assert reader.read_ply_cc(path, ascii_body=True, chunk_bytes=chunk_bytes, fallback=lambda q: ("fallback", q)) == ("fallback", path)
    # a token that is no number, in a later tile
    broken = [list(r) for r in rows]
    broken[100][7] = "1_0"
    path = pt.write_text(str(tmp_path / "tok.ply"), [("vertex", props, broken)])
    with pytest.raises(reader.UnsupportedPlyError, match="line 101, property %r" % props[7][0]):
        reader.read_ply_3dgs(path, ascii_body=True)


def test_converter_ascii_cc_to_splat_equals_the_binary_twin(lib, tmp_path):
    conv = importlib.import_module("3dgsconverter_amd.converter")
    rng = np.random.default_rng(10)
    table = pn.build(400, pn.cc_fields(3), rng)
    binary = pn.write_ply(str(tmp_path / "b.ply"), [("vertex", table)])
    text = pt.write_arrays(str(tmp_path / "a.ply"), [("vertex", table)], eol="\r\n")
    out = {}
    for kind, src in (("binary", binary), ("text", text)):
        dst = str(tmp_path / (kind + ".splat"))
        with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
            conv.Converter(src, dst, "splat", resident=True).run()
        out[kind] = open(dst, "rb").read()
    assert len(out["text"]) == 400 * 32 and out["text"] == out["binary"]
    assert lib.ResidentRows.open_count == 0
