"""-m "not gpu": the ASCII bodies of the 3DGS / CloudCompare PLY readers on the host -- the kernels' tokeniser and number code run
on the host (gsx_ply_text_host, csrc/dec_to_f64.h) against the contract's oracle in plain Python (tests/ply_text_numpy.py), bit
for bit; every entry of the certificate's power table against Python's integers; every refusal with its line through
read_ply_*(ascii_body=True); the golden file the reference's own readers made; the caps on what the host may settle."""
import ctypes as C
import importlib
import json
import os
import re
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ply_read_numpy as pn  # noqa: E402
import ply_text_numpy as pt  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ply_text_ref.npz")
WANTED_CASES = {"digits15", "repr", "cc_crlf", "camera_both_sides", "every_source_type"}


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return g, json.loads(bytes(g["spec"]).decode())


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgsconverter_amd._lib")


@pytest.fixture(scope="module")
def reader():
    return importlib.import_module("3dgsconverter_amd.formats.ply_reader")


def model_device(monkeypatch, lib, calls=None):
    """ply_text_table without a device: the same chunk loop over the kernels' host twin"""
    def refuse(*a, **k):
        raise AssertionError("the device was asked for")

    def model(path, body_offset, n, props, layout, dtype, stage_ms=None, device=0, stats=None, chunk_bytes=None, element="vertex", **kw):
        if calls is not None:
            calls.append((path, n))
        return lib.ply_text_host(path, body_offset, n, props, layout, dtype, stats=stats, chunk_bytes=chunk_bytes, element=element)
    monkeypatch.setattr(lib, "require_hip", refuse)
    monkeypatch.setattr(lib, "ply_text_table", model)


def _read(reader, dialect):
    return reader.read_ply_3dgs if dialect == "3dgs" else reader.read_ply_cc


def _same(got, want):
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


def _element_host(lib, path, stats=None, chunk_bytes=None):
    """the file's first element through the host twin, as the element's own rows"""
    h = importlib.import_module("3dgsconverter_amd.formats.ply_reader").parse_header(path)
    e = h.elements[0]
    return lib.ply_text_host(path, h.header_bytes, e.count, e.props, stats=stats, chunk_bytes=chunk_bytes, element=e.name)


def test_every_power_table_entry_against_python_integers(lib):
    L = lib.load()
    hi, lo, e2 = C.c_uint64(), C.c_uint64(), C.c_int32()
    for q in range(-342, 309):
        assert L.gsx_dec_pow5_entry(q, C.byref(hi), C.byref(lo), C.byref(e2)) == 0
        m = (hi.value << 64) | lo.value
        assert (1 << 127) <= m < (1 << 128), q
        # 5^q in [m, m + 1) * 2^e2, as integers
        if q >= 0:
            v = 5 ** q
            lo_end, hi_end = (m << e2.value, (m + 1) << e2.value) if e2.value >= 0 else (m, m + 1)
            v = v if e2.value >= 0 else v << -e2.value
            assert lo_end <= v < hi_end, q
            assert (0 <= q <= 55) == (v == lo_end), q
        else:
            assert m * 5 ** -q <= (1 << -e2.value) < (m + 1) * 5 ** -q, q
    assert L.gsx_dec_pow5_entry(309, C.byref(hi), C.byref(lo), C.byref(e2)) != 0 and L.gsx_dec_pow5_entry(-343, C.byref(hi), C.byref(lo), C.byref(e2)) != 0


def _bulk_tokens(n):
    rng = np.random.default_rng(11)
    f32 = rng.integers(0, 1 << 32, 2 * n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    f32 = f32[np.isfinite(f32)][:n]
    f64 = rng.integers(0, 1 << 64, 4 * n, dtype=np.uint64).view(np.float64)
    f64 = f64[np.isfinite(f64)]
    ints = rng.integers(-10 ** 9, 10 ** 9, n)
    as_float = [("%d.0", "%d.", "%de0", "%d.000", "%dE+2")[k % 5] % v for k, v in enumerate(ints.tolist())]
    cols = [["%.9g" % v for v in f32.tolist()], [repr(v) for v in f64[:n].tolist()], ["%.18e" % v for v in f64[n:2 * n].tolist()],
            ["%f" % v for v in f32.tolist()], as_float]
    props = [("a", "f4"), ("b", "f8"), ("c", "f8"), ("d", "f4"), ("e", "f8")]
    return props, [list(r) for r in zip(*cols)]


def test_float_tokens_bit_for_bit_against_python(lib, tmp_path):
    """>= 200 000 float tokens: %.9g of random-bit float32, repr of random-bit float64, %.18e, %f, integers written as floats"""
    props, rows = _bulk_tokens(41000)
    assert len(rows) * len(props) >= 200_000
    path = pt.write_text(str(tmp_path / "bulk.ply"), [("vertex", props, rows)])
    st = {}
    got = _element_host(lib, path, st)
    _same(got, pt.parse(path)[0][1])
    # %f of a large float32 has up to 39 digits and repr of a random-bit double is a subnormal once in 2048: a few go to the host
    assert st["tokens"] == len(rows) * len(props) and st["host_tokens"] <= st["tokens"] // 100, st
    # ... and in many chunks, wherever the cuts fall
    st2 = {}
    _same(_element_host(lib, path, st2, chunk_bytes=50_000), got)
    assert st2["chunks"] >= 3 and st2["tokens"] == st["tokens"] and st2["host_tokens"] == st["host_tokens"]


def test_number_code_alone_on_the_hard_set(lib):
    """gsx_dec_to_f64 token by token: what it answers is float()'s bits; what it leaves to the host is little"""
    L = lib.load()
    toks = pt.hard_tokens()
    left = 0
    for t in toks:
        b, raw = C.c_uint64(), t.encode()
        rc = L.gsx_dec_to_f64(raw, len(raw), C.byref(b))
        assert rc in (0, lib.DEC_FLAGGED), t
        if rc:
            left += 1
            continue
        assert b.value == struct.unpack("<Q", struct.pack("<d", float(t)))[0], t
    assert left < len(toks) // 2                       # exact midpoints, subnormal results: the host's; the rest is certified
    for t in pt.REFUSED_FLOAT_TOKENS:
        raw, b = t.encode("latin-1"), C.c_uint64()
        assert L.gsx_dec_to_f64(raw, len(raw), C.byref(b)) == lib.DEC_FLAGGED, t


def test_hard_set_as_a_file(lib, tmp_path):
    toks = pt.hard_tokens()
    props = [("d", "f8"), ("f", "f4"), ("g", "f8")]
    rows = [[t, t, toks[-1 - k]] for k, t in enumerate(toks)]
    path = pt.write_text(str(tmp_path / "hard.ply"), [("vertex", props, rows)])
    st = {}
    got = _element_host(lib, path, st)
    want = pt.parse(path)[0][1]
    _same(got, want)
    assert 0 < st["host_tokens"] < st["tokens"] // 2, st           # 1e-320 is the host's; most are not
    # double rounding shows: just above a float32 midpoint, the double is the midpoint and ties to even
    k = toks.index("1.00000005960464477539062500001")
    assert want["f"][k] == np.float32(1.0) and want["d"][k] == 1.0000000596046448


def test_every_property_type(lib, tmp_path):
    n = 256
    arr = np.zeros(n, [(t, ("<" + t) if t[1] != "1" else t) for t in pn.SOURCE_TYPES])
    for t in pn.SOURCE_TYPES:
        v = pn.edge_values(t, n)
        arr[t] = np.where(np.isnan(v), 0, v) if t[0] == "f" else v           # (a NaN's payload has no text)
    path = pt.write_arrays(str(tmp_path / "types.ply"), [("vertex", arr)])
    got = _element_host(lib, path)
    _same(got, pt.parse(path)[0][1])
    _same(got, arr)                                                          # %.9g / %.17g / %d round-trip every finite value
    for typ, toks in pt.ACCEPTED_INT_TOKENS.items():
        p = pt.write_text(str(tmp_path / "ok.ply"), [("vertex", [("v", typ)], [[t] for t in toks])])
        st = {}
        _same(_element_host(lib, p, st), pt.parse(p)[0][1])
        assert st["host_tokens"] == 0


def test_plan_without_the_keyword_still_refuses(reader, lib, tmp_path, monkeypatch):
    model_device(monkeypatch, lib)
    path = pt.write_arrays(str(tmp_path / "a.ply"), [("vertex", pn.build(5, pn.canonical_fields(1), np.random.default_rng(0)))])
    h = reader.parse_header(path)
    assert reader.plan(h, "3dgs").refusal == "an ascii body" and reader.plan(h, "cc").refusal == "an ascii body"
    p = reader.plan(h, "3dgs", ascii_body=True)
    assert p.refusal is None and p.ascii and not p.identity
    with pytest.raises(reader.UnsupportedPlyError, match="ascii"):
        reader.read_ply_3dgs(path)
    assert reader.read_ply_cc(path, fallback=lambda q: ("fallback", q)) == ("fallback", path)
    # the other refusals stay under the keyword
    listy = tmp_path / "list.ply"
    listy.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n1\n3 0 1 2\n")
    with pytest.raises(reader.UnsupportedPlyError, match="list property 'vertex_indices'"):
        reader.read_ply_3dgs(str(listy), ascii_body=True)
    wide = pt.write_text(str(tmp_path / "wide.ply"), [("vertex", [("p%d" % i, "f8") for i in range(65)], [["0"] * 65])])
    with pytest.raises(reader.UnsupportedPlyError, match="rows of 520 bytes"):
        reader.read_ply_3dgs(wide, ascii_body=True)


def _xyz_rows(n):
    return [["%d" % r, "%d.5" % r, "-%d" % r] for r in range(n)]


XYZ = [("x", "f4"), ("y", "f4"), ("z", "f4")]


def _broken(kind, n, at):
    """-> (rows of tokens, lines to drop at the end): n rows of x y z whose 0-based row `at` breaks the rules"""
    rows = _xyz_rows(n)
    if kind == "short":
        rows[at] = rows[at][:2]
    elif kind == "long":
        rows[at] = rows[at] + ["7"]
    elif kind == "blank":
        rows[at] = []
    elif kind == "blank_spaces":
        rows[at] = [" \t "]
    elif kind == "hash":
        rows[at] = ["#", "1", "2"]
    elif kind == "hash_glued":
        rows[at] = ["#1", "1", "2"]
    elif kind == "early_end":
        return rows[:at], None
    else:
        rows[at][1] = kind
    return rows, None


STRUCTURAL = ["short", "long", "blank", "blank_spaces", "hash", "hash_glued", "early_end"]


@pytest.mark.parametrize("chunk_bytes", [None, 64])
def test_every_refusal_names_its_line(reader, lib, tmp_path, monkeypatch, chunk_bytes):
    model_device(monkeypatch, lib)
    n = 40
    for kind in STRUCTURAL + pt.REFUSED_FLOAT_TOKENS[:-1]:
        for at in (0, 17, n - 1):
            rows, _ = _broken(kind, n, at)
            path = str(tmp_path / "bad.ply")
            pt.write_text(path, [("vertex", XYZ, rows)])
            if kind == "early_end":            # (the header still promises n rows)
                raw = open(path, "rb").read().replace(b"element vertex %d" % at, b"element vertex %d" % n)
                open(path, "wb").write(raw)
            with pytest.raises(pt.Refused) as want:
                pt.parse(path)
            assert want.value.line == at + 1 and want.value.element == "vertex"
            for dialect in ("3dgs", "cc"):
                with pytest.raises(reader.UnsupportedPlyError) as e:
                    _read(reader, dialect)(path, ascii_body=True, chunk_bytes=chunk_bytes)
                assert "element 'vertex'" in str(e.value) and re.search(r"line %d\b" % (at + 1), str(e.value)), (kind, at, str(e.value))
            assert reader.read_ply_3dgs(path, ascii_body=True, fallback=lambda q: ("fallback", q)) == ("fallback", path)
    # a bad token on an earlier line than a short line: the earlier line is named
    rows = _xyz_rows(n)
    rows[3][2], rows[9] = "1_0", rows[9][:1]
    path = pt.write_text(str(tmp_path / "two.ply"), [("vertex", XYZ, rows)])
    with pytest.raises(reader.UnsupportedPlyError, match="line 4, property 'z'"):
        reader.read_ply_3dgs(path, ascii_body=True, chunk_bytes=chunk_bytes)


def test_integer_refusals_and_other_elements(reader, lib, tmp_path, monkeypatch):
    model_device(monkeypatch, lib)
    for typ, toks in pt.REFUSED_INT_TOKENS.items():
        for t in toks:
            rows = [["1", "0"], ["2", t], ["3", "0"]]
            path = pt.write_text(str(tmp_path / "int.ply"), [("vertex", [("x", "f4"), ("scalar_k", typ)], rows)])
            with pytest.raises(pt.Refused) as want:
                pt.parse(path)
            assert want.value.line == 2
            with pytest.raises(reader.UnsupportedPlyError, match="line 2, property 'scalar_k'"):
                reader.read_ply_cc(path, ascii_body=True)
    # a camera element that breaks the rules is refused by its own name and line, before or behind `vertex`
    cam = [("fx", "f8"), ("id", "i4")]
    for order in (0, 1):
        els = [("camera", cam, [["1.5", "1"], ["2.5", "x"]]), ("vertex", XYZ, _xyz_rows(4))]
        path = pt.write_text(str(tmp_path / "cam.ply"), els[::-1] if order else els)
        with pytest.raises(reader.UnsupportedPlyError, match="element 'camera', line 2, property 'id'"):
            reader.read_ply_3dgs(path, ascii_body=True)


def test_separators_line_ends_and_empty_tables(reader, lib, tmp_path, monkeypatch):
    calls = []
    model_device(monkeypatch, lib, calls)
    rng = np.random.default_rng(3)
    table = pn.build(37, pn.cc_fields(1), rng)
    camera = pn.build(3, [("fx", "f4"), ("fy", "f8"), ("id", "i4"), ("flag", "u1")], rng)
    seps = lambda r, c: (" ", "\t", "   ", " \t\x0b\x0c ", "\r")[(r + c) % 5]     # noqa: E731
    variants = [dict(), dict(eol="\r\n"), dict(sep=seps, lead=lambda r: " \t"[: r % 3], trail=lambda r: "  \t"[: r % 4]),
                dict(last_newline=False), dict(eol="\r\n", last_newline=False, sep="\t")]
    for kw in variants:
        for els in ([("vertex", table)], [("camera", camera), ("vertex", table), ("camera2", camera[:1])]):
            path = pt.write_arrays(str(tmp_path / "v.ply"), els, **kw)
            for dialect in ("3dgs", "cc"):
                want, others = pt.read(path, dialect)
                for cb in (None, 700, 2000):
                    st = {}
                    rows, extras = _read(reader, dialect)(path, ascii_body=True, chunk_bytes=cb, stats=st)
                    _same(rows, want)
                    assert [e.name for e in extras] == [n for n, _ in others]
                    for e, (_, d) in zip(extras, others):
                        _same(e.data, d)
                    assert st["host_tokens"] == 0 and st["tokens"] == 37 * len(table.dtype.names) and (cb is None or st["chunks"] >= 3)
    assert calls
    # n = 0: the empty table without a launch, the elements behind it still read
    del calls[:]
    path = pt.write_arrays(str(tmp_path / "zero.ply"), [("vertex", table[:0]), ("camera", camera)])
    rows, extras = reader.read_ply_cc(path, ascii_body=True)
    assert len(rows) == 0 and rows.dtype == pt.read(path, "cc")[0].dtype and not calls
    _same(extras[0].data, camera)


def test_golden_cases_and_the_caps_on_the_host_list(gold, reader, lib, tmp_path, monkeypatch):
    g, spec = gold
    assert set(spec) == WANTED_CASES and os.path.getsize(GOLD) < 1_000_000
    model_device(monkeypatch, lib)
    stats = {}
    for name, rec in spec.items():
        path = str(tmp_path / (name + ".ply"))
        open(path, "wb").write(g[name + "__file"].tobytes())
        for dialect, r in rec["readers"].items():
            st = stats[name] = {}
            rows, extras = _read(reader, dialect)(path, ascii_body=True, stats=st)
            assert list(rows.dtype.names) == r["names"] and [rows.dtype[f].str for f in rows.dtype.names] == r["dtype"]
            assert rows.tobytes() == g["%s__%s__rows" % (name, dialect)].tobytes(), (name, dialect)
            assert [e.name for e in extras] == r["extra_elements"]
    assert stats["digits15"]["tokens"] == stats["repr"]["tokens"] == 100 * 62
    assert stats["digits15"]["host_tokens"] == 0                                   # at most 15 digits: every token is certified
    assert stats["repr"]["host_tokens"] <= stats["repr"]["tokens"] // 100          # 17 digits: the certificate leaves almost nothing
