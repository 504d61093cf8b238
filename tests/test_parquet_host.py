"""not gpu: the Parquet reader's and writer's host halves -- plan() and plan_write() against every golden case; the numpy
restatement (tests/parquet_numpy.py) against the rows and columns the reference's own codec recorded
(tests/golden/parquet_ref.npz); the kernels' cast and split code, run on the host (gsx_parquet_rows_host,
gsx_parquet_columns_host), against the same; each refusal with its reason; and, where the reference is mounted and pyarrow and
pandas are the recorded versions, the restatement's file against the reference's file, byte for byte; install()'s two switches,
their bound methods and uninstall() on a stand-in for the reference's package, the kernels' host twins underneath."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parquet_numpy as pqn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "parquet_ref.npz")
COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 257)
ARROW_OF = {v: k for k, v in pqn.ARROW_TYPES.items()}


@pytest.fixture(scope="module")
def golden():
    return pqn.load_cases(GOLD)


@pytest.fixture(scope="module")
def reader():
    return importlib.import_module("3dgsconverter_amd.formats.parquet_reader")


@pytest.fixture(scope="module")
def writer():
    return importlib.import_module("3dgsconverter_amd.formats.parquet_writer")


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgsconverter_amd._lib")


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def case_plan(reader, c):
    """plan() of a reader case, from the recorded schema alone (a type the fixture could not decode is a string column)"""
    meta = {b"pandas": json.dumps({"index_columns": [{"kind": "range", "name": None, "start": 0, "stop": c.n, "step": 1}], "columns": []}).encode()} if c.has_pandas else None
    return reader.plan(c.names, [ARROW_OF.get(t, "string") for t in c.types], meta)


def case_columns(c, p):
    """the chunk lists of the plan's columns, in the plan's order, and the descriptors over them"""
    index_of = {name: k for k, name in enumerate(p.columns)}
    return [c.columns[c.names.index(name)] for name in p.columns], p.descriptors(index_of)


def test_the_fixture_holds_the_cases_the_kernels_edges_need(golden):
    writers, readers, versions = golden
    assert {"pyarrow", "pandas"} <= set(versions)
    assert {len(writers["w_n%d" % n].table) for n in COUNTS} == set(COUNTS)
    assert {readers["r_groups50_n%d" % n].n for n in COUNTS} == set(COUNTS)
    assert writers["w_canonical_1000"].table.dtype.itemsize == 248 and writers["w_rgb_extras_300"].table.dtype.itemsize == 251 + 22
    assert "nx" not in writers["w_no_nx_holes_130"].table.dtype.names and writers["w_wide_200"].table.dtype.itemsize > 256
    big = writers["w_canonical_1000"]
    nulls = {col["name"]: col["nulls"] for col in big.columns}
    assert nulls["r_sh8"] == 1000 and nulls["y"] == 0 and 0 < nulls["x"] < 1000          # all NaN (f_rest_7), none, some
    assert any(col["type"] == "f8" and col["nulls"] for col in writers["w_rgb_extras_300"].columns)
    d = readers["r_direct_1000"]
    assert not d.has_pandas and {"f8", "f2", "i8", "u8", None} <= set(d.types) and "nx" not in d.names
    assert max(len(ch) for ch in d.columns.values()) == 10                               # row groups of 100
    x = np.concatenate([v for v, _, _, _ in d.columns[d.names.index("x")]])
    assert 0xfff4000012345678 in x.view(np.uint64)
    assert readers["r_rgb_extras_300"].rows.dtype.itemsize == 251 and readers["r_canonical_1000"].rows.dtype.itemsize == 248


def test_restatement_reads_the_references_rows(golden):
    _, readers, _ = golden
    for c in readers.values():
        rows = pqn.read_rows(c.names, c.types, c.columns, c.n)
        assert rows.dtype == c.rows.dtype and same_bytes(rows, c.rows), c.name


def test_plan_gives_the_references_dtype_and_sources(golden, reader):
    _, readers, _ = golden
    for c in readers.values():
        p = case_plan(reader, c)
        assert p.refusal is None and p.dtype == c.rows.dtype, (c.name, p.refusal)
        _, listed = pqn.read_plan(c.names, c.types)
        assert [(f.name, f.source) for f in p.fields] == listed, c.name
        assert p.columns == [n for n in c.names if n in {s for _, s in listed}], c.name
        assert all(f.src_type == c.types[c.names.index(f.source)] for f in p.fields if f.source), c.name


def test_kernel_casts_on_the_host_give_the_references_rows(golden, reader, lib):
    _, readers, _ = golden
    for c in readers.values():
        p = case_plan(reader, c)
        columns, fields = case_columns(c, p)
        rows = lib.parquet_rows_host(columns, c.n, fields, p.dtype)
        assert same_bytes(rows, c.rows), c.name


def test_restatement_splits_the_references_columns(golden):
    writers, _, _ = golden
    for c in writers.values():
        cols = pqn.write_columns(c.table)
        assert [(n, t) for n, t, _, _, _ in cols] == [(col["name"], col["type"]) for col in c.columns], c.name
        for (name, t, col, bitmap, nulls), want in zip(cols, c.columns):
            n = len(c.table)
            assert nulls == want["nulls"], (c.name, name)
            valid = np.unpackbits(bitmap, bitorder="little")[:n].astype(bool) if bitmap is not None else np.ones(n, bool)
            assert (valid == want["valid"]).all(), (c.name, name)
            assert same_bytes(col.view(t)[valid], want["values"][valid]), (c.name, name)


def test_plan_write_gives_the_references_columns(golden, writer):
    writers, _, _ = golden
    for c in writers.values():
        p = writer.plan_write(c.table.dtype)
        assert p.refusal is None, (c.name, p.refusal)
        assert [(col.name, col.type) for col in p.columns] == [(col["name"], col["type"]) for col in c.columns], c.name
        assert [(col.name, col.source) for col in p.columns] == pqn.write_plan(c.table.dtype), c.name
        assert all(col.kind == pqn.kind_of(col.type) and col.src_offset == c.table.dtype.fields[col.source][1] for col in p.columns)


def test_kernel_split_on_the_host_gives_the_restatements_columns(golden, writer, lib):
    writers, _, _ = golden
    for c in writers.values():
        p = writer.plan_write(c.table.dtype)
        cols, bitmaps, nulls = lib.parquet_columns_host(c.table, p.entries())
        want_cols, want_bitmaps, want_nulls = pqn.split_columns(c.table, p.entries())
        assert nulls == want_nulls == [col["nulls"] for col in c.columns], c.name
        for k in range(len(cols)):
            assert same_bytes(cols[k], want_cols[k]), (c.name, k)
            assert (bitmaps[k] is None) == (want_bitmaps[k] is None) and (bitmaps[k] is None or same_bytes(bitmaps[k], want_bitmaps[k])), (c.name, k)


def test_chunk_lists_with_any_bit_offset_on_the_host(lib):
    """bit offsets 1, 7 and 9, a one-row chunk, an empty chunk: the re-packed bitmap is the rows' own"""
    rng = np.random.default_rng(5)
    n = 300
    vals = rng.standard_normal(n)
    valid = rng.random(n) > 0.3
    chunks, pos = [], 0
    for length, off in ((1, 1), (70, 7), (0, 3), (129, 9), (100, 0)):
        bits = np.zeros(off + length, bool)
        bits[off:] = valid[pos:pos + length]
        bits[:off] = rng.random(off) > 0.5                      # what lies ahead of the chunk is another chunk's business
        lead = np.full(off, 123.0)
        chunks.append((np.concatenate([lead, vals[pos:pos + length]])[off:], np.packbits(bits, bitorder="little"), off, length))
        pos += length
    assert pos == n
    dt = np.dtype([("a", "<f4"), ("b", "u1")])
    fields = [(0, pqn.CODES["f8"], 0, 4), (None, pqn.RAW, 4, 1)]
    got = lib.parquet_rows_host([chunks], n, fields, dt)
    want = pqn.rows_from_descriptors([chunks], n, fields, dt)
    assert same_bytes(got, want)
    assert (got["a"].view(np.uint32)[~valid] == 0x7fc00000).all() and same_bytes(got["a"][valid], vals[valid].astype("f4"))


def test_read_refusals_carry_their_reason(reader):
    base = ["x", "y", "z", "alpha"]
    f4 = ["float"] * 4

    def why(names, types, meta=None):
        return reader.plan(names, types, meta).refusal or ""
    assert why(base, f4) == ""
    assert "'alpha', 'opacity' all land on 'opacity'" in why(base + ["opacity"], f4 + ["float"])
    assert "'x', 'x' all land on 'x'" in why(base + ["x"], f4 + ["float"])
    assert "column 'alpha' is string" in why(base, ["float"] * 3 + ["string"])
    assert "column 'z' is bool" in why(base, ["float", "float", "bool", "float"])
    assert why(base + ["label"], f4 + ["string"]) == ""                                   # an unused column may be anything
    assert "column 'red' is int32" in why(base + ["red"], f4 + ["int32"])
    meta = {b"pandas": json.dumps({"index_columns": ["__index_level_0__"], "columns": []}).encode()}
    assert "stores the index in column '__index_level_0__'" in why(base + ["__index_level_0__"], f4 + ["int64"], meta)
    meta = {b"pandas": json.dumps({"index_columns": [], "columns": [{"name": "z", "field_name": "z", "numpy_type": "Int64"}]}).encode()}
    assert "restores column 'z' (int64) as Int64" in why(base, ["float", "float", "int64", "float"], meta)
    p = reader.plan(base + ["red"], ["float", "float", "int64", "float", "uint8"])
    assert p.refusal is None
    assert "integer column 'z' has 3 nulls" in reader.refuse_integer_nulls(p, {"z": 3, "x": 5}).refusal
    p = reader.plan(base + ["red"], f4 + ["uint8"])
    assert "integer column 'red' has 1 nulls" in reader.refuse_integer_nulls(p, {"red": 1}).refusal
    assert reader.refuse_integer_nulls(reader.plan(base, f4), {"x": 5}).refusal is None   # nulls in a float column are the kernel's


def test_read_limits_are_refusals(reader, monkeypatch):
    monkeypatch.setattr(reader, "MAX_STRIDE", 200)
    assert "rows of 248 bytes" in reader.plan(["x"], ["float"]).refusal
    monkeypatch.setattr(reader, "MAX_STRIDE", 512)
    monkeypatch.setattr(reader, "MAX_FIELDS", 61)
    assert "62 output fields" in reader.plan(["x"], ["float"]).refusal


def test_write_refusals_carry_their_reason(writer):
    base = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]

    def why(fields):
        return writer.plan_write(np.dtype(fields)).refusal or ""
    assert why(base) == ""
    assert "field 'b' is bool" in why(base + [("b", "?")])
    assert "field 'h' is float16" in why(base + [("h", "<f2")])
    assert "field 's' is |S4" in why(base + [("s", "S4")])
    assert "field 'v' is" in why(base + [("v", "<f4", (3,))])
    assert "field 'e' is big-endian" in why(base + [("e", ">f4")])
    assert "fields 'opacity' and 'alpha' both land on column 'alpha'" in why(base + [("opacity", "<f4"), ("alpha", "<f4")])
    assert "rows of 516 bytes" in why(base + [("t%d" % i, "<f8") for i in range(63)])
    assert "129 columns" in why(base + [("t%d" % i, "u1") for i in range(126)])
    # ny without nx: a target of the mapping and not in the order -- dropped, as the reference drops it
    assert [c.name for c in writer.plan_write(np.dtype(base + [("ny", "<f4"), ("k", "<i4")])).columns] == ["x", "y", "z", "k"]


def test_restatements_file_is_the_references_file(golden, tmp_path):
    writers, _, versions = golden
    pa = pytest.importorskip("pyarrow")
    pd = pytest.importorskip("pandas")
    if (pa.__version__, pd.__version__) != (versions["pyarrow"], versions["pandas"]):
        pytest.skip("the fixture was written by pyarrow %s and pandas %s, here are %s and %s" % (versions["pyarrow"], versions["pandas"], pa.__version__, pd.__version__))
    for c in writers.values():
        path = str(tmp_path / (c.name + ".parquet"))
        pqn.write_file(c.table, path)
        with open(path, "rb") as f:
            assert f.read() == c.file, c.name


def test_restatements_file_is_the_live_references_file(golden, tmp_path):
    try:
        from oracle import refload
        ok = refload.available()
    except ImportError:
        ok = False
    if not ok:
        pytest.skip("the reference is not mounted")
    pytest.importorskip("pyarrow")
    pytest.importorskip("pandas")
    refload.load()
    from gsconverter.formats.parquet import ParquetFormat  # type: ignore
    writers, _, _ = golden
    for name in ("w_n0", "w_n65", "w_rgb_extras_300", "w_no_nx_holes_130"):
        c = writers[name]
        a, b = str(tmp_path / "a.parquet"), str(tmp_path / "b.parquet")
        pqn.write_file(c.table, a)
        write = getattr(ParquetFormat.write, "__wrapped__", ParquetFormat.write)
        with np.errstate(all="ignore"):
            write(ParquetFormat(), c.table, b)
        with open(a, "rb") as fa, open(b, "rb") as fb:
            assert fa.read() == fb.read(), name


def _model_device(monkeypatch, lib):
    """the two table wrappers without a device: the kernels' own cast and split code on the host"""
    def rows_table(columns, n, fields, dtype, stage_ms=None, device=0):
        return lib.parquet_rows_host(columns, n, fields, dtype)

    def columns_table(data, fields, stage_ms=None, device=0, consume=None):
        got = lib.parquet_columns_host(data, fields)
        return consume(*got) if consume is not None else got
    monkeypatch.setattr(lib, "parquet_rows_table", rows_table)
    monkeypatch.setattr(lib, "parquet_columns_table", columns_table)


def test_install_binds_both_ends_on_a_stand_in_and_uninstall_restores_them(gsx, golden, lib, tmp_path, monkeypatch):
    pa = pytest.importorskip("pyarrow")
    pytest.importorskip("pandas")
    import pyarrow.parquet as pq
    writers, readers, _ = golden
    mine = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    monkeypatch.setattr(mine, "_REFERENCE_CLASS", None)
    _model_device(monkeypatch, lib)
    dup = str(tmp_path / "dup.parquet")
    pq.write_table(pa.table({"x": pa.array([1.0]), "alpha": pa.array([0.5]), "opacity": pa.array([0.1])}), dup)
    with pqn.standin_reference(tmp_path) as ParquetFormat:
        pqn.check_install(gsx, ParquetFormat, writers, readers, tmp_path, np.zeros(3, [("x", "<f4"), ("h", "<f2")]), dup)


def test_a_path_whose_schema_cannot_be_read_goes_to_the_fallback(reader, tmp_path):
    pytest.importorskip("pyarrow")
    d = str(tmp_path / "dataset_dir")
    os.makedirs(d)
    assert reader.read_parquet(d, fallback=lambda p: ("reference", p)) == ("reference", d)
    with pytest.raises(Exception):
        reader.read_parquet(d)


def test_bound_write_keeps_the_converters_kwargs_away_from_write_parquet(writer, monkeypatch):
    seen = {}
    monkeypatch.setattr(writer, "write_parquet", lambda data, path, **kw: seen.update(kw))
    bound = writer.bind_write(lambda self, data, path, **kw: ("own", sorted(kw)))
    bound(object(), "table", "p", device=3, stage_ms=1, fallback=2)
    assert set(seen) == {"fallback"} and seen["fallback"]() == ("own", ["device", "fallback", "stage_ms"])
