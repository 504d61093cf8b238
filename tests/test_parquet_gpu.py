"""-m gpu: the Parquet reader's and writer's kernels on the device.  Through the _lib wrappers, with no pyarrow: every reader
case's chunk lists against the reference's rows, bit for bit; every writer case's table against the columns the reference's file
reads back as (values at valid slots, bitmaps, null counts); chunk lists with bit offsets 1, 7 and 9, a one-row chunk, both
ends of the stride range and 128 fields against the numpy restatement (tests/parquet_numpy.py, which the host tests tie to the
reference).  With pyarrow: write_parquet's file against the restatement's and the fixture's, read_parquet of the fixture's
files, a kernel stage for every non-empty case and none for n = 0, refusals reaching `fallback`, and install()'s bindings."""
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
ARROW_OF = {v: k for k, v in pqn.ARROW_TYPES.items()}
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return pqn.load_cases(GOLD)


@pytest.fixture(scope="module")
def lib():
    mod = importlib.import_module("3dgsconverter_amd._lib")
    mod.require_hip()
    return mod


@pytest.fixture(scope="module")
def reader():
    return importlib.import_module("3dgsconverter_amd.formats.parquet_reader")


@pytest.fixture(scope="module")
def writer():
    return importlib.import_module("3dgsconverter_amd.formats.parquet_writer")


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def case_plan(reader, c):
    meta = {b"pandas": json.dumps({"index_columns": [{"kind": "range", "name": None, "start": 0, "stop": c.n, "step": 1}], "columns": []}).encode()} if c.has_pandas else None
    return reader.plan(c.names, [ARROW_OF.get(t, "string") for t in c.types], meta)


def first_difference(got, want):
    if len(got) != len(want):
        return "%d bytes, %d expected" % (len(got), len(want))
    bad = np.nonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[0]
    return "%d bytes differ, first at byte %d" % (len(bad), bad[0])


def check_columns(data, fields, got):
    cols, bitmaps, nulls = got
    want_cols, want_bitmaps, want_nulls = pqn.split_columns(data, fields)
    assert nulls == want_nulls
    for k in range(len(fields)):
        assert same_bytes(cols[k], want_cols[k]), k
        assert (bitmaps[k] is None) == (want_bitmaps[k] is None) and (bitmaps[k] is None or same_bytes(bitmaps[k], want_bitmaps[k])), k


def test_every_reader_cases_chunks_give_the_references_rows(golden, reader, lib):
    _, readers, _ = golden
    for c in readers.values():
        p = case_plan(reader, c)
        assert p.refusal is None, c.name
        index_of = {name: k for k, name in enumerate(p.columns)}
        columns = [c.columns[c.names.index(name)] for name in p.columns]
        st = {}
        rows = lib.parquet_rows_table(columns, c.n, p.descriptors(index_of), p.dtype, stage_ms=st)
        assert rows.dtype == c.rows.dtype and same_bytes(rows, c.rows), c.name
        assert ("kernel" in st) == (c.n > 0), (c.name, st)


def test_every_writer_cases_table_gives_the_references_columns(golden, writer, lib):
    writers, _, _ = golden
    for c in writers.values():
        n = len(c.table)
        if n == 0:
            continue                                              # (no launch: write_parquet's business, below)
        p = writer.plan_write(c.table.dtype)
        st = {}
        cols, bitmaps, nulls = lib.parquet_columns_table(c.table, p.entries(), stage_ms=st)
        assert "kernel" in st, c.name
        assert nulls == [col["nulls"] for col in c.columns], c.name
        for col, values, bitmap, want in zip(p.columns, cols, bitmaps, c.columns):
            valid = want["valid"]
            assert (bitmap is None) == (col.kind == 0), (c.name, col.name)
            if bitmap is not None:
                assert same_bytes(bitmap, np.packbits(valid, bitorder="little")), (c.name, col.name)     # the bits past n are zero
            assert same_bytes(values.view(col.type)[valid], want["values"][valid]), (c.name, col.name)
        check_columns(c.table, p.entries(), (cols, bitmaps, nulls))                                      # NaN payloads: a bit copy


def test_chunks_at_bit_offsets_1_7_9_and_a_one_row_chunk(lib):
    rng = np.random.default_rng(5)
    n = 300
    specials = np.array([0xfff4000012345678, 0x7ff0000000000000, 0x8000000000000000], np.uint64).view(np.float64)
    vals = rng.standard_normal(n)
    vals[[0, 1, 70, 71, 199, 200, 299]] = specials[[0, 1, 2, 0, 1, 2, 0]]
    valid = rng.random(n) > 0.3
    valid[[0, 71, 299]] = True
    small = rng.integers(0, 255, n).astype(np.uint8)
    chunks, bytes_chunks, pos = [], [], 0
    for length, off in ((1, 1), (70, 7), (0, 3), (129, 9), (100, 0)):
        bits = np.zeros(off + length, bool)
        bits[off:] = valid[pos:pos + length]
        bits[:off] = rng.random(off) > 0.5                        # what lies ahead of the chunk is another chunk's business
        chunks.append((np.concatenate([np.full(off, 123.0), vals[pos:pos + length]])[off:], np.packbits(bits, bitorder="little"), off, length))
        bytes_chunks.append((small[pos:pos + length], None, off, length))
        pos += length
    dt = np.dtype([("a", "<f4"), ("b", "u1"), ("c", "<f4")])
    fields = [(0, pqn.CODES["f8"], 0, 4), (1, pqn.RAW, 4, 1), (1, pqn.CODES["u1"], 5, 4)]
    got = lib.parquet_rows_table([chunks, bytes_chunks], n, fields, dt)
    assert same_bytes(got, pqn.rows_from_descriptors([chunks, bytes_chunks], n, fields, dt))
    assert (got["a"].view(np.uint32)[~valid] == 0x7fc00000).all() and got["a"].view(np.uint32)[0] == 0xffe00000


@pytest.mark.parametrize("n", [65, 257])
def test_reader_strides_at_both_ends_and_128_fields(lib, n):
    rng = np.random.default_rng(n)
    types = ["i1", "u1", "i2", "u2", "i4", "u4", "f4", "f8", "i8", "u8", "f2"]

    def column(t, k):
        if t[0] == "f":
            v = (rng.integers(-40, 41, n) / 8.0).astype(t)
            v[rng.integers(0, n, 4)] = np.nan
        else:
            info = np.iinfo(t)
            v = rng.integers(info.min, info.max, n, dtype=t, endpoint=True)
        cut = sorted(rng.integers(0, n + 1, 2))
        valid = rng.random(n) > 0.2 if t[0] == "f" and k % 2 else None
        out = []
        for a, b in zip([0] + list(cut), list(cut) + [n]):
            out.append((v[a:b], None if valid is None else np.packbits(valid[a:b], bitorder="little"), 0, b - a))
        return out
    layouts = {"one byte a row": [("u1", True)],
               "128 fields, 512 bytes a row, tiles of 64 rows": [(types[k % 11], False) for k in range(127)] + [(None, False)],
               "257 bytes a row": [(types[k % 11], False) for k in range(64)] + [("u1", True)]}
    strides = []
    for name, layout in layouts.items():
        columns, fields, off = [], [], 0
        for k, (t, raw) in enumerate(layout):
            nb = 1 if raw else 4
            if t is None:                                         # a field without a source stays zero
                fields.append((None, pqn.CODES["f4"], off, nb))
            else:
                fields.append((len(columns), pqn.RAW if raw else pqn.CODES[t], off, nb))
                columns.append(column(t, k))
            off += nb
        dt = np.dtype({"names": ["f%d" % k for k in range(len(fields))], "formats": ["u1" if nb == 1 else "<f4" for _, _, _, nb in fields],
                       "offsets": [o for _, _, o, _ in fields], "itemsize": off})
        got = lib.parquet_rows_table(columns, n, fields, dt)
        assert same_bytes(got, pqn.rows_from_descriptors(columns, n, fields, dt)), name
        strides.append((off, len(fields)))
    assert strides == [(1, 1), (512, 128), (257, 65)]


@pytest.mark.parametrize("n", [65, 257])
def test_writer_strides_at_both_ends_and_128_fields(lib, n):
    rng = np.random.default_rng(100 + n)
    specials4 = np.array([0x7fc00000, 0x7fa12345, 0xffc00001, 0x7f800000, 0x80000000], np.uint32)
    for fields in ([("a", "u1")],
                   [("k", "u1")] + [("f%d" % i, ("<f4", "<f8", "<i2", "u1", "<u8", "u1", "<f4", "u1")[i % 8]) for i in range(127)],   # 128 fields, odd offsets
                   [("d%d" % i, "<f8") for i in range(64)]):                                                                   # 512 bytes
        dt = np.dtype(fields)
        assert dt.itemsize <= 512
        t = np.frombuffer(rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).tobytes(), dt).copy()
        for f in dt.names:
            if dt[f].kind == "f":
                t[f] = (rng.integers(-40, 41, n) / 8.0).astype(dt[f])
                rows = [r for r in (0, 63, 64, n - 1) if r < n]
                if dt[f].itemsize == 4:
                    t[f].view(np.uint32)[rows] = specials4[:len(rows)]
                else:
                    t[f][rows] = np.array([0xfff4000012345678, 0x7ff8000000000000, 0xfff0000000000000, 0x7ff0000000000001], np.uint64).view(np.float64)[:len(rows)]
        entries = [(dt.fields[f][1], dt[f].itemsize, pqn.kind_of(dt[f])) for f in dt.names]
        check_columns(t, entries, lib.parquet_columns_table(t, entries))
    assert dt.itemsize == 512


def test_a_column_that_is_all_nan_and_one_that_has_none(lib):
    n = 129
    t = np.zeros(n, [("a", "<f4"), ("b", "<f8"), ("c", "<f4")])
    t["a"], t["b"] = np.nan, 1.5
    cols, bitmaps, nulls = lib.parquet_columns_table(t, [(0, 4, 1), (4, 8, 2), (12, 4, 1)])
    assert nulls == [n, 0, 0] and not bitmaps[0].any() and same_bytes(bitmaps[1], np.packbits(np.ones(n, bool), bitorder="little"))


# ------------------------------------------------------------------------------------------------------------- with pyarrow

def test_written_file_is_the_restatements_file(golden, writer, tmp_path):
    pytest.importorskip("pyarrow")
    pytest.importorskip("pandas")
    writers, _, _ = golden
    for c in writers.values():
        a, b = str(tmp_path / "a.parquet"), str(tmp_path / "b.parquet")
        st = {}
        plan = writer.write_parquet(c.table, a, stage_ms=st)
        pqn.write_file(c.table, b)
        with open(a, "rb") as fa, open(b, "rb") as fb:
            got, want = fa.read(), fb.read()
        assert got == want, "%s: %s" % (c.name, first_difference(got, want))
        assert plan.refusal is None and ("kernel" in st) == (len(c.table) > 0) == ("upload" in st), (c.name, st)
        assert {"plan", "table", "encode_write"} <= set(st), (c.name, st)


def test_written_file_is_the_fixtures_file(golden, writer, tmp_path):
    pa = pytest.importorskip("pyarrow")
    pd = pytest.importorskip("pandas")
    writers, _, versions = golden
    if (pa.__version__, pd.__version__) != (versions["pyarrow"], versions["pandas"]):
        pytest.skip("the fixture's files were written by pyarrow %s and pandas %s; here are pyarrow %s and pandas %s, whose files differ"
                    % (versions["pyarrow"], versions["pandas"], pa.__version__, pd.__version__))
    for c in writers.values():
        path = str(tmp_path / "w.parquet")
        writer.write_parquet(c.table, path)
        with open(path, "rb") as f:
            got = f.read()
        assert got == c.file, "%s: %s" % (c.name, first_difference(got, c.file))


def test_read_parquet_of_the_fixtures_files_gives_the_references_rows(golden, reader, tmp_path):
    pytest.importorskip("pyarrow")
    _, readers, _ = golden
    for c in readers.values():
        path = str(tmp_path / "r.parquet")
        with open(path, "wb") as f:
            f.write(c.file)
        st = {}
        rows = reader.read_parquet(path, stage_ms=st)
        assert rows.dtype == c.rows.dtype and same_bytes(rows, c.rows), c.name
        assert ("kernel" in st) == (c.n > 0) == ("upload" in st) and "decode" in st, (c.name, st)


def test_refused_files_and_tables_reach_the_fallback(reader, writer, tmp_path):
    pa = pytest.importorskip("pyarrow")
    import pyarrow.parquet as pq
    path = str(tmp_path / "dup.parquet")
    pq.write_table(pa.table({"x": pa.array([1.0, 2.0]), "alpha": pa.array([0.5, 0.25]), "opacity": pa.array([0.1, 0.2])}), path)
    seen = []
    assert reader.read_parquet(path, fallback=lambda p: seen.append(p) or "rows") == "rows" and seen == [path]
    path = str(tmp_path / "nulls.parquet")
    pq.write_table(pa.table({"x": pa.array([1.0, 2.0]), "z": pa.array([1, None], pa.int32())}), path)
    assert reader.read_parquet(path, fallback=lambda p: seen.append(p) or "rows") == "rows" and seen[-1] == path
    with pytest.raises(reader.UnsupportedParquetError, match="integer column 'z' has 1 nulls"):
        reader.read_parquet(path)
    called = []
    table = np.zeros(3, [("x", "<f4"), ("h", "<f2")])
    plan = writer.write_parquet(table, str(tmp_path / "h.parquet"), fallback=lambda: called.append(1))
    assert called == [1] and "field 'h' is float16" in plan.refusal and not os.path.exists(str(tmp_path / "h.parquet"))


def test_install_binds_both_ends_and_uninstall_restores_them(gsx, golden, tmp_path, monkeypatch):
    """on a stand-in for the reference's package (it is not on this machine), the device underneath"""
    pa = pytest.importorskip("pyarrow")
    pytest.importorskip("pandas")
    import pyarrow.parquet as pq
    writers, readers, _ = golden
    mine = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    monkeypatch.setattr(mine, "_REFERENCE_CLASS", None)
    dup = str(tmp_path / "dup.parquet")
    pq.write_table(pa.table({"x": pa.array([1.0]), "alpha": pa.array([0.5]), "opacity": pa.array([0.1])}), dup)
    with pqn.standin_reference(tmp_path) as ParquetFormat:
        pqn.check_install(gsx, ParquetFormat, writers, readers, tmp_path, np.zeros(3, [("x", "<f4"), ("h", "<f2")]), dup)
