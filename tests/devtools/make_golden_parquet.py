"""Build tests/golden/parquet_ref.npz from the REFERENCE's own Parquet codec (build box only: needs the reference, pandas and
pyarrow).  The reference's ``ParquetFormat.write`` and ``ParquetFormat.read`` (formats/parquet.py) run unchanged.

  writer cases   the table's raw rows (every byte, holes included, and its dtype), the reference file's bytes, the pyarrow and
                 pandas versions that made it, and the file read back with pq.read_table: column names in order, types,
                 validity, null counts and the values at valid slots (the others zeroed)
  reader cases   the file's bytes, the chunk lists exactly as pq.read_table returned them here (values from the chunk's offset
                 on, the validity bitmap as it lies in memory, the offset, the length), and the rows of the reference's read.
                 Files the reference wrote, and files written by pyarrow directly: the reference reads any parquet file, and
                 only so do row groups get small (chunk ends inside tiles and inside bitmap bytes), sources get to be f64,
                 f16 and the integers, columns go missing or unused, and the pandas metadata is absent.

Values come from small pools, so that the dictionary pages and the npz's deflate keep the fixture small: the transposes and
the bitmaps under test do not care what the bits are, the planted specials do the rest.

    python tests/devtools/make_golden_parquet.py
"""
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import parquet_numpy as pqn  # noqa: E402
from oracle import refload  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "parquet_ref.npz")
COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 257)
F4_SPECIALS = np.array([0x7fc00000, 0x7f800000, 0xff800000, 0x80000000, 0x7fa12345, 0xffc00001], np.uint32).view(np.float32)
F8_SPECIALS = np.array([0x7ff8000000000000, 0x7ff0000000000000, 0xfff0000000000000, 0x8000000000000000, 0xfff4000012345678, 0x7ff8000000000001],
                       np.uint64).view(np.float64)
NO_NAN = {"y", "scale_1", "f_rest_3", "f_dc_1"}          # columns that get no NaN (+-inf and -0.0 only): no bitmap in the file
ALL_NAN = {"f_rest_7", "scale_0"}                        # columns that are NaN in every row


def special_rows(n):
    """the first and last row of a 64-bit bitmap word, of a 128-row tile, and of the table"""
    return sorted({r for r in (0, 63, 64, 127, 128, 191, 192, 255, 256, n - 1) if 0 <= r < n})


def build(n, dtype, rng):
    """a table of `dtype` with values from small pools and the specials planted at special_rows()"""
    dtype = np.dtype(dtype)
    t = np.zeros(n, dtype)
    t.view(np.uint8).reshape(n, dtype.itemsize)[:] = 0xA5 if n else 0            # the holes hold something
    for j, f in enumerate(dtype.names):
        ft = dtype[f]
        if ft.kind == "f":
            t[f] = (rng.integers(-3, 4, n) / 2.0).astype(ft)
            sp = F4_SPECIALS if ft.itemsize == 4 else F8_SPECIALS
            if f in NO_NAN:
                sp = sp[1:4]
            for i, r in enumerate(special_rows(n)):
                t[f][r] = sp[(i + j) % len(sp)]
            if f in ALL_NAN:
                t[f] = sp[0]
        else:
            info = np.iinfo(ft)
            t[f] = rng.integers(0, 8, n).astype(ft)
            for i, r in enumerate(special_rows(n)):
                t[f][r] = (info.min, info.max, 0)[(i + j) % 3]
    return t


def reference_format():
    refload.load()
    from gsconverter.formats.parquet import ParquetFormat  # type: ignore
    return ParquetFormat()


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def writer_case(name, table, tmp, arrays):
    import pyarrow.parquet as pq
    path = os.path.join(tmp, name + ".parquet")
    with quiet(), np.errstate(all="ignore"):
        reference_format().write(table, path)
    with open(path, "rb") as f:
        data = f.read()
    arrays[name + "/table"] = np.frombuffer(table.tobytes(), np.uint8)
    arrays[name + "/file"] = np.frombuffer(data, np.uint8)
    back = pq.read_table(path)
    cols = []
    for k, field in enumerate(back.schema):
        col = back.column(k).combine_chunks()
        valid = np.asarray(col.is_valid().to_numpy(zero_copy_only=False), bool) if len(col) else np.zeros(0, bool)
        code = pqn.ARROW_TYPES[str(field.type)]
        values = np.asarray(col.fill_null(0).to_numpy(zero_copy_only=False)).astype(code) if len(col) else np.zeros(0, code)
        cols.append({"name": field.name, "type": code, "nulls": int(col.null_count)})
        arrays["%s/rb%d/values" % (name, k)] = values
        if col.null_count:
            arrays["%s/rb%d/valid" % (name, k)] = np.packbits(valid, bitorder="little")
    return {"name": name, "dtype": pqn.dtype_to_json(table.dtype), "columns": cols}, path


def reader_case(name, path, arrays, file_of=None):
    import pyarrow as pa
    import pyarrow.parquet as pq
    with open(path, "rb") as f:
        data = f.read()
    with quiet(), np.errstate(all="ignore"):
        rows = reference_format().read(path)
    table = pq.read_table(path)
    names, types, chunks = [], [], {}
    for k, field in enumerate(table.schema):
        code = pqn.ARROW_TYPES.get(str(field.type))
        names.append(field.name)
        types.append(code)
        if code is None:
            continue
        lst, vals, vbytes = [], [], []
        for a in table.column(k).chunks:
            validity, body = a.buffers()[:2]
            off, ln = a.offset, len(a)
            vals.append(np.frombuffer(body, code, count=off + ln)[off:] if ln else np.zeros(0, code))
            vlen = -1
            if validity is not None:
                vlen = (off + ln + 7) // 8
                vbytes.append(np.frombuffer(validity, np.uint8)[:vlen])
            lst.append([ln, off, vlen])
        chunks[str(k)] = lst
        arrays["%s/c%d/values" % (name, k)] = np.concatenate(vals) if vals else np.zeros(0, code)
        if vbytes:
            arrays["%s/c%d/validity" % (name, k)] = np.concatenate(vbytes)
    if file_of is None:                       # (a writer case's file is stored once, with that case)
        arrays[name + "/file"] = np.frombuffer(data, np.uint8)
    arrays[name + "/rows"] = np.frombuffer(rows.tobytes(), np.uint8)
    return {"name": name, "n": int(table.num_rows), "names": names, "types": types, "chunks": chunks, "dtype": pqn.dtype_to_json(rows.dtype), "file_of": file_of,
            "has_pandas": b"pandas" in (table.schema.metadata or {})}


def small_frame(n, rng):
    """a pandas frame for the row-count cases: f4 and f8 sources with NaN (nulls in the file), an i4, uint8 colours, a column the
    rows do not use; nx ny nz and most of the rest are missing"""
    import pandas as pd
    t = build(n, [("x", "<f4"), ("y", "<f8"), ("z", "<f4"), ("alpha", "<f4"), ("cov_s0", "<f8"), ("r_sh0", "<i4"), ("red", "u1"), ("green", "u1"),
                  ("blue", "u1"), ("unused", "<f4"), ("b_sh15", "<f4")], rng)
    return pd.DataFrame({f: t[f] for f in t.dtype.names})


def direct_table(n, rng):
    """a pa.Table with no pandas metadata: f64 (the sNaN among its values, not null), f16, int64, the other integers, explicit
    nulls in the float columns, an unused string column, a name the mapping does not know (f_rest_44), missing columns"""
    import pyarrow as pa
    rows = special_rows(n)
    null_at = np.zeros(n, bool)
    null_at[[r for r in rows[1::2]]] = True
    null_at[rng.integers(0, n, n // 16)] = True

    def floats(t, specials):
        v = (rng.integers(-3, 4, n) / 2.0).astype(t)
        for i, r in enumerate(rows):
            v[r] = specials[i % len(specials)]
        return v

    def ints(t, extra=()):
        info = np.iinfo(t)
        v = rng.integers(0, 8, n).astype(t)
        pool = [info.min, info.max, 0] + list(extra)
        for i, r in enumerate(rows):
            v[r] = pool[i % len(pool)]
        return v
    f2_specials = np.array([0x7e00, 0x7c00, 0xfc00, 0x8000, 0x7e01, 0xfd55, 0x0001, 0x83ff], np.uint16).view(np.float16)
    cols = {
        "x": pa.array(floats("f8", F8_SPECIALS), mask=null_at),
        "y": pa.array(floats("f2", f2_specials), mask=np.roll(null_at, 1)),
        "z": pa.array(ints("i8", (2 ** 53 + 1, -(2 ** 53) - 1, 16777217, 2 ** 62 + 2 ** 38))),
        "ny": pa.array(floats("f4", F4_SPECIALS), mask=np.roll(null_at, 2)),
        "alpha": pa.array(ints("i4", (16777217, -16777219))),
        "r_sh0": pa.array(ints("u2")),
        "g_sh0": pa.array(ints("u8", (2 ** 53 + 1, 2 ** 63 + 2 ** 39, 2 ** 64 - 2 ** 39 - 1))),
        "b_sh0": pa.array(ints("i1")),
        "cov_s0": pa.array(ints("u4", (16777217, 2 ** 32 - 129))),
        "cov_s1": pa.array(ints("i2")),
        "cov_s2": pa.array(ints("u1")),
        "label": pa.array(["s%d" % (i % 3) for i in range(n)]),
        "f_rest_44": pa.array(floats("f4", F4_SPECIALS)),
        "red": pa.array(ints("u1")), "green": pa.array(ints("u1")), "blue": pa.array(ints("u1")),
    }
    for q in range(4):
        cols["cov_q%d" % q] = pa.array(floats("f4", F4_SPECIALS), mask=np.roll(null_at, 3 + q))
    for i in (1, 2, 15):
        cols["g_sh%d" % i] = pa.array(floats("f8", F8_SPECIALS))
    return pa.table(cols)


def main():
    import pandas as pd
    import pyarrow as pa
    import pyarrow.parquet as pq
    assert refload.available(), "the reference is needed"
    rng = np.random.default_rng(20261019)
    arrays, writers, readers = {}, [], []
    extras = [("ei", "<i4"), ("ed", "<f8"), ("eh", "<u2"), ("el", "<i8")]
    with tempfile.TemporaryDirectory() as tmp:
        # the writer's tables; every file the reference writes is a reader case too
        small = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("opacity", "<f4"), ("scale_0", "<f4"), ("ed", "<f8"), ("ei", "<i4"), ("c", "u1")]
        tables = [("w_n%d" % n, build(n, small, rng)) for n in COUNTS]
        tables.append(("w_canonical_1000", build(1000, pqn.canonical_fields(False), rng)))
        tables.append(("w_rgb_extras_300", build(300, pqn.canonical_fields(True) + extras, rng)))
        no_nx = [f for f in pqn.canonical_fields(False) if f[0] not in ("nx", "ny", "nz")]
        holes = np.dtype({"names": [f for f, _ in no_nx] + ["eb"], "formats": [t for _, t in no_nx] + ["i1"],
                          "offsets": [1 + 4 * i for i in range(len(no_nx))] + [0], "itemsize": 4 * len(no_nx) + 3})
        tables.append(("w_no_nx_holes_130", build(130, holes, rng)))
        tables.append(("w_wide_200", build(200, pqn.canonical_fields(True) + extras + [("t%d" % i, "<f8") for i in range(6)], rng)))
        for name, table in tables:
            m, path = writer_case(name, table, tmp, arrays)
            writers.append(m)
            if name in ("w_canonical_1000", "w_rgb_extras_300", "w_n129"):
                readers.append(reader_case("r_" + name[2:], path, arrays, file_of=name))
        # pandas-written files with small row groups, at every row count
        for n in COUNTS:
            path = os.path.join(tmp, "p%d.parquet" % n)
            small_frame(n, rng).to_parquet(path, row_group_size=50)
            readers.append(reader_case("r_groups50_n%d" % n, path, arrays))
        # pyarrow's own file, no pandas metadata, row groups of 100
        path = os.path.join(tmp, "direct.parquet")
        pq.write_table(direct_table(1000, rng), path, row_group_size=100)
        readers.append(reader_case("r_direct_1000", path, arrays))
    meta = {"versions": {"pyarrow": pa.__version__, "pandas": pd.__version__, "numpy": np.__version__}, "writers": writers, "readers": readers}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode("utf8"), np.uint8)
    np.savez_compressed(OUT, **arrays)
    print("%s: %d writer cases, %d reader cases, %d bytes" % (OUT, len(writers), len(readers), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
