"""A numpy restatement of the reference's ParquetFormat (gsconverter/formats/parquet.py) in both directions, and the loader of
tests/golden/parquet_ref.npz (tests/devtools/make_golden_parquet.py).

  read    rename (:14-32, :41-42), has_rgb and the dtype (:46-48), `converted_data[name] = df_renamed[name].values` (:51-55) on
          the chunk lists pq.read_table delivers: a null is np.nan in the column's own float type before the cast, as
          to_pandas makes it
  write   rename (:63-77, :97-98), the strict order and the extras (:80-108), then what pa.Table.from_pandas builds of the
          frame: one contiguous column per field, for f4 / f8 the validity bitmap !isnan(v) and the null count, a bitmap only
          where there are nulls, the `pandas` schema metadata; and to_parquet's pq.write_table(table, path, compression="snappy")

Nothing here imports the package under test: the host tests tie this file to the reference's recorded results, the GPU tests
use it where no fixture applies."""
import json

import numpy as np

N_REST = 45
COLOURS = ["red", "green", "blue"]
STD = (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + ["f_rest_%d" % i for i in range(N_REST)]
       + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"])
# the kernel's type codes (include/gsx_hip.h GSX_PLY_T_*, GSX_PARQUET_T_*)
CODES = {"i1": 0, "u1": 1, "i2": 2, "u2": 3, "i4": 4, "u4": 5, "f4": 6, "f8": 7, "i8": 9, "u8": 10, "f2": 11}
RAW = 8
CODE_TYPES = {v: k for k, v in CODES.items()}
ARROW_TYPES = {"int8": "i1", "uint8": "u1", "int16": "i2", "uint16": "u2", "int32": "i4", "uint32": "u4", "int64": "i8", "uint64": "u8",
               "halffloat": "f2", "float": "f4", "double": "f8"}
PA_NAMES = {"f4": "float32", "f8": "float64", "i1": "int8", "i2": "int16", "i4": "int32", "i8": "int64", "u1": "uint8", "u2": "uint16",
            "u4": "uint32", "u8": "uint64"}


def canonical_fields(with_rgb=False):
    return [(f, "<f4") for f in STD] + ([(c, "u1") for c in COLOURS] if with_rgb else [])


# ---------------------------------------------------------------------------------------------------------------- the reader

def column_mapping():
    m = {"x": "x", "y": "y", "z": "z", "r_sh0": "f_dc_0", "g_sh0": "f_dc_1", "b_sh0": "f_dc_2", "alpha": "opacity",
         "cov_s0": "scale_0", "cov_s1": "scale_1", "cov_s2": "scale_2", "cov_q3": "rot_0", "cov_q0": "rot_1", "cov_q1": "rot_2", "cov_q2": "rot_3"}
    k = 0
    for ch in "rgb":
        for i in range(1, 16):
            m["%s_sh%d" % (ch, i)] = "f_rest_%d" % k
            k += 1
    return m


def chunk_bits(validity, bit_offset, length):
    if validity is None:
        return np.ones(length, bool)
    bits = np.unpackbits(np.frombuffer(validity, np.uint8), bitorder="little")
    return bits[bit_offset:bit_offset + length].astype(bool)


def column_values(chunks):
    """[(values, validity or None, bit offset, length)] -> (values[n], valid[n])"""
    vals = np.concatenate([np.asarray(v)[:ln] for v, _, _, ln in chunks])
    valid = np.concatenate([chunk_bits(b, bo, ln) for _, b, bo, ln in chunks])
    return vals, valid


def cast_f4(vals, valid):
    """to_pandas: a null is NaN in the column's own float type; then numpy's cast to float32"""
    with np.errstate(all="ignore"):
        if vals.dtype.kind == "f" and not valid.all():
            vals = vals.copy()
            vals[~valid] = np.nan if vals.dtype.itemsize > 2 else np.array(0x7fff, np.uint16).view(np.float16)   # to_pandas' half NaN
        elif not valid.all():
            raise ValueError("an integer column with nulls")
        if vals.dtype == np.float32:
            return vals
        return vals.astype(np.float32)


def rows_from_descriptors(columns, n, fields, dtype):
    """what gsx_parquet_rows_dev computes: fields = [(column index or None, type code, destination offset, destination bytes)]"""
    dtype = np.dtype(dtype)
    out = np.zeros((n, dtype.itemsize), np.uint8)
    for ci, code, dof, nb in fields:
        if ci is None or n == 0:
            continue
        vals, valid = column_values(columns[ci])
        if code != RAW:
            assert vals.dtype.str[1:] == CODE_TYPES[code], (vals.dtype, code)
            vals = np.ascontiguousarray(cast_f4(vals, valid))
        assert vals.dtype.itemsize == nb
        out[:, dof:dof + nb] = np.ascontiguousarray(vals).view(np.uint8).reshape(n, nb)
    return out.reshape(-1).view(dtype) if n else np.zeros(0, dtype)


def read_plan(names, types):
    """-> (dtype, [(output field, file column or None)]); types: numpy codes ("f4", ...) or None for what is no such type"""
    m = column_mapping()
    renamed = [m.get(c, c) for c in names]
    has_rgb = "red" in renamed
    dtype = np.dtype(canonical_fields(has_rgb))
    return dtype, [(f, names[renamed.index(f)] if f in renamed else None) for f in dtype.names]


def read_rows(names, types, columns, n):
    """ParquetFormat.read on a file's columns: names, types (numpy codes) and chunk lists in file order"""
    dtype, listed = read_plan(names, types)
    fields = []
    for f, src in listed:
        t = dtype[f]
        if src is None:
            fields.append((None, RAW if t.kind == "u" else CODES["f4"], dtype.fields[f][1], t.itemsize))
        else:
            k = names.index(src)
            fields.append((k, RAW if t.kind == "u" else CODES[types[k]], dtype.fields[f][1], t.itemsize))
    return rows_from_descriptors(columns, n, fields, dtype)


# ---------------------------------------------------------------------------------------------------------------- the writer

def reverse_mapping():
    m = {"x": "x", "y": "y", "z": "z", "rot_0": "cov_q3", "rot_1": "cov_q0", "rot_2": "cov_q1", "rot_3": "cov_q2",
         "scale_0": "cov_s0", "scale_1": "cov_s1", "scale_2": "cov_s2", "opacity": "alpha",
         "f_dc_0": "r_sh0", "f_dc_1": "g_sh0", "f_dc_2": "b_sh0", "nx": "nx", "ny": "ny", "nz": "nz"}
    for i in range(15):
        m["f_rest_%d" % i], m["f_rest_%d" % (15 + i)], m["f_rest_%d" % (30 + i)] = "r_sh%d" % (i + 1), "g_sh%d" % (i + 1), "b_sh%d" % (i + 1)
    return m


def write_plan(dtype):
    """-> [(column name, table field)] in file order"""
    names = list(np.dtype(dtype).names)
    m = reverse_mapping()
    renamed = [m.get(f, f) for f in names]
    order = ["x", "y", "z"] + (["nx", "ny", "nz"] if "nx" in names else []) + ["cov_q0", "cov_q1", "cov_q2", "cov_q3", "cov_s0", "cov_s1", "cov_s2", "alpha"]
    for ch in "rgb":
        order += ["%s_sh%d" % (ch, i) for i in range(16)]
    targets = set(m.values())
    final = [c for c in order if c in renamed] + [c for c in renamed if c not in targets]
    return [(c, names[renamed.index(c)]) for c in final]


def split_field(data, so, nb, kind):
    """one field of a table -> (column bytes uint8[n * nb], bitmap uint8[(n + 7) // 8] or None, null count)"""
    n = len(data)
    raw = np.ascontiguousarray(data).view(np.uint8).reshape(n, data.dtype.itemsize)
    col = np.ascontiguousarray(raw[:, so:so + nb]).reshape(-1)
    if not kind:
        return col, None, 0
    nan = np.isnan(col.view("<f4" if kind == 1 else "<f8"))
    return col, np.packbits(~nan, bitorder="little"), int(nan.sum())


def split_columns(data, fields):
    """what gsx_parquet_columns_dev computes: fields = [(source offset, bytes, kind)] -> (columns, bitmaps, null counts)"""
    got = [split_field(data, so, nb, kind) for so, nb, kind in fields]
    return [g[0] for g in got], [g[1] for g in got], [g[2] for g in got]


def kind_of(t):
    return {"f4": 1, "f8": 2}.get(np.dtype(t).str[1:], 0)


def write_columns(data):
    """-> [(column name, numpy code, column bytes, bitmap or None, null count)] in file order"""
    out = []
    for c, f in write_plan(data.dtype):
        t = data.dtype[f]
        col, bitmap, nulls = split_field(data, data.dtype.fields[f][1], t.itemsize, kind_of(t))
        out.append((c, t.str[1:], col, bitmap, nulls))
    return out


def write_file(data, path):
    """the restatement's file: the columns above as a pa.Table with from_pandas' schema, through to_parquet's write_table call"""
    import pandas as pd
    import pyarrow as pa
    import pyarrow.parquet as pq
    n = len(data)
    cols = write_columns(data)
    schema = pa.Schema.from_pandas(pd.DataFrame({c: np.zeros(0, t) for c, t, _, _, _ in cols}, columns=[c for c, *_ in cols]))
    doc = json.loads(schema.metadata[b"pandas"].decode("utf8"))
    doc["index_columns"][0]["stop"] = n
    schema = schema.with_metadata({**schema.metadata, b"pandas": json.dumps(doc).encode("utf8")})
    arrays = [pa.Array.from_buffers(getattr(pa, PA_NAMES[t])(), n, [pa.py_buffer(bitmap.tobytes()) if nulls else None, pa.py_buffer(col.tobytes())], nulls)
              for _, t, col, bitmap, nulls in cols]
    pq.write_table(pa.Table.from_arrays(arrays, schema=schema), path, compression="snappy")


# --------------------------------------------------------------------------------------------------------------- the fixture

def dtype_to_json(dt):
    dt = np.dtype(dt)
    return {"names": list(dt.names), "formats": [dt[f].str for f in dt.names], "offsets": [int(dt.fields[f][1]) for f in dt.names], "itemsize": int(dt.itemsize)}


def dtype_from_json(d):
    return np.dtype({"names": d["names"], "formats": d["formats"], "offsets": d["offsets"], "itemsize": d["itemsize"]})


class WriterCase:
    """name, table, file (bytes), versions {pyarrow, pandas}, columns: [{name, type, nulls, values (invalid slots zero), valid
    (bool[n])}] as pq.read_table gave the reference's file back"""


class ReaderCase:
    """name, file (bytes), names / types (numpy code or None) of the file's columns, columns: chunk lists of the decodable
    columns by file column index ({index: [(values, validity, bit offset, length)]}), n, rows (the reference's read)"""


def load_cases(path):
    z = np.load(path)
    meta = json.loads(bytes(z["meta"]).decode("utf8"))
    writers, readers = {}, {}
    for m in meta["writers"]:
        c = WriterCase()
        c.name, c.versions = m["name"], meta["versions"]
        c.table = np.frombuffer(z[c.name + "/table"].tobytes(), dtype_from_json(m["dtype"])).copy()
        c.file = z[c.name + "/file"].tobytes()
        c.columns = []
        for k, col in enumerate(m["columns"]):
            n = len(c.table)
            valid = np.unpackbits(z["%s/rb%d/valid" % (c.name, k)], bitorder="little")[:n].astype(bool) if col["nulls"] else np.ones(n, bool)
            c.columns.append({"name": col["name"], "type": col["type"], "nulls": col["nulls"], "valid": valid, "values": z["%s/rb%d/values" % (c.name, k)]})
        writers[c.name] = c
    for m in meta["readers"]:
        c = ReaderCase()
        c.name, c.n, c.names, c.types, c.has_pandas = m["name"], m["n"], m["names"], m["types"], m["has_pandas"]
        c.file = z[(m["file_of"] or c.name) + "/file"].tobytes()
        c.rows = np.frombuffer(z[c.name + "/rows"].tobytes(), dtype_from_json(m["dtype"])).copy()
        c.columns = {}
        for k, chunks in m["chunks"].items():
            k = int(k)
            vals = z["%s/c%d/values" % (c.name, k)]
            vbytes = z["%s/c%d/validity" % (c.name, k)] if any(ch[2] >= 0 for ch in chunks) else None
            pos = vpos = 0
            lst = []
            for length, off, vlen in chunks:
                validity = None
                if vlen >= 0:
                    validity = vbytes[vpos:vpos + vlen].copy()
                    vpos += vlen
                lst.append((vals[pos:pos + length].copy(), validity, off, length))
                pos += length
            c.columns[k] = lst
        readers[c.name] = c
    return writers, readers, meta["versions"]


# ------------------------------------------------------------------------------ a stand-in for the reference, for install()

STANDIN = {
    "gsconverter/__init__.py": "",
    "gsconverter/processing/__init__.py": "from . import gpu_ops\nfrom .data_processor import DataProcessor\n",
    "gsconverter/processing/gpu_ops.py": "HAS_TAICHI = False\n",
    "gsconverter/processing/data_processor.py": "class DataProcessor:\n    def __init__(self, data):\n        self.data = data\n",
    "gsconverter/converter.py": "from .processing import DataProcessor\n",
    "gsconverter/formats/__init__.py": "",
    "gsconverter/formats/parquet.py": ("class ParquetFormat:\n    def read(self, path, **kw):\n        return ('own read', path, sorted(kw))\n"
                                       "    def write(self, data, path, **kw):\n        open(path, 'w').write('own write ' + ' '.join(sorted(kw)))\n"),
}


class standin_reference:
    """``with standin_reference(tmp_path) as ParquetFormat:`` -- a package named gsconverter with the modules install() binds and
    a ParquetFormat whose own read and write say that they ran; the real one, where it is loaded, is put back afterwards"""

    def __init__(self, tmp_path):
        self.root = str(tmp_path / "standin")

    def __enter__(self):
        import importlib
        import os
        import sys
        for rel, src in STANDIN.items():
            os.makedirs(os.path.dirname(os.path.join(self.root, rel)), exist_ok=True)
            with open(os.path.join(self.root, rel), "w") as f:
                f.write(src)
        self.saved = {m: sys.modules.pop(m) for m in list(sys.modules) if m == "gsconverter" or m.startswith("gsconverter.")}
        sys.path.insert(0, self.root)
        importlib.invalidate_caches()
        return importlib.import_module("gsconverter.formats.parquet").ParquetFormat

    def __exit__(self, *exc):
        import sys
        sys.path.remove(self.root)
        for m in [m for m in sys.modules if m == "gsconverter" or m.startswith("gsconverter.")]:
            del sys.modules[m]
        sys.modules.update(self.saved)


def check_install(gsx, ParquetFormat, writers, readers, tmp_path, refused_table, refused_file):
    """install() leaves ParquetFormat alone unless asked; install(parquet_reader=True, parquet_writer=True) binds both ends: a
    write through the bound method is the restatement's file whatever kwargs the converter passes along, a read of it gives
    the reference's rows, what the device path refuses reaches the class's own methods with the kwargs; uninstall() restores"""
    import os
    own_read, own_write = ParquetFormat.read, ParquetFormat.write
    gsx.install()
    try:
        assert ParquetFormat.read is own_read and ParquetFormat.write is own_write           # off unless asked for
    finally:
        gsx.uninstall()
    gsx.install(parquet_reader=True)
    try:
        assert ParquetFormat.read.__wrapped__ is own_read and ParquetFormat.write is own_write
    finally:
        gsx.uninstall()
    assert ParquetFormat.read is own_read
    gsx.install(parquet_reader=True, parquet_writer=True)
    try:
        assert ParquetFormat.read.__wrapped__ is own_read and ParquetFormat.write.__wrapped__ is own_write
        c = writers["w_rgb_extras_300"]
        got, want = str(tmp_path / "bound.parquet"), str(tmp_path / "want.parquet")
        # the converter's kwargs never reach write_parquet's own keywords: the reference ignores every one of them
        assert ParquetFormat().write(c.table, got, device=7, stage_ms="no dict", fallback=None, compression_level=3) is None
        write_file(c.table, want)
        with open(got, "rb") as fa, open(want, "rb") as fb:
            assert fa.read() == fb.read()
        rows = ParquetFormat().read(got, anything=1)
        assert rows.dtype == readers["r_rgb_extras_300"].rows.dtype and rows.tobytes() == readers["r_rgb_extras_300"].rows.tobytes()
        path = str(tmp_path / "refused.parquet")
        ParquetFormat().write(refused_table, path, crop_sh=False)
        with open(path) as f:
            assert f.read() == "own write crop_sh"
        assert ParquetFormat().read(refused_file, x=1) == ("own read", refused_file, ["x"])
        assert ParquetFormat().read(os.path.join(str(tmp_path), "no_such_dir")) == ("own read", os.path.join(str(tmp_path), "no_such_dir"), [])
    finally:
        gsx.uninstall()
    assert ParquetFormat.read is own_read and ParquetFormat.write is own_write
