"""``write_parquet`` -- the reference's ``ParquetFormat.write`` (formats/parquet.py:59-112) with the frame's columns built on the
MI355X, and no DataFrame.

  | step (parquet.py)                                  | here                                                               |
  |----------------------------------------------------|--------------------------------------------------------------------|
  | :63-77 reverse_mapping, :97-98 the rename          | plan_write(): reverse_mapping()                                    |
  | :80-91 column_order, :101-108 existing_order and   | plan_write(): the strict order (nx ny nz only when `nx` is a       |
  |        the extras                                  | field), then the extras in table order                             |
  | :94 pd.DataFrame(data): a strided copy per field   | the table uploaded once, gsx_parquet_columns_dev                   |
  | :111 to_parquet -> pa.Table.from_pandas: a NaN     | (csrc/parquet.hip): one launch writes every column, and for f4 /   |
  |        scan per float column (bitmap, null count)  | f8 its validity bitmap and null count; one download into           |
  |                                                    | page-locked staging, wrapped by pyarrow without a copy             |
  | :111 -> pq.write_table(table, compression=snappy)  | the same call, on a table with the schema and the `pandas`         |
  |                                                    | metadata from_pandas would have made                               |
  | :112 the status line                               | the same line                                                      |

The file is the reference's byte for byte under the same pyarrow and pandas ("Parquet reader and writer"): every float
NaN is a null (the validity bit is !isnan(v), the statistics count the nulls), a column without nulls carries no bitmap.  What
the device path does not take is refused with a reason (WritePlan.refusal) and goes to `fallback`, the reference's own write,
so its own error is raised: a field that is not one of f4, f8, i1 ... i8, u1 ... u8 little-endian (bool, f2, strings and
sub-arrays), two fields that land on one column name (pandas raises on duplicates), rows over 512 bytes or more than 128 fields.
"""
from __future__ import annotations

import json
import time

import numpy as np

from .. import _lib
from ..utils import debug_print, status_print
from .parquet_reader import UnsupportedParquetError

MAX_STRIDE = _lib.PARQUET_MAX_STRIDE
MAX_FIELDS = _lib.PARQUET_MAX_FIELDS
FIELD_TYPES = ("f4", "f8", "i1", "i2", "i4", "i8", "u1", "u2", "u4", "u8")
ARROW_NAMES = {"f4": "float32", "f8": "float64", "i1": "int8", "i2": "int16", "i4": "int32", "i8": "int64",
               "u1": "uint8", "u2": "uint16", "u4": "uint32", "u8": "uint64"}      # pa.<name>()


def reverse_mapping() -> dict:
    """parquet.py:63-77"""
    m = {"x": "x", "y": "y", "z": "z", "rot_0": "cov_q3", "rot_1": "cov_q0", "rot_2": "cov_q1", "rot_3": "cov_q2",
         "scale_0": "cov_s0", "scale_1": "cov_s1", "scale_2": "cov_s2", "opacity": "alpha",
         "f_dc_0": "r_sh0", "f_dc_1": "g_sh0", "f_dc_2": "b_sh0", "nx": "nx", "ny": "ny", "nz": "nz"}
    for i in range(15):
        m["f_rest_%d" % i] = "r_sh%d" % (i + 1)
        m["f_rest_%d" % (15 + i)] = "g_sh%d" % (i + 1)
        m["f_rest_%d" % (30 + i)] = "b_sh%d" % (i + 1)
    return m


def column_order(with_normals: bool) -> list:
    """parquet.py:80-91"""
    order = ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else [])
    order += ["cov_q0", "cov_q1", "cov_q2", "cov_q3", "cov_s0", "cov_s1", "cov_s2", "alpha"]
    for channel in "rgb":
        order += ["%s_sh%d" % (channel, i) for i in range(16)]
    return order


class WriteColumn:
    """one column of the file: its name there, the table field it is, that field's type, offset and size"""
    __slots__ = ("name", "source", "type", "src_offset", "nbytes")

    def __init__(self, name, source, typ, src_offset, nbytes):
        self.name, self.source, self.type, self.src_offset, self.nbytes = name, source, typ, src_offset, nbytes

    @property
    def kind(self) -> int:
        """0: a bit copy alone; 1: float32, 2: float64 -- a validity bitmap and a null count with it"""
        return {"f4": 1, "f8": 2}.get(self.type, 0)

    def entry(self):
        return self.src_offset, self.nbytes, self.kind


class WritePlan:
    """what the writer does with a table, from its dtype alone: the file's columns in order; `refusal` says why the device path
    does not take the table"""

    def __init__(self):
        self.columns = self.refusal = None
        self.in_stride = 0

    def entries(self):
        return [c.entry() for c in self.columns]


def plan_write(dtype: np.dtype) -> WritePlan:
    """parquet.py:63-108 on a table's dtype -> WritePlan.  Touches no device and no pyarrow.

    :97-98 a field is renamed where the reverse mapping knows it; :80-91 the strict order, nx ny nz in it only when `nx` is a
    field; :101 the columns of that order that exist; :104-105 the extras are the columns whose name is no target of the
    mapping, in table order (so ny or nz without nx are dropped: targets, and not in the order)."""
    dtype = np.dtype(dtype)
    if dtype.names is None:
        raise ValueError("plan_write: a structured dtype is needed")
    p = WritePlan()
    p.in_stride = dtype.itemsize
    names = dtype.names
    mapping = reverse_mapping()
    renamed = [mapping.get(n, n) for n in names]
    source_of = {}
    for n, r in zip(names, renamed):
        if r in source_of and p.refusal is None:
            p.refusal = "fields %r and %r both land on column %r" % (source_of[r], n, r)
        source_of.setdefault(r, n)
    targets = set(mapping.values())
    final = [c for c in column_order("nx" in names) if c in source_of] + [r for r in renamed if r not in targets]
    p.columns = []
    for c in final:
        src = source_of[c]
        ft = dtype[src]
        code = ft.str[1:]
        if p.refusal is None:
            if ft.shape or ft.names or ft.kind not in "iuf" or code not in FIELD_TYPES:
                p.refusal = "field %r is %s (the device path writes %s)" % (src, ft, ", ".join(FIELD_TYPES))
            elif ft.str[0] == ">":
                p.refusal = "field %r is big-endian (%s)" % (src, ft.str)
        p.columns.append(WriteColumn(c, src, code, dtype.fields[src][1], ft.itemsize))
    if p.refusal is None:
        if p.in_stride > MAX_STRIDE:
            p.refusal = "rows of %d bytes (the device path takes up to %d)" % (p.in_stride, MAX_STRIDE)
        elif len(p.columns) > MAX_FIELDS:
            p.refusal = "%d columns (the device path takes up to %d)" % (len(p.columns), MAX_FIELDS)
        elif not p.columns:
            p.refusal = "no column to write"
    return p


def pandas_schema(p: WritePlan, n: int):
    """the Arrow schema `pa.Table.from_pandas(df)` gives the reference's frame: pa.Schema.from_pandas of an EMPTY frame with
    the same columns, the RangeIndex's stop in its `pandas` metadata set to n"""
    import pandas as pd
    import pyarrow as pa
    empty = pd.DataFrame({c.name: np.zeros(0, c.type) for c in p.columns}, columns=[c.name for c in p.columns])
    schema = pa.Schema.from_pandas(empty)
    meta = dict(schema.metadata)
    doc = json.loads(meta[b"pandas"].decode("utf8"))
    for ic in doc["index_columns"]:
        if isinstance(ic, dict) and ic.get("kind") == "range":
            ic["stop"] = int(n)
    meta[b"pandas"] = json.dumps(doc).encode("utf8")
    return schema.with_metadata(meta)


def arrow_table(p: WritePlan, n: int, columns, bitmaps, null_counts):
    """per column the value bytes, the validity bitmap (or None) and the null count -> the pa.Table from_pandas would have
    built: buffers wrapped where they lie (pa.py_buffer: no copy), a bitmap only on a column that has nulls"""
    import pyarrow as pa
    schema = pandas_schema(p, n)
    arrays = []
    for c, values, bitmap, nulls in zip(p.columns, columns, bitmaps, null_counts):
        validity = pa.py_buffer(bitmap) if nulls else None
        arrays.append(pa.Array.from_buffers(getattr(pa, ARROW_NAMES[c.type])(), n, [validity, pa.py_buffer(values)], int(nulls)))
    return pa.Table.from_arrays(arrays, schema=schema)


def _clock(stage_ms, name, t0):
    if stage_ms is not None:
        stage_ms[name] = round(stage_ms.get(name, 0.0) + (time.perf_counter() - t0) * 1e3, 3)


def write_table(p: WritePlan, n: int, columns, bitmaps, null_counts, path, stage_ms=None):
    """arrow_table(), then the reference's own pq.write_table call (what df.to_parquet(path) ends in)"""
    import pyarrow.parquet as pq
    t0 = time.perf_counter()
    table = arrow_table(p, n, columns, bitmaps, null_counts)
    _clock(stage_ms, "table", t0)
    t0 = time.perf_counter()
    pq.write_table(table, path, compression="snappy")
    _clock(stage_ms, "encode_write", t0)


def _reference_write():
    try:
        from gsconverter.formats.parquet import ParquetFormat as cls  # type: ignore
    except ImportError:
        return None
    write = getattr(cls.write, "__wrapped__", cls.write)
    return lambda data, path, **kw: write(cls(), data, path, **kw)


def write_parquet(data: np.ndarray, path: str, stage_ms: "dict | None" = None, device: int = 0, fallback=None, **kwargs):
    """parquet.py:59-112: `data` (a 1-D structured table) -> a snappy Parquet file at `path`, the reference's file byte for
    byte under the same pyarrow and pandas.  -> the WritePlan that was carried out.

    fallback: a function () -> None that writes the file the reference's way, for the tables the device path does not take
    (WritePlan.refusal); without one the reference's own write is used when the reference is there, else such tables raise
    UnsupportedParquetError.  stage_ms: a dict that receives the stage clocks plan, upload, kernel, download, table (the Arrow
    table around the staging) and encode_write (pq.write_table: pages, snappy and the file).  n = 0 writes the empty table
    without a launch.  kwargs are ignored, as the reference ignores them."""
    debug_print(f"[DEBUG] Writing Parquet file to {path}")
    if not isinstance(data, np.ndarray) or data.dtype.names is None or data.ndim != 1:
        raise ValueError("write_parquet: a 1-D structured table is needed")
    if fallback is None:
        ref = _reference_write()
        fallback = None if ref is None else (lambda: ref(data, path, **kwargs))
    t0 = time.perf_counter()
    p = plan_write(data.dtype)
    _clock(stage_ms, "plan", t0)
    if p.refusal is not None:
        if fallback is None:
            raise UnsupportedParquetError("%s: %s -- this table needs the reference's writer (pandas)" % (path, p.refusal))
        debug_print(f"[DEBUG] Parquet: {p.refusal}; the reference's writer takes it")
        fallback()
        return p
    n = len(data)
    if n == 0:
        write_table(p, 0, [np.zeros(0, np.uint8)] * len(p.columns), [None] * len(p.columns), [0] * len(p.columns), path, stage_ms)
    else:
        _lib.parquet_columns_table(np.ascontiguousarray(data), p.entries(), stage_ms=stage_ms, device=device,
                                   consume=lambda cols, bitmaps, nulls: write_table(p, n, cols, bitmaps, nulls, path, stage_ms))
    status_print(f"Parquet write completed. {n} rows.")                             # :112
    return p


def bind_write(original):
    """-> a replacement for ``ParquetFormat.write`` that builds the columns on the device; tables the device path does not take
    go to `original` (the reference's write)"""
    def write(self, data, path, **kwargs):
        # the reference ignores every kwarg: they reach only its own write, never write_parquet's stage_ms / device / fallback
        write_parquet(data, path, fallback=lambda: original(self, data, path, **kwargs))
    write.__wrapped__ = original
    return write
