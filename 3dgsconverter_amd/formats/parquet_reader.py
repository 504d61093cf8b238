"""``read_parquet`` -- the reference's ``ParquetFormat.read`` (formats/parquet.py:8-57) with its column loop on the MI355X.

  | step (parquet.py)                                  | here                                                               |
  |----------------------------------------------------|--------------------------------------------------------------------|
  | :10 pd.read_parquet                                | pq.read_schema, then pq.read_table of the columns the rows use;    |
  |                                                    | no DataFrame is built                                              |
  | :14-32 column_mapping, :41-42 the rename           | plan(): column_mapping()                                           |
  | :35-37 nx ny nz = 0.0 where missing                | plan(): a field without a source stays zero                        |
  | :46-49 has_rgb, define_dtype, np.zeros             | plan(): define_dtype(has_rgb, no extras), packed and little-endian |
  | :51-55 `converted_data[name] = df_renamed[name]    | plan(): one descriptor per output field; Arrow's chunks laid end   |
  |        .values`, and to_pandas' null -> NaN        | to end in page-locked staging, one upload, gsx_parquet_rows_dev    |
  |                                                    | (csrc/parquet.hip): one launch, whole rows, one download           |

The rows are the reference's bit for bit ("Parquet reader and writer"): a null reads 0x7fc00000 (0x7fffe000 from an
f16 column, whose nulls to_pandas makes the half 0x7fff), a NaN that is not null keeps its bits, f64 rounds as x86 does, int64
and f16 are cast by value.  pyarrow keeps the pages, snappy, the dictionaries and Thrift.

What the device path does not take is refused with a reason (Plan.refusal) and goes to `fallback`, the reference's own read:
two columns that land on one output name (the reference fails there on a 2-D assignment), a needed column that is none of
i1 ... i8, u1 ... u8, f2, f4, f8 (or red green blue that are not uint8: numpy's cast to uint8 is platform-defined), a needed
integer column with nulls (pandas makes it float64, and red green blue would cast NaN to u1), a needed column that pandas
metadata restores as another type than its own, pandas metadata that stores an index column (it is no column of the frame
then), rows over 512 bytes or over 128 fields.  A path whose schema pq.read_schema cannot read as one file (a partitioned
dataset directory, a damaged footer) goes to `fallback` as well, so that the reference's own result or error stands.

The one known deviation: columns the output does not use are not decoded.  A page that is damaged only in such a column raises
in the reference and not here.
"""
from __future__ import annotations

import json
import time

import numpy as np

from .. import _lib
from ..utils import debug_print
from .ply_reader import COLOURS, define_dtype

MAX_STRIDE = _lib.PARQUET_MAX_STRIDE
MAX_FIELDS = _lib.PARQUET_MAX_FIELDS
# Arrow's name of a type -> numpy's code (the kernel's codes: _lib.PARQUET_TYPE_CODES)
ARROW_TYPES = {"int8": "i1", "uint8": "u1", "int16": "i2", "uint16": "u2", "int32": "i4", "uint32": "u4", "int64": "i8", "uint64": "u8",
               "halffloat": "f2", "float": "f4", "double": "f8"}
NUMPY_NAMES = {"i1": "int8", "u1": "uint8", "i2": "int16", "u2": "uint16", "i4": "int32", "u4": "uint32", "i8": "int64", "u8": "uint64",
               "f2": "float16", "f4": "float32", "f8": "float64"}


class UnsupportedParquetError(ValueError):
    """a file or table the device path refuses, and no fallback to hand it to"""


def column_mapping() -> dict:
    """parquet.py:14-32"""
    m = {"x": "x", "y": "y", "z": "z", "r_sh0": "f_dc_0", "g_sh0": "f_dc_1", "b_sh0": "f_dc_2", "alpha": "opacity",
         "cov_s0": "scale_0", "cov_s1": "scale_1", "cov_s2": "scale_2", "cov_q3": "rot_0", "cov_q0": "rot_1", "cov_q1": "rot_2", "cov_q2": "rot_3"}
    rest = 0
    for channel in "rgb":
        for i in range(1, 16):
            m["%s_sh%d" % (channel, i)] = "f_rest_%d" % rest
            rest += 1
    return m


class Field:
    """one output field: the file column it takes (None: it stays zero), that column's type, where it goes"""
    __slots__ = ("name", "type", "dst_offset", "dst_bytes", "source", "src_type")

    def __init__(self, name, typ, dst_offset):
        self.name, self.type, self.dst_offset, self.dst_bytes = name, typ, dst_offset, np.dtype(typ).itemsize
        self.source = self.src_type = None

    def code(self) -> int:
        return _lib.PLY_T_RAW if self.type != "f4" else _lib.PARQUET_TYPE_CODES[self.src_type or "f4"]


class Plan:
    """what the reader does with a file, from its Arrow schema alone: the output dtype, one Field per output field, the file
    columns to decode; `refusal` says why the device path does not take the file"""

    def __init__(self):
        self.dtype = self.fields = self.refusal = None
        self.has_rgb = False
        self.columns = []              # the file's columns the rows use, in file order
        self.out_stride = 0

    def descriptors(self, index_of):
        """[(column index or None, type code, destination offset, destination bytes)]; index_of: file column name -> index"""
        return [(None if f.source is None else index_of[f.source], f.code(), f.dst_offset, f.dst_bytes) for f in self.fields]


def stored_index_columns(metadata) -> list:
    """the columns pandas metadata names as the frame's index (a RangeIndex kept as metadata alone is none)"""
    raw = (metadata or {}).get(b"pandas")
    if raw is None:
        return []
    try:
        meta = json.loads(raw.decode("utf8"))
    except (ValueError, UnicodeDecodeError):
        return []
    return [c for c in meta.get("index_columns", []) if isinstance(c, str)]


def pandas_numpy_types(metadata) -> dict:
    """file column name -> the numpy_type pandas metadata records for it"""
    raw = (metadata or {}).get(b"pandas")
    if raw is None:
        return {}
    try:
        meta = json.loads(raw.decode("utf8"))
    except (ValueError, UnicodeDecodeError):
        return {}
    return {c.get("field_name", c.get("name")): c.get("numpy_type") for c in meta.get("columns", []) if isinstance(c, dict)}


def plan(names, types, metadata=None) -> Plan:
    """parquet.py:14-55 on a file's schema -> Plan.  Touches no device and no pyarrow.

    names: the file's column names in order; types: Arrow's name of each column's type (str(field.type)); metadata: the
    schema's key-value metadata (bytes -> bytes) or None.  :41-42 a column is renamed where the mapping knows it; :46 has_rgb
    is `'red' in columns` after the rename; :47 define_dtype(has_scal=False, has_rgb); :51-55 an output name takes the column
    that carries it after the rename, else it stays zero (:35-37: missing nx ny nz are zero columns)."""
    names, types = list(names), [str(t) for t in types]
    p = Plan()
    mapping = column_mapping()
    renamed = [mapping.get(n, n) for n in names]
    p.has_rgb = "red" in renamed
    listed = define_dtype(p.has_rgb, None)
    p.dtype = np.dtype([(n, "<" + t if np.dtype(t).itemsize > 1 else t) for n, t in listed])
    p.out_stride = p.dtype.itemsize
    p.fields = []
    index_cols = stored_index_columns(metadata)
    if index_cols:
        p.refusal = "pandas metadata stores the index in column %r" % index_cols[0]
    restored = pandas_numpy_types(metadata)
    for n, t in listed:
        f = Field(n, t, p.dtype.fields[n][1])
        sources = [k for k, r in enumerate(renamed) if r == n]
        if len(sources) > 1 and p.refusal is None:
            p.refusal = "columns %s all land on %r" % (", ".join(repr(names[k]) for k in sources), n)
        if sources:
            k = sources[0]
            f.source, f.src_type = names[k], ARROW_TYPES.get(types[k])
            if p.refusal is None:
                if f.src_type is None:
                    p.refusal = "column %r is %s (the device path reads %s)" % (names[k], types[k], ", ".join(sorted(ARROW_TYPES)))
                elif n in COLOURS and f.src_type != "u1":
                    p.refusal = "column %r is %s (the device path reads uint8 colours: numpy's cast to uint8 is platform-defined)" % (names[k], types[k])
                elif restored.get(names[k]) not in (None, NUMPY_NAMES[f.src_type]):
                    p.refusal = "pandas metadata restores column %r (%s) as %s" % (names[k], types[k], restored[names[k]])
        p.fields.append(f)
    p.columns = [n for n in names if any(f.source == n for f in p.fields)]
    if p.refusal is None:
        if p.out_stride > MAX_STRIDE:
            p.refusal = "rows of %d bytes (the device path takes up to %d)" % (p.out_stride, MAX_STRIDE)
        elif len(p.fields) > MAX_FIELDS:
            p.refusal = "%d output fields (the device path takes up to %d)" % (len(p.fields), MAX_FIELDS)
    return p


def refuse_integer_nulls(p: Plan, null_counts: dict) -> Plan:
    """null_counts: file column -> nulls in it.  A needed integer column with nulls: pandas hands the reference float64 with
    NaN there, and the u1 cast of NaN is undefined"""
    for f in p.fields:
        if p.refusal is None and f.source is not None and f.src_type[0] in "iu" and null_counts.get(f.source, 0):
            p.refusal = "integer column %r has %d nulls (pandas makes it float64)" % (f.source, null_counts[f.source])
    return p


def plan_of_schema(schema) -> Plan:
    """plan() of a pyarrow schema"""
    return plan(schema.names, [str(f.type) for f in schema], schema.metadata)


def arrow_chunks(column, src_type: str) -> list:
    """a pyarrow ChunkedArray of a primitive type -> [(values, validity bytes or None, bit offset, length)], straight from
    Arrow's memory: `values` begins at the chunk's offset, the bitmap is handed on as it lies with the offset as its first bit"""
    dt = np.dtype("<" + src_type if src_type[1] != "1" else src_type)
    out = []
    for a in column.chunks:
        validity, data = a.buffers()[:2]
        n, off = len(a), a.offset
        values = np.frombuffer(data, dt, count=off + n)[off:] if n else np.zeros(0, dt)
        has_nulls = validity is not None and a.null_count > 0
        out.append((values, np.frombuffer(validity, np.uint8) if has_nulls else None, off, n))
    return out


def _clock(stage_ms, name, t0):
    if stage_ms is not None:
        stage_ms[name] = round(stage_ms.get(name, 0.0) + (time.perf_counter() - t0) * 1e3, 3)


def read_parquet(path: str, stage_ms: "dict | None" = None, fallback=None, device: int = 0, profile: "dict | None" = None, keep: "dict | None" = None) -> np.ndarray:
    """parquet.py:8-57 -> the reference's structured array (define_dtype(has_scal=False, has_rgb) at sh_degree=3, packed,
    little-endian).

    fallback: a function path -> rows for the files the device path does not take (Plan.refusal); without one such files raise
    UnsupportedParquetError.  stage_ms: a dict that receives the stage clocks plan, decode (pq.read_table), gather (Arrow's
    chunks into page-locked staging), upload, kernel, download (tools/probe_parquet.py).  n = 0 returns the empty array of the
    plan's dtype without a launch.  profile: a dict that receives the returned table's profile (_lib.TableProfile.as_dict) from
    one more pass over the transposed rows before their download (stage clock "profile").  keep: a dict that receives the decoded rows in HBM as keep["rows"] (_lib.ResidentRows; the caller
    closes it) when the returned table's rows are resident; it stays empty otherwise."""
    return _lib.with_keep(keep, lambda: _lib.with_profile(profile, lambda: _read(path, stage_ms, fallback, device, profile, keep)))


def _read(path, stage_ms, fallback, device, profile, keep=None):
    import pyarrow.parquet as pq
    debug_print(f"[DEBUG] Reading Parquet file from {path}")

    def refuse(why):
        if fallback is None:
            raise UnsupportedParquetError("%s: %s -- this file needs the reference's reader (pandas)" % (path, why))
        debug_print(f"[DEBUG] Parquet: {why}; the reference's reader takes it")
        return fallback(path)

    t0 = time.perf_counter()
    try:
        schema = pq.read_schema(path)
    except Exception as e:              # a partitioned dataset directory, a file object, a damaged footer: what pd.read_parquet
        if fallback is None:            # makes of it is the reference's to say
            raise
        debug_print(f"[DEBUG] Parquet: the schema cannot be read from one file ({type(e).__name__}: {e}); the reference's reader takes it")
        return fallback(path)
    p = plan_of_schema(schema)
    _clock(stage_ms, "plan", t0)
    if p.refusal is not None:
        return refuse(p.refusal)
    t0 = time.perf_counter()
    table = pq.read_table(path, columns=p.columns)
    _clock(stage_ms, "decode", t0)
    n = table.num_rows
    refuse_integer_nulls(p, {c: table.column(c).null_count for c in p.columns})
    if p.refusal is not None:
        return refuse(p.refusal)
    if n == 0:                                                                      # :49 np.zeros(0, dtype)
        return np.zeros(0, p.dtype)
    index_of = {c: k for k, c in enumerate(p.columns)}
    src_type = {f.source: f.src_type for f in p.fields if f.source is not None}
    columns = [arrow_chunks(table.column(c), src_type[c]) for c in p.columns]
    rows = _lib.parquet_rows_table(columns, n, p.descriptors(index_of), p.dtype, stage_ms=stage_ms, device=device, **_lib.profile_kw(profile), **_lib.keep_kw(keep))
    debug_print(f"[DEBUG] Loaded {n} rows from Parquet")
    return rows


def bind_read(original):
    """-> a replacement for ``ParquetFormat.read`` that transposes and casts the columns on the device; files the device path
    does not take go to `original` (the reference's read)"""
    def read(self, path, **kwargs):
        return read_parquet(path, fallback=lambda p: original(self, p, **kwargs))
    read.__wrapped__ = original
    return read
