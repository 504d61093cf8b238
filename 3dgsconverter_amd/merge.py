"""The planning of a merge of several scenes into one table (numpy dtypes only, no device): ``merged_dtype`` decides the common
row layout of the union from the sources' dtypes, ``remap_runs`` turns one source's layout into the byte runs that
csrc/rows_remap.hip (``gsx_rows_remap_dev`` / ``gsx_rows_remap_host``) moves per row.

The merged layout is the reference's standard order (formats/ply_reader.get_standard_order) -- x y z nx ny nz f_dc_0..2
f_rest_0..R-1 opacity scale_0..2 rot_0..3, all '<f4', packed -- with R the largest f_rest count among the sources, and
red green blue as 'u1' behind it when every source has all three as 'u1'.  f_rest is channel-major, m / 3 coefficients per colour
channel ("f_rest channel-major"): a source of m columns goes into R columns as f_rest_(c m/3 + k) ->
f_rest_(c R/3 + k), and the coefficients it does not have are zero.  Fields a source lacks (normals, f_rest) are zero bits in
its rows of the union; fields the union lacks are dropped, and named in the notes.
"""
from __future__ import annotations

import re

import numpy as np

XYZ = ("x", "y", "z")
NORMALS = ("nx", "ny", "nz")
F_DC = ("f_dc_0", "f_dc_1", "f_dc_2")
TAIL = ("opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3")
COLOURS = ("red", "green", "blue")
REQUIRED = XYZ + F_DC + TAIL
REST_COUNTS = (0, 9, 24, 45)
MAX_RUNS = 128              # csrc/rows_remap.hip REMAP_MAX_RUNS
F4, U1 = np.dtype("<f4"), np.dtype("u1")


def rest_count(dtype, label: str = "the table") -> int:
    """the f_rest columns of `dtype`: f_rest_0 .. f_rest_(m-1) with m in (0, 9, 24, 45), or ValueError"""
    ids = sorted(int(m.group(1)) for m in (re.fullmatch(r"f_rest_(\d+)", nm) for nm in np.dtype(dtype).names or ()) if m)
    if ids != list(range(len(ids))) or len(ids) not in REST_COUNTS:
        raise ValueError(f"merge: {len(ids)} f_rest fields of {label} cannot be merged: whole bands of three colour channels are "
                         f"needed (0, 9, 24 or 45 fields named f_rest_0 ...)")
    return len(ids)


def standard_names(n_rest: int) -> tuple:
    return XYZ + NORMALS + F_DC + tuple(f"f_rest_{i}" for i in range(n_rest)) + TAIL


def merged_dtype(dtypes, labels=None):
    """-> (the union's dtype, notes: one line per source that loses fields, naming them).  dtypes: the sources' structured
    dtypes, the main source first; labels: what the messages call them ("source k" without).  ValueError for a source without
    one of x y z f_dc_0..2 opacity scale_0..2 rot_0..3 (the first one missing is named) or with f_rest fields that are no whole
    bands; TypeError, naming the field, for a standard field that is not '<f4' (no silent casts)."""
    dtypes = [np.dtype(d) for d in dtypes]
    if not dtypes:
        raise ValueError("merge: no source")
    labels = [f"source {k}" for k in range(len(dtypes))] if labels is None else [str(s) for s in labels]
    counts = []
    for dt, label in zip(dtypes, labels):
        fields = dt.fields or {}
        for nm in REQUIRED:
            if nm not in fields:
                raise ValueError(f"merge: {label} has no field {nm!r}")
        m = rest_count(dt, label)
        for nm in standard_names(m):
            if nm in fields and fields[nm][0] != F4:
                raise TypeError(f"merge: field {nm!r} of {label} is {fields[nm][0].str}, and the merge copies '<f4' fields only "
                                f"(no silent casts) -- cast the table to float32 first if that is what is wanted")
        counts.append(m)
    R = max(counts)
    names = standard_names(R)
    coloured = all(all(nm in dt.fields and dt.fields[nm][0] == U1 for nm in COLOURS) for dt in dtypes)
    out = np.dtype([(nm, "<f4") for nm in names] + ([(nm, "u1") for nm in COLOURS] if coloured else []))
    notes = []
    for dt, label in zip(dtypes, labels):
        lost = [nm for nm in dt.names if nm not in out.fields]
        if lost:
            notes.append(f"Merge: {label} loses {len(lost)} field{'s' if len(lost) != 1 else ''} the union does not have: {', '.join(lost)}")
    return out, notes


def source_field(name: str, m: int, R: int):
    """the source field that fills the union's field `name` (None: zero), for a source of m f_rest columns in a union of R"""
    hit = re.fullmatch(r"f_rest_(\d+)", name)
    if not hit:
        return name
    c, k = divmod(int(hit.group(1)), R // 3)
    return f"f_rest_{c * (m // 3) + k}" if k < m // 3 else None


def remap_fields(src: np.ndarray, dst: np.ndarray, dst_row0: int = 0) -> np.ndarray:
    """rows [dst_row0, dst_row0 + len(src)) of `dst` from `src`, field by field in numpy: for a host table the row routines do
    not take (rows over 512 bytes, or not contiguous).  The same name map as remap_runs; absent fields become zero -> dst"""
    m, R = rest_count(src.dtype, "the source"), rest_count(dst.dtype, "the destination")
    part = dst[dst_row0:dst_row0 + len(src)]
    for name in dst.dtype.names:
        want = source_field(name, m, R)
        if want is None or want not in src.dtype.fields:
            part[name] = 0
        elif src.dtype.fields[want][0] != dst.dtype.fields[name][0]:
            raise TypeError(f"merge: field {want!r} is {src.dtype.fields[want][0].str} in the source and "
                            f"{dst.dtype.fields[name][0].str} in the union (no silent casts)")
        else:
            part[name] = src[want]
    return dst


def remap_runs(src_dtype, dst_dtype) -> list:
    """-> [(source byte offset or -1 for zero fill, destination byte offset, byte count), ...], sorted by the destination offset,
    every byte of a destination row in exactly one run, neighbours that are contiguous on both sides joined; a source of the
    destination's own dtype is one run of the whole row.  A destination field the source has under another type is a TypeError."""
    src, dst = np.dtype(src_dtype), np.dtype(dst_dtype)
    if src.fields is None or dst.fields is None:
        raise ValueError("merge: structured dtypes are needed")
    if src == dst:
        return [(0, 0, dst.itemsize)]
    m, R = rest_count(src, "the source"), rest_count(dst, "the destination")
    if m > R:
        raise ValueError(f"merge: {m} f_rest fields do not fit a union of {R}")
    from_byte = [-1] * dst.itemsize          # the source byte of every destination byte (padding and absent fields: zero)
    for name in dst.names:
        ftype, at = dst.fields[name][:2]
        want = source_field(name, m, R)
        if want is None or want not in src.fields:
            continue
        if src.fields[want][0] != ftype:
            raise TypeError(f"merge: field {want!r} is {src.fields[want][0].str} in the source and {ftype.str} in the union (no silent casts)")
        for i in range(ftype.itemsize):
            from_byte[at + i] = src.fields[want][1] + i
    runs = []
    for d, s in enumerate(from_byte):
        if runs and (runs[-1][0] + runs[-1][2] == s if s >= 0 and runs[-1][0] >= 0 else s < 0 and runs[-1][0] < 0):
            runs[-1][2] += 1
        else:
            runs.append([s, d, 1])
    if len(runs) > MAX_RUNS:
        raise ValueError(f"merge: {len(runs)} runs per row (at most {MAX_RUNS})")
    return [tuple(r) for r in runs]
