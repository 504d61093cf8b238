"""The binary little-endian PLY container as plyfile lays it out for ``PlyData(elements, byte_order='<')``: the header lines
`ply` / `format binary_little_endian 1.0` / `element <name> <count>` / `property <type> <name>` / `end_header`, then every
element's rows.  Shared by the writers that end in such a file when plyfile is not there (formats/compressed_ply_writer.py) or
never use it (formats/ply_writer.py)."""
from __future__ import annotations

import numpy as np

# numpy type (without its byte order) -> the property type plyfile writes
PLY_TYPE_NAMES = {"i1": "char", "u1": "uchar", "i2": "short", "u2": "ushort", "i4": "int", "u4": "uint", "f4": "float", "f8": "double"}


def properties(dtype: np.dtype) -> list:
    """-> [(property type, name)] of a structured dtype of PLY scalars (KeyError for a field of another type)"""
    return [(PLY_TYPE_NAMES[dtype[name].str[1:]], name) for name in dtype.names]


def header(elements) -> bytes:
    """elements: [(name, count, [(property type, property name)])] -> the header's bytes"""
    head = ["ply", "format binary_little_endian 1.0"]
    for name, count, props in elements:
        head.append(f"element {name} {count}")
        for typ, prop in props:
            head.append(f"property {typ} {prop}")
    head.append("end_header")
    return ("\n".join(head) + "\n").encode("ascii")


def little_endian(arr: np.ndarray) -> np.ndarray:
    """the array's rows as they go into the file: C-contiguous, packed, every field little-endian (a big-endian field is
    byte-swapped by value, as plyfile does)"""
    packed = np.dtype([(name, arr.dtype[name].newbyteorder("<")) for name in arr.dtype.names])
    if arr.dtype == packed:
        return np.ascontiguousarray(arr)
    out = np.empty(len(arr), packed)
    for name in packed.names:
        out[name] = arr[name]
    return out


def write_ply(path, elements):
    """binary little-endian PLY with the given (name, structured array) elements -- the layout plyfile produces for
    ``PlyData(elements, text=False, byte_order='<')`` (compressed_ply.py:385-390)"""
    with open(path, "wb") as f:
        f.write(header([(name, len(arr), properties(arr.dtype)) for name, arr in elements]))
        for _, arr in elements:
            f.write(little_endian(arr).tobytes())
