"""The definition of a merge, numpy only: the union's dtype from the sources' dtypes and the union's rows as per-field column
assignments through the name map.  tests/test_merge_host.py and tests/test_merge_gpu.py hold the package against it on
``tobytes()``: every value is a bit copy."""
import re

import numpy as np

BEFORE = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
AFTER = ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
COLOURS = ["red", "green", "blue"]


def n_rest(dtype) -> int:
    return sum(1 for nm in np.dtype(dtype).names if re.fullmatch(r"f_rest_\d+", nm))


def merged_dtype(dtypes) -> np.dtype:
    """the standard order with the largest f_rest count, '<f4'; red green blue as 'u1' when every source has the three as 'u1'"""
    dtypes = [np.dtype(d) for d in dtypes]
    R = max(n_rest(d) for d in dtypes)
    fields = [(nm, "<f4") for nm in BEFORE + ["f_rest_%d" % i for i in range(R)] + AFTER]
    if all(all(nm in d.names and d[nm] == np.dtype("u1") for nm in COLOURS) for d in dtypes):
        fields += [(nm, "u1") for nm in COLOURS]
    return np.dtype(fields)


def name_map(src_dtype, dst_dtype) -> dict:
    """{destination field: source field or None (zero)}: equal names, and f_rest channel-major -- channel c, coefficient k of m / 3
    is f_rest_(c m/3 + k) in the source and f_rest_(c R/3 + k) in the destination"""
    src, dst = np.dtype(src_dtype), np.dtype(dst_dtype)
    m, R = n_rest(src), n_rest(dst)
    out = {}
    for nm in dst.names:
        hit = re.fullmatch(r"f_rest_(\d+)", nm)
        if hit:
            c, k = divmod(int(hit.group(1)), R // 3)
            out[nm] = "f_rest_%d" % (c * (m // 3) + k) if k < m // 3 else None
        else:
            out[nm] = nm if nm in src.names else None
    return out


def merge_into(out: np.ndarray, row0: int, src: np.ndarray) -> np.ndarray:
    """rows [row0, row0 + len(src)) of `out` from `src`, column by column; a field without a source is zero"""
    part = out[row0:row0 + len(src)]
    for nm, want in name_map(src.dtype, out.dtype).items():
        if want is None:
            part[nm] = 0
        else:
            assert src.dtype[want] == out.dtype[nm], (nm, want)
            part[nm] = src[want]
    return out


def merge_tables(tables, dtype=None) -> np.ndarray:
    dtype = merged_dtype([t.dtype for t in tables]) if dtype is None else np.dtype(dtype)
    out = np.zeros(sum(len(t) for t in tables), dtype)
    row0 = 0
    for t in tables:
        merge_into(out, row0, t)
        row0 += len(t)
    return out
