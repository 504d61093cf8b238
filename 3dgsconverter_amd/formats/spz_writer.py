"""``write_spz`` -- the reference's ``SpzFormat.write`` (formats/spz.py:49-109) with its body on the MI355X.

  | step (formats/spz.py)                          | here                                                             |
  |------------------------------------------------|------------------------------------------------------------------|
  | :52-77 SH degree: naive by columns, then       | names on the host; the content scan is ONE device pass over the  |
  |        `np.any(data[f] != 0)` per f_rest column | resident rows (gsx_spz_rest_nonzero_dev)                         |
  | :111-170 `_pack_v3`, :298-343 `_pack_rot_v3`   | gsx_spz_pack_dev: the whole body, one workgroup per row tile;    |
  |                                                | numpy only for the listed alpha bytes / NaN rotation words       |
  | :92-103 header, gzip, file                     | the same calls on the host, on the downloaded buffer             |

Identical file bytes: the gzip container is Python's own ``gzip.compress`` of an identical payload.  Tables whose fields this
writer reads are not little-endian float32 are refused (TypeError) rather than cast; a table that lacks a field the reference
reads raises numpy's own ValueError, before any file is created.
"""
from __future__ import annotations

import gzip
import struct

import numpy as np

from .. import _lib
from ..utils import debug_print, status_print

MAGIC = 0x5053474E        # spz.py:11
VERSION = 3
FRACTIONAL_BITS = 12      # :86
FLAGS = 1                 # :96 FlagAntialiased
HEADER = "<IIIBBBB"

_MAX_IDX = {3: 44, 2: 23, 1: 8}


def naive_degree(names) -> int:
    """:55-58 -- the degree the f_rest columns allow"""
    if "f_rest_0" not in names:
        return 0
    if "f_rest_44" in names:
        return 3
    if "f_rest_23" in names:
        return 2
    if "f_rest_8" in names:
        return 1
    return 0


def degree_from_last_index(last_active_idx: int) -> int:
    """:72-75"""
    if last_active_idx >= 24:
        return 3
    if last_active_idx >= 9:
        return 2
    if last_active_idx >= 0:
        return 1
    return 0


def sh_fields(degree: int):
    """:152-154 -- the f_rest fields the body reads for a degree, in the order the reference reads them"""
    d = _lib.SPZ_SH_DIM[degree]
    return [f"f_rest_{i + 15 * c}" for c in range(3) for i in range(d)]


def _no_field(data, name):
    """numpy's own error for a field the table lacks (what the reference's `data[name]` raises)"""
    return data[:0][name]


def _check_f4(data, name):
    dt = data.dtype.fields[name][0]
    if dt != np.dtype("<f4"):
        raise TypeError(f"SPZ writer: field {name!r} is {dt.str}; the GPU writer reads little-endian float32 ('<f4') fields only")


def plan(data: np.ndarray):
    """The host's part, before the device is touched: every check, and the SH degree where the table's columns decide it
    (-> degree), or the f_rest fields whose content the device scans (-> None, scan).  Raises ValueError / TypeError."""
    names = data.dtype.names
    if names is None:
        raise TypeError("SPZ writer: a numpy structured array is required")
    if data.ndim != 1:
        raise TypeError("SPZ writer: a 1-D structured array is required")
    naive = naive_degree(names)
    scan = [i for i in range(_MAX_IDX[naive], -1, -1) if f"f_rest_{i}" in names] if naive else []
    # the fields the body reads whatever the content, in the reference's order (:113, :119, :127-129, :137-139, :145)
    used = ["x", "y", "z"] + (["opacity"] if "opacity" in names else [])
    used += (["f_dc_0", "f_dc_1", "f_dc_2"] if "f_dc_0" in names else []) + ["scale_0", "scale_1", "scale_2"]
    used += ["rot_0", "rot_1", "rot_2", "rot_3"]
    for nm in used:
        if nm not in names:
            _no_field(data, nm)
        _check_f4(data, nm)
    for i in scan:
        _check_f4(data, f"f_rest_{i}")
    if not scan:
        return 0, []
    if all(f in names for f in sh_fields(naive)):
        return None, scan          # every degree up to the naive one has its fields: the device decides
    # a table of 9 or 24 coefficients: the stride-15 read can miss a field, and the reference then raises -- decided here, on the host
    last = -1
    for i in scan:
        if np.any(data[f"f_rest_{i}"] != 0):
            last = i
            break
    degree = degree_from_last_index(last)
    for f in sh_fields(degree):
        if f not in names:
            _no_field(data, f)
    return degree, []


def encode(data: np.ndarray, stage_ms: "dict | None" = None, listed: "dict | None" = None):
    """-> (payload, degree): the uncompressed file content (header + body, a uint8 array) the reference hands to gzip"""
    num_points = len(data)
    degree, scan = plan(data)
    struct.pack("<I", num_points)                  # :98: n must fit in a uint32 (struct.error, as in the reference)
    if num_points == 0:
        out, degree = np.zeros(_lib.SPZ_HEADER_BYTES, np.uint8), degree or 0
    else:
        data = np.ascontiguousarray(data)
        out, degree = _lib.spz_pack_table(data, degree_from_last_index if degree is None else degree, scan, stage_ms=stage_ms,
                                          listed=listed)
    out[:_lib.SPZ_HEADER_BYTES] = np.frombuffer(struct.pack(HEADER, MAGIC, VERSION, num_points, degree, FRACTIONAL_BITS, FLAGS, 0),
                                                np.uint8)
    return out, degree


def write_spz(data: np.ndarray, path: str, stage_ms: "dict | None" = None, listed: "dict | None" = None, **kwargs) -> None:
    """spz.py:49-109.  stage_ms: a dict that receives per-stage clocks (tools/probe_spz.py); listed: see _lib.spz_pack_table"""
    import time
    out, degree = encode(data, stage_ms, listed)
    debug_print(f"[DEBUG] SPZ Write: Detected effective SH degree {degree} (from content).")
    t0 = time.perf_counter()
    comp_level = kwargs.get("compression_level", 0)
    compressed = gzip.compress(memoryview(out), compresslevel=comp_level)
    t1 = time.perf_counter()
    with open(path, "wb") as f:
        f.write(compressed)
    if stage_ms is not None:
        stage_ms["gzip"] = round((t1 - t0) * 1e3, 3)
        stage_ms["file_write"] = round((time.perf_counter() - t1) * 1e3, 3)
    status_print(f"Native SPZ (v3, no-flip, lvl={comp_level}) export completed. {len(data)} points.")
