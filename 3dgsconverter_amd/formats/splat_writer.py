"""``write_splat`` -- the reference's ``SplatFormat.write`` (formats/splat.py:82-166) with its sort and records on the MI355X.

  | step (formats/splat.py)                          | here                                                             |
  |--------------------------------------------------|------------------------------------------------------------------|
  | :92-94 metric exp((s0 + s1) + s2) * sigmoid(o)   | gsx_splat_pack_dev: the sort key of -metric per row, in the same |
  | :104-161 positions, np.exp scales, colour and    | pass as the row's 32-byte record (input order, row tiles staged  |
  |          alpha u8, normalised rotation u8        | in LDS)                                                          |
  | :98 np.argsort(-metric)                          | gsx_splat_order_dev: a stable radix sort of (key, row index)     |
  | :101 data[sorted_indices]                        | gsx_splat_permute_dev on the 32-byte records, not the raw rows   |
  | :163-164 file                                    | one write of the downloaded buffer                               |

Identical records: the float32 arithmetic is numpy's, in numpy's order, and the exp is numpy's own SIMD exp (csrc/np_exp.h,
probed at first use against this process's numpy: _lib.np_exp_probe; on a mismatch the metric, scales and alpha come from
numpy).  The order is ``np.argsort(-metric, kind="stable")``: the reference's sort is numpy's unstable default, whose order
inside a run of equal metrics depends on numpy's build and the CPU; here equal keys keep input order (-0.0 equals +0.0, NaNs
sort last and tie with each other).  On tables without ties the file is the reference's, byte for byte.  The reference's
errors (a missing field: numpy's ValueError) come before the device is touched, and no file is created.  Float fields this
writer reads that are not little-endian float32, and red / green / blue that are not u1, are refused (TypeError).
"""
from __future__ import annotations

import numpy as np

from .. import _lib
from ..utils import debug_print

METRIC_FIELDS = ["scale_0", "scale_1", "scale_2", "opacity"]                                  # :92-93
RECORD_FIELDS = ["x", "y", "z", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]   # :104-113
DC_FIELDS = ["f_dc_0", "f_dc_1", "f_dc_2"]                                                    # :134-138
RGB_FIELDS = ["red", "green", "blue"]                                                         # :140-143


def _no_field(data, name):
    """numpy's own error for a field the table lacks (what the reference's `data[name]` raises)"""
    return data[:0][name]


def check_fields(data: np.ndarray) -> bool:
    """the fields in the order the reference reads them -> rgb (True: the colour comes from the u1 fields red, green, blue)"""
    if data.dtype.names is None:
        raise TypeError("Splat writer: a numpy structured array is required")
    if data.ndim != 1:
        raise TypeError("Splat writer: a 1-D structured array is required")
    names = data.dtype.names
    rgb = "f_dc_0" not in names
    reads = METRIC_FIELDS + RECORD_FIELDS + (RGB_FIELDS if rgb else DC_FIELDS)
    for nm in reads:
        if nm not in names:
            _no_field(data, nm)
    for nm in reads:
        dt = data.dtype.fields[nm][0]
        want = np.dtype("u1") if nm in RGB_FIELDS else np.dtype("<f4")
        if dt != want:
            raise TypeError(f"Splat writer: field {nm!r} is {dt.str}; the GPU writer reads {want.str!r} here")
    return rgb


def encode(data: np.ndarray, listed: "dict | None" = None, stage_ms: "dict | None" = None, resident=None) -> np.ndarray:
    """-> uint8[32 n]: the file's bytes"""
    rgb = check_fields(data)
    if len(data) == 0:
        return np.empty(0, np.uint8)
    return _lib.splat_pack_table(data, rgb, stage_ms=stage_ms, listed=listed, **({} if resident is None else {"resident": resident}))


def write_splat(data: np.ndarray, path: str, stage_ms: "dict | None" = None, listed: "dict | None" = None, resident=None, **kwargs) -> None:
    """splat.py:82-166.  stage_ms: a dict that receives per-stage clocks (tools/probe_splat.py); listed: see
    _lib.splat_pack_table.  resident: the rows of `data` in HBM (_lib.ResidentRows, the caller's, not closed here): when they
    match `data` by count and dtype the table is not uploaded and stage_ms has no "upload" key"""
    import time
    debug_print(f"[DEBUG] Writing .splat file to {path}")
    out = encode(data, listed, stage_ms, resident)
    t0 = time.perf_counter()
    with open(path, "wb") as f:
        f.write(memoryview(out))
    if stage_ms is not None:
        stage_ms["file_write"] = round((time.perf_counter() - t0) * 1e3, 3)
    debug_print(f".splat write completed. {len(data)} splats sorted and packed.")
