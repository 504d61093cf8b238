"""``read_splat`` -- the reference's ``SplatFormat.read`` (formats/splat.py:9-80) with its per-field decode on the MI355X.

  | step (formats/splat.py)                          | here                                                                 |
  |--------------------------------------------------|----------------------------------------------------------------------|
  | :12-21 `os.path.getsize`, the size warning, n    | the same statements in the same order (a missing path raises there)  |
  | :32 `np.fromfile` (whole records, the tail       | the first 32 n bytes read straight into page-locked staging; the     |
  |     ignored)                                     | file is opened before anything else, so a directory raises as it does |
  | :35-36 `np.zeros(n, standard_dtype)`             | the SPZ reader's degree-0 dtype, packed: 17 float32 + red green blue |
  | :38-77 the vectorised decode, field by field     | gsx_splat_unpack_dev (csrc/splat_read.hip): one launch, whole rows   |

The rows are the reference's bit for bit (".splat reader"): np.log of the scales is numpy's own float32 routine
(csrc/np_log.h, probed at first use against this process's numpy: _lib.np_log_probe; on a mismatch the scales come from numpy on
the host), the colour and opacity come from 256-entry tables numpy builds, the rest is exact IEEE arithmetic.  An empty file
returns without touching the device.
"""
from __future__ import annotations

import os
import time

import numpy as np

from .. import _lib
from ..utils import debug_print
from .spz_reader import define_dtype

RECORD_BYTES = 32                                                                  # splat.py:15


def read_splat(path: str, stage_ms: "dict | None" = None, device: int = 0, profile: "dict | None" = None, keep: "dict | None" = None) -> np.ndarray:
    """:9-80 -> the reference's structured array: define_dtype(has_scal=False, has_rgb=True, sh_degree=0), float32 fields then
    red green blue as bytes, packed; nx ny nz and red green blue zero.

    stage_ms: a dict that receives the stage clocks parse, file_read, upload, kernel, download (tools/probe_splat_read.py).  profile: a dict that receives the returned table's profile
    (_lib.TableProfile.as_dict) from one more pass over the decoded rows before their download (stage clock "profile").  keep: a dict that receives the decoded rows in HBM as keep["rows"] (_lib.ResidentRows; the caller
    closes it) when the returned table's rows are resident; it stays empty otherwise."""
    return _lib.with_keep(keep, lambda: _lib.with_profile(profile, lambda: _read(path, stage_ms, device, profile, keep)))


def _read(path, stage_ms, device, profile, keep=None):
    debug_print(f"[DEBUG] Reading .splat file from {path}")
    t0 = time.perf_counter()
    file_size = os.path.getsize(path)
    if file_size % RECORD_BYTES != 0:
        debug_print(f"[WARNING] File size {file_size} is not a multiple of {RECORD_BYTES}. Truncation may occur.")
    n = file_size // RECORD_BYTES
    debug_print(f"[DEBUG] Estimated {n} splats based on file size.")
    with open(path, "rb"):                                                         # :32 np.fromfile opens it whatever its size
        pass
    dtype = define_dtype(0)
    if stage_ms is not None:
        stage_ms["parse"] = round((time.perf_counter() - t0) * 1e3, 3)
    if n == 0:
        return np.zeros(0, dtype)
    rows = _lib.splat_unpack_table(path, n, dtype, stage_ms=stage_ms, device=device, **_lib.profile_kw(profile), **_lib.keep_kw(keep))
    debug_print(f"[DEBUG] Loaded {n} points from .splat")
    return rows


def bind_read(original):
    """-> a replacement for ``SplatFormat.read`` that decodes on the device (every .splat file is taken: `original`, the
    reference's read, is kept only for uninstall())"""
    def read(self, path, **kwargs):
        return read_splat(path)
    read.__wrapped__ = original
    return read
