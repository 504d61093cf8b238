"""``write_ksplat`` -- the reference's ``KSplatFormat.write`` (formats/ksplat.py:319-544) with its payload on the MI355X.

  | step (formats/ksplat.py)                         | here                                                             |
  |--------------------------------------------------|------------------------------------------------------------------|
  | :320-333 parameters                              | the same conversions (params)                                    |
  | :340-368 SH degree: `np.all(data[f] == 0)` per   | names on the host; the content scan is ONE device pass over the  |
  |          present f_rest_0..23, capped by sh_level | resident rows (gsx_spz_rest_nonzero_dev)                         |
  | :370-424 file and section headers                | the same struct calls on the host (headers)                      |
  | :426-450 bucket centres                          | gsx_ksplat_centres_dev, into their payload slot                  |
  | :452-536 positions, exp scales, f16 / u8 casts,  | gsx_ksplat_pack_dev: every interleaved row, one workgroup per    |
  |          colours, SH, interleaving               | row tile; numpy only for the rows and buckets the device lists   |
  | :538-542 file                                    | one write of the downloaded buffer                               |

Identical file bytes: the float32 arithmetic is numpy's, the exp is numpy's own SIMD exp (csrc/np_exp.h, probed at first use
against this process's numpy: _lib.np_exp_probe), and what depends on numpy's NaN casts or its reduction order comes from numpy.
The reference's errors are raised with its exception types and messages, and no file is created.  Errors that do not depend on
the table's SH content come before the device is touched; the few that do (an f_rest field the degree needs is absent, a
payload past the header's 32-bit size) come after the device's degree scan, still before anything is packed or the file is
opened.  Fields this writer reads that are not little-endian float32 are refused (TypeError) rather than cast.
"""
from __future__ import annotations

import struct

import numpy as np

from .. import _lib
from ..utils import debug_print

HEADER_BYTES = 4096         # ksplat.py:12
SECTION_BYTES = 1024        # :13
MAGIC = (0, 1)              # :10-11
SCALE_RANGE = 32767         # :387
MIN_SH, MAX_SH = -2.0, 2.0  # :379
FIXED_FIELDS = ["scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3", "f_dc_0", "f_dc_1", "f_dc_2", "opacity"]


def params(compression_level, kwargs):
    """:320-333 -> (level, sh_level or None, bucket_size, block_size)"""
    level = int(compression_level)
    sh_level = kwargs.get("sh_level")
    if sh_level is not None:
        sh_level = int(sh_level)
    bucket_size = kwargs.get("bucket_size")
    bucket_size = 256 if bucket_size is None else int(bucket_size)
    block_size = kwargs.get("block_size")
    block_size = 5.0 if block_size is None else float(block_size)
    return level, sh_level, bucket_size, block_size


def degree_plan(names, sh_level):
    """:340-368 on the column names -> (degree, []) where the names decide it, or (None, f_rest indices the device scans)"""
    lo = [j for j in range(9) if f"f_rest_{j}" in names]
    hi = [j for j in range(9, 24) if f"f_rest_{j}" in names]
    if sh_level is not None and sh_level <= 0:
        return sh_level, []        # below any content's degree
    if not lo:
        return 0, []
    return None, lo + (hi if sh_level is None or sh_level >= 2 else [])


def degree_from_mask(mask: int, sh_level) -> int:
    """:340-368 from the scan's bits (bit j: some row holds f_rest_j != 0)"""
    d = 0
    if mask & 0x1FF:
        d = 2 if mask & (0xFFFF << 9) else 1
    if sh_level is not None and sh_level < d:
        d = sh_level
    return d


def sh_count_of(degree: int) -> int:
    return 9 if degree == 1 else (24 if degree == 2 else 0)


def bytes_per_row(level: int, sh_count: int) -> int:
    """:401-407"""
    if level == 0:
        return 44 + 4 * sh_count
    return 24 + (2 if level == 1 else 1) * sh_count


def headers(n: int, level: int, bucket_size: int, block_size: float, degree: int):
    """:370-424 -> (file header, section header, first payload word, geometry dict); raises where the reference's struct and
    integer arithmetic raise, in its order"""
    head = bytearray(HEADER_BYTES)
    head[0], head[1] = MAGIC
    for off, v in ((4, 1), (8, 1), (12, n), (16, n)):
        struct.pack_into("<I", head, off, v)
    struct.pack_into("<H", head, 20, level)
    struct.pack_into("<f", head, 36, MIN_SH)
    struct.pack_into("<f", head, 40, MAX_SH)
    sec = bytearray(SECTION_BYTES)
    struct.pack_into("<I", sec, 0, n)
    struct.pack_into("<I", sec, 4, n)
    if level >= 1:
        struct.pack_into("<I", sec, 8, bucket_size)
        struct.pack_into("<I", sec, 12, (n + bucket_size - 1) // bucket_size)
        struct.pack_into("<f", sec, 16, block_size)
        struct.pack_into("<H", sec, 20, 12)
        struct.pack_into("<I", sec, 24, SCALE_RANGE)
    sh_count = sh_count_of(degree)
    bps = bytes_per_row(level, sh_count)
    full = n // bucket_size
    partial = 1 if n % bucket_size != 0 else 0
    n_buckets = full + partial
    centre_bytes = 12 * n_buckets if level >= 1 else 0
    storage = 4 * partial + centre_bytes + n * bps
    struct.pack_into("<I", sec, 28, storage)
    struct.pack_into("<I", sec, 32, full)
    struct.pack_into("<I", sec, 36, partial)
    struct.pack_into("<H", sec, 40, degree)
    first = struct.pack("<I", n % bucket_size) if partial else b""
    geo = dict(level=min(level, 3), sh_count=sh_count, bucket_size=bucket_size, n_buckets=n_buckets, row_base=4 * partial + centre_bytes,
               payload_bytes=storage, head=first, bps=bps)
    return bytes(head), bytes(sec), first, geo


def _no_field(data, name):
    """numpy's own error for a field the table lacks (what the reference's `data[name]` raises)"""
    return data[:0][name]


def _field(data, name):
    if name not in data.dtype.names:
        _no_field(data, name)
    dt = data.dtype.fields[name][0]
    if dt != np.dtype("<f4"):
        raise TypeError(f"KSplat writer: field {name!r} is {dt.str}; the GPU writer reads little-endian float32 ('<f4') fields only")


def check_fields(data, level: int, block_size: float, sh_count=None):
    """:415-489: the fields in the order the reference reads them, with the ZeroDivisionError of :452 where it falls
    (sh_count None: the fields before the SH block only) -> sf_inv, the Python float of :452 (None at level 0)"""
    for a in "xyz":
        _field(data, a)
    sf_inv = SCALE_RANGE / (block_size / 2.0) if level >= 1 else None
    for nm in FIXED_FIELDS:
        _field(data, nm)
    for j in range(sh_count or 0):
        _field(data, f"f_rest_{j}")
    return sf_inv


def plan(data: np.ndarray, compression_level=0, **kwargs):
    """The host's part, before the device is touched -> dict: the parameters, and the SH degree where the names decide it
    (degree) or the f_rest fields the device scans (scan).  Raises what the reference raises for the parameters and headers."""
    if data.dtype.names is None:
        raise TypeError("KSplat writer: a numpy structured array is required")
    if data.ndim != 1:
        raise TypeError("KSplat writer: a 1-D structured array is required")
    level, sh_level, bucket_size, block_size = params(compression_level, kwargs)
    n = len(data)
    degree, scan = degree_plan(data.dtype.names, sh_level)
    for j in scan:
        _field(data, f"f_rest_{j}")
    if degree is not None:
        lowest = highest = degree
    else:
        lowest, highest = 0, degree_from_mask(sum(1 << j for j in scan), sh_level)
        if any(f"f_rest_{j}" not in data.dtype.names for j in range(sh_count_of(highest))):
            # a degree the content may reach reads a field the table lacks (the reference's ValueError): decided here, on the
            # host, with the reference's own per-field test, so that the error comes before the device is touched
            degree = lowest = highest = degree_from_mask(sum(1 << j for j in scan if np.count_nonzero(data[f"f_rest_{j}"])), sh_level)
            scan = []
    headers(n, level, bucket_size, block_size, lowest)          # what every possible degree raises
    try:
        headers(n, level, bucket_size, block_size, highest)
        early = True
    except struct.error:                                        # only a content degree's payload size can raise: after the scan
        early = False
    if early:
        check_fields(data, level, block_size, sh_count_of(degree) if degree is not None else None)
    return dict(level=level, sh_level=sh_level, bucket_size=bucket_size, block_size=block_size, degree=degree, scan=scan)


def encode(data: np.ndarray, compression_level=0, stage_ms: "dict | None" = None, listed: "dict | None" = None, **kwargs):
    """-> (out, degree): the whole file's bytes (uint8 array) the reference writes"""
    p = plan(data, compression_level, **kwargs)
    n = len(data)
    level, bs, blk = p["level"], p["bucket_size"], p["block_size"]

    def geometry(degree):
        head, sec, _, g = headers(n, level, bs, blk, degree)
        sf_inv = check_fields(data, level, blk, sh_count_of(degree))
        g["py_sf_inv"] = sf_inv
        with np.errstate(over="ignore"):
            g["sf_inv"] = float(np.float32(sf_inv)) if sf_inv is not None else 0.0
        out = np.empty(HEADER_BYTES + SECTION_BYTES + g["payload_bytes"], np.uint8)
        out[:HEADER_BYTES] = np.frombuffer(head, np.uint8)
        out[HEADER_BYTES:HEADER_BYTES + SECTION_BYTES] = np.frombuffer(sec, np.uint8)
        return out, g

    if n == 0:                              # headers only: every content test of :340-368 sees no non-zero value
        degree = p["degree"] if p["degree"] is not None else degree_from_mask(0, p["sh_level"])
        out, _ = geometry(degree)
        return out, degree
    degree = p["degree"]
    if degree is None:
        sh_level = p["sh_level"]
        degree = lambda mask: degree_from_mask(mask, sh_level)   # noqa: E731
    return _lib.ksplat_pack_table(data, degree, p["scan"], geometry, stage_ms=stage_ms, listed=listed)


def write_ksplat(data: np.ndarray, path: str, compression_level=0, stage_ms: "dict | None" = None, listed: "dict | None" = None,
                 **kwargs) -> None:
    """ksplat.py:319-544.  stage_ms: a dict that receives per-stage clocks (tools/probe_ksplat.py); listed: see
    _lib.ksplat_pack_table"""
    import time
    debug_print(f"[DEBUG] Writing .ksplat file to {path}")
    out, degree = encode(data, compression_level, stage_ms, listed, **kwargs)
    t0 = time.perf_counter()
    with open(path, "wb") as f:
        f.write(memoryview(out))
    if stage_ms is not None:
        stage_ms["file_write"] = round((time.perf_counter() - t0) * 1e3, 3)
    debug_print(f"KSplat (Level {int(compression_level)}) write completed. {len(data)} points.")
