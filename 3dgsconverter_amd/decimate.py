"""Voxel decimation's plan (numpy only, no device): ``plan_decimate`` decides from a table's dtype alone which fields the device
kernels (csrc/decimate.hip) read, average or copy, and raises every refusal before any device work -- the role
transform.plan_transform has for a scene transform.

All splats of a voxel of side ``voxel_size`` are replaced by the single Gaussian that has their combined weight, mean and
covariance (the definition is tests/decimate_numpy.py).  A field of a row belongs to one of four classes:

  geometry   x y z, scale_0..2, rot_0..3, opacity: read for the moments, rewritten from the merged Gaussian
  mean       f_dc_*, f_rest_*, nx ny nz: the weighted mean of the members, float32
  colour     red green blue (u1, all three): the weighted mean, rounded and clipped
  copy       everything else: the first member's bytes
"""
from __future__ import annotations

import math
import re

import numpy as np

XYZ = ("x", "y", "z")
SCALES = ("scale_0", "scale_1", "scale_2")
ROTS = ("rot_0", "rot_1", "rot_2", "rot_3")
GEOMETRY = XYZ + SCALES + ROTS + ("opacity",)
RGB = ("red", "green", "blue")
MAX_MEAN = 51        # GSX_DECIMATE_MAX_MEAN: 3 f_dc + 45 f_rest + 3 normals
MAX_ZERO = 128       # GSX_DECIMATE_MAX_ZERO
MAX_ROW_BYTES = 512  # csrc/row_tile.h SPZ_MAX_ROW_BYTES
_MEAN = re.compile(r"f_dc_\d+|f_rest_\d+|nx|ny|nz")


def check_voxel_size(voxel_size) -> float:
    """-> the voxel size as a float; ValueError unless it is a finite number greater than 0"""
    try:
        h = float(voxel_size)
    except (TypeError, ValueError):
        raise ValueError(f"decimate: the voxel size must be a finite number greater than 0, got {voxel_size!r}") from None
    if isinstance(voxel_size, (bool, np.bool_)) or not math.isfinite(h) or h <= 0:
        raise ValueError(f"decimate: the voxel size must be a finite number greater than 0, got {voxel_size!r}")
    return h


def missing_fields(dtype):
    """the geometry fields a table of `dtype` lacks (none: the table can be decimated)"""
    names = np.dtype(dtype).names or ()
    return tuple(nm for nm in GEOMETRY if nm not in names)


class DecimatePlan:
    """What plan_decimate decides: the voxel size, the byte offsets of the geometry fields, ``mean`` ((name, offset) of the
    averaged float32 fields, in the dtype's order), ``u8`` (of the three colour bytes, or empty), ``zero`` (of the fields zeroed
    in every output row) and ``float_names`` (every '<f4' field: where a NaN may differ in its payload)."""

    def __init__(self):
        self.dtype = None
        self.voxel_size = 0.0
        self.xyz = self.scales = (-1, -1, -1)
        self.rots = (-1, -1, -1, -1)
        self.opacity = -1
        self.mean = ()
        self.u8 = ()
        self.zero = ()
        self.float_names = ()


def plan_decimate(dtype, voxel_size, zero_names=()) -> DecimatePlan:
    """The decimation of a table of `dtype` at `voxel_size`.  Every refusal is raised here: ValueError for a voxel size that is
    not a finite number above 0, a table that lacks a geometry field (missing_fields tells beforehand), rows above 512 bytes,
    more averaged fields than the kernel has lanes for, or a zeroed field that is a geometry field; TypeError, naming the field,
    for a field the kernels read or write as float32 that is not '<f4' (no silent casts)."""
    dtype = np.dtype(dtype)
    fields = dtype.fields or {}
    p = DecimatePlan()
    p.dtype = dtype
    p.voxel_size = check_voxel_size(voxel_size)
    lacking = missing_fields(dtype)
    if lacking:
        raise ValueError(f"decimate: the table has no field {lacking[0]!r}; x y z, scale_0..2, rot_0..3 and opacity are needed")
    if not 1 <= dtype.itemsize <= MAX_ROW_BYTES:
        raise ValueError(f"decimate: rows of {dtype.itemsize} bytes (1 ... {MAX_ROW_BYTES} are supported)")
    mean = tuple(nm for nm in dtype.names if _MEAN.fullmatch(nm))
    f4 = np.dtype("<f4")
    for nm in GEOMETRY + mean:
        if fields[nm][0] != f4:
            raise TypeError(f"decimate: field {nm!r} is {fields[nm][0].str}, and the merge reads and writes '<f4' fields only "
                            f"(no silent casts) -- cast the table to float32 first if that is what is wanted")
    if len(mean) > MAX_MEAN:
        raise ValueError(f"decimate: {len(mean)} averaged fields (f_dc_*, f_rest_*, normals); at most {MAX_MEAN} are supported")
    off = lambda names: tuple(int(fields[nm][1]) for nm in names)
    p.xyz, p.scales, p.rots, p.opacity = off(XYZ), off(SCALES), off(ROTS), int(fields["opacity"][1])
    p.mean = tuple((nm, int(fields[nm][1])) for nm in mean)
    if all(nm in fields and fields[nm][0] == np.dtype("u1") for nm in RGB):
        p.u8 = tuple((nm, int(fields[nm][1])) for nm in RGB)
    p.zero = zero_fields(dtype, zero_names)
    p.float_names = tuple(nm for nm in dtype.names if fields[nm][0] == f4)
    return p


def zero_fields(dtype, zero_names) -> tuple:
    """-> (name, byte offset) of the fields among `zero_names` that a table of `dtype` has, for the zero fill of every output
    row (cap_sh_degree's deferred columns).  ValueError for a geometry field -- the merge is computed from it -- or more than
    the kernel takes; TypeError for a field that is not 4 bytes wide."""
    fields = np.dtype(dtype).fields or {}
    zero = []
    for nm in zero_names:
        if nm not in fields:
            continue
        if nm in GEOMETRY:
            raise ValueError(f"decimate: field {nm!r} cannot be zeroed: the merge is computed from it")
        if fields[nm][0].itemsize != 4:
            raise TypeError(f"decimate: zeroed field {nm!r} is {fields[nm][0].str}; 4-byte fields only")
        zero.append((nm, int(fields[nm][1])))
    if len(zero) > MAX_ZERO:
        raise ValueError(f"decimate: {len(zero)} zeroed fields; at most {MAX_ZERO} are supported")
    return tuple(zero)
