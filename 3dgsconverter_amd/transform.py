"""The host mathematics of a scene transform ``p' = s R p + t`` (float64, numpy only, no device): the rotation from Euler
angles, its quaternion, the matrices that rotate the spherical-harmonic bands 1..3 of the 3DGS rasteriser's real basis, and
``plan_transform``, which decides from a table's dtype alone which fields the device kernel (csrc/transform.hip) rewrites.

A splat cannot be moved by editing x y z alone: the log-scales grow with log(s), the orientation quaternion is multiplied by
the rotation's, and every SH band above DC is rotated with the scene -- ``c' = D c`` per colour channel and band, where
``sum_k c'_k Y_k(R d) = sum_k c_k Y_k(d)`` for every unit direction d.
"""
from __future__ import annotations

import math
import re

import numpy as np

C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)

XYZ = ("x", "y", "z")
NORMALS = ("nx", "ny", "nz")
SCALES = ("scale_0", "scale_1", "scale_2")
ROTS = ("rot_0", "rot_1", "rot_2", "rot_3")
PART_POSITION, PART_NORMALS, PART_SCALES, PART_ROTATION, PART_SH1, PART_SH2, PART_SH3 = 1, 2, 4, 8, 16, 32, 64   # GSX_TF_* (include/gsx_hip.h)
SNAP = 1e-12

# The directions the band matrices are fitted on: the 48 images of (1, 2, 3) under the axis permutations and sign changes,
# normalised.  Integers, a square root and a division: the same float64 values everywhere.  An orbit of the cube's symmetry
# group spreads evenly over the sphere; the fit's condition numbers on it are 1.0, 1.41 and 1.38 for the bands 1, 2, 3.
FIT_DIRECTIONS = tuple((sx * p[0], sy * p[1], sz * p[2])
                       for p in ((1, 2, 3), (1, 3, 2), (2, 1, 3), (2, 3, 1), (3, 1, 2), (3, 2, 1))
                       for sx in (1, -1) for sy in (1, -1) for sz in (1, -1))


def _axis_sin_cos(deg: float):
    """(sin, cos) of an angle in degrees; a whole multiple of 90 takes them from the exact values 0, +-1"""
    deg = float(deg)
    quarter = deg / 90.0
    if quarter == math.floor(quarter) and math.isfinite(quarter):
        return ((0.0, 1.0), (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0))[int(quarter) % 4]
    r = math.radians(deg)
    return math.sin(r), math.cos(r)


def rotation_from_euler_deg(rx, ry, rz) -> np.ndarray:
    """Rz(rz) Ry(ry) Rx(rx): about the fixed X axis, then the fixed Y axis, then the fixed Z axis"""
    for v in (rx, ry, rz):
        if not math.isfinite(float(v)):
            raise ValueError(f"transform: the rotation angles must be finite, got [{rx}, {ry}, {rz}]")
    (sx, cx), (sy, cy), (sz, cz) = _axis_sin_cos(rx), _axis_sin_cos(ry), _axis_sin_cos(rz)
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    Rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    return (Rz @ Ry @ Rx) + 0.0     # (+ 0.0: no negative zero in a signed permutation matrix)


def check_rotation(R) -> np.ndarray:
    """-> R as a float64 (3, 3) array, used as given; ValueError unless it is finite, orthonormal to 1e-9 and proper"""
    try:
        A = np.array(R, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("transform: the rotation must be a 3x3 matrix") from None
    if A.shape != (3, 3):
        raise ValueError(f"transform: the rotation must be a 3x3 matrix, got shape {A.shape}")
    if not np.all(np.isfinite(A)):
        raise ValueError("transform: the rotation matrix must be finite")
    err = float(np.max(np.abs(A @ A.T - np.eye(3))))
    if err > 1e-9:
        raise ValueError(f"transform: the rotation matrix is not orthonormal (max|R R^T - I| = {err:.3g}, at most 1e-9)")
    if np.linalg.det(A) <= 0:
        raise ValueError("transform: the rotation matrix is a reflection (det R < 0); a proper rotation is needed")
    return A


def quat_from_rotation(R) -> tuple:
    """(w, x, y, z) with w >= 0 of the rotation matrix R, by Shepperd's method: the largest of the four candidates under the
    root, the other three from the off-diagonal sums and differences"""
    R = np.asarray(R, dtype=np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    cands = (tr, R[0, 0], R[1, 1], R[2, 2])
    i = max(range(4), key=lambda k: cands[k])
    if i == 0:
        w = 0.5 * math.sqrt(max(1.0 + tr, 0.0))
        f = 0.25 / w
        q = (w, (R[2, 1] - R[1, 2]) * f, (R[0, 2] - R[2, 0]) * f, (R[1, 0] - R[0, 1]) * f)
    elif i == 1:
        x = 0.5 * math.sqrt(max(1.0 + R[0, 0] - R[1, 1] - R[2, 2], 0.0))
        f = 0.25 / x
        q = ((R[2, 1] - R[1, 2]) * f, x, (R[0, 1] + R[1, 0]) * f, (R[0, 2] + R[2, 0]) * f)
    elif i == 2:
        y = 0.5 * math.sqrt(max(1.0 - R[0, 0] + R[1, 1] - R[2, 2], 0.0))
        f = 0.25 / y
        q = ((R[0, 2] - R[2, 0]) * f, (R[0, 1] + R[1, 0]) * f, y, (R[1, 2] + R[2, 1]) * f)
    else:
        z = 0.5 * math.sqrt(max(1.0 - R[0, 0] - R[1, 1] + R[2, 2], 0.0))
        f = 0.25 / z
        q = ((R[1, 0] - R[0, 1]) * f, (R[0, 2] + R[2, 0]) * f, (R[1, 2] + R[2, 1]) * f, z)
    q = tuple(float(v) + 0.0 for v in q)
    if q[0] < 0:
        q = tuple(-v + 0.0 for v in q)
    return q


def sh_basis(dirs, band: int) -> np.ndarray:
    """the 2 band + 1 functions of one band of the 3DGS rasteriser's real basis, in f_rest order, on (n, 3) unit directions"""
    d = np.asarray(dirs, dtype=np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz = x * x, y * y, z * z
    if band == 1:
        cols = [-C1 * y, C1 * z, -C1 * x]
    elif band == 2:
        cols = [C2[0] * x * y, C2[1] * y * z, C2[2] * (2.0 * zz - xx - yy), C2[3] * x * z, C2[4] * (xx - yy)]
    elif band == 3:
        cols = [C3[0] * y * (3.0 * xx - yy), C3[1] * x * y * z, C3[2] * y * (4.0 * zz - xx - yy), C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy),
                C3[4] * x * (4.0 * zz - xx - yy), C3[5] * z * (xx - yy), C3[6] * x * (xx - 3.0 * yy)]
    else:
        raise ValueError(f"sh_basis: band {band} (1 ... 3)")
    return np.stack(cols, axis=1)


def fit_directions() -> np.ndarray:
    d = np.array(FIT_DIRECTIONS, dtype=np.float64)
    return d / np.sqrt(np.sum(d * d, axis=1, keepdims=True))


def sh_rotation(R):
    """-> (D1 (3, 3), D2 (5, 5), D3 (7, 7)): c' = D c rotates the coefficients of one colour channel and one band with the scene.
    Least squares over FIT_DIRECTIONS: Y(dirs R^T) D = Y(dirs) per band; entries within 1e-12 of 0, +1 or -1 are those values
    (the identity and the axis permutations give exact matrices)."""
    R = np.asarray(R, dtype=np.float64)
    dirs = fit_directions()
    moved = dirs @ R.T
    out = []
    for band in (1, 2, 3):
        D = np.linalg.lstsq(sh_basis(moved, band), sh_basis(dirs, band), rcond=None)[0]
        for v in (0.0, 1.0, -1.0):
            D[np.abs(D - v) <= SNAP] = v
        out.append(np.ascontiguousarray(D))
    return tuple(out)


class TransformPlan:
    """What plan_transform decides: the numbers of the transform (R, s, t, M = s R, q_R, float32 log(s), D1..D3), the byte
    offsets of the fields it may touch (-1: absent), ``parts`` (the PART_* bits of the parts the kernel rewrites) and
    ``written`` (their field names).  ``identity``: there is nothing to do, not even on the device."""

    def __init__(self):
        self.dtype = None
        self.R = np.eye(3)
        self.s = 1.0
        self.t = np.zeros(3)
        self.M = np.eye(3)
        self.q = (1.0, 0.0, 0.0, 0.0)
        self.log_scale = np.float32(0.0)
        self.D = (np.eye(3), np.eye(5), np.eye(7))
        self.xyz = self.normals = self.scales = (-1, -1, -1)
        self.rots = (-1, -1, -1, -1)
        self.rest = ()
        self.m = 0
        self.parts = 0
        self.written = ()
        self.identity = True


def _offsets(fields, names):
    return tuple(int(fields[nm][1]) for nm in names) if all(nm in fields for nm in names) else (-1,) * len(names)


def plan_transform(dtype, R=None, s=None, t=None) -> TransformPlan:
    """The transform p' = s R p + t of a table of `dtype` (None: the identity rotation, scale 1, no translation).  Every
    refusal is raised here, before any device work: ValueError for a table without x y z, a matrix that is no proper rotation,
    a scale that is not a finite number above 0, a translation that is not finite, and -- under a rotation -- f_rest fields that
    are no whole bands of three channels; TypeError, naming the field, for a field the transform would write that is not
    '<f4' (no silent casts)."""
    dtype = np.dtype(dtype)
    fields = dtype.fields or {}
    for nm in XYZ:
        if nm not in fields:
            raise ValueError(f"transform: the table has no field {nm!r}; x, y and z are needed")
    p = TransformPlan()
    p.dtype = dtype
    p.R = check_rotation(np.eye(3) if R is None else R)
    try:
        p.s = float(1.0 if s is None else s)
    except (TypeError, ValueError):
        raise ValueError(f"transform: the scale must be a finite number greater than 0, got {s!r}") from None
    if not math.isfinite(p.s) or p.s <= 0:
        raise ValueError(f"transform: the scale must be a finite number greater than 0, got {p.s}")
    try:
        p.t = np.array([0.0, 0.0, 0.0] if t is None else t, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"transform: the translation must be three finite numbers, got {t!r}") from None
    if p.t.shape != (3,) or not np.all(np.isfinite(p.t)):
        raise ValueError(f"transform: the translation must be three finite numbers, got {t!r}")
    rotates = not np.array_equal(p.R, np.eye(3))
    scales = p.s != 1.0
    p.identity = not rotates and not scales and not np.any(p.t != 0)

    p.xyz, p.normals, p.scales, p.rots = (_offsets(fields, names) for names in (XYZ, NORMALS, SCALES, ROTS))
    rest_ids = sorted(int(m.group(1)) for m in (re.fullmatch(r"f_rest_(\d+)", nm) for nm in dtype.names) if m)
    n_rest = len(rest_ids)
    written = list(XYZ)
    parts = PART_POSITION
    if scales and p.scales[0] >= 0:
        parts |= PART_SCALES
        written += SCALES
    if rotates:
        if p.normals[0] >= 0:
            parts |= PART_NORMALS
            written += NORMALS
        if p.rots[0] >= 0:
            parts |= PART_ROTATION
            written += ROTS
        if rest_ids != list(range(n_rest)) or n_rest % 3 or n_rest // 3 not in (0, 3, 8, 15):
            raise ValueError(f"transform: {n_rest} f_rest fields cannot be rotated: whole bands of three colour channels are "
                             f"needed (0, 9, 24 or 45 fields named f_rest_0 ...)")
        p.m = n_rest // 3
        p.rest = tuple(int(fields[f"f_rest_{i}"][1]) for i in range(n_rest))
        for band, bit in ((1, PART_SH1), (2, PART_SH2), (3, PART_SH3)):
            if p.m >= band * band + 2 * band:
                parts |= bit
        written += [f"f_rest_{c * p.m + k}" for c in range(3) for k in range(p.m)]
    for nm in written:
        if fields[nm][0] != np.dtype("<f4"):
            raise TypeError(f"transform: field {nm!r} is {fields[nm][0].str}, and the transform writes '<f4' fields only "
                            f"(no silent casts) -- cast the table to float32 first if that is what is wanted")
    p.parts, p.written = parts, tuple(written)
    p.M = np.float64(p.s) * p.R
    p.log_scale = np.float32(np.log(np.float64(p.s)))
    if rotates:
        p.q = quat_from_rotation(p.R)
        p.D = sh_rotation(p.R)
    return p
