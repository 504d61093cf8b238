"""The preview renderer's host side (numpy, zlib and struct only; no device): ``plan_camera`` frames a scene from its bounding
box, ``plan_render`` decides from a table's dtype alone which fields the rasteriser (csrc/render.hip) reads and raises every
refusal before any device work -- the role decimate.plan_decimate has for the decimation -- and ``write_png`` stores the
(h, w, 3) uint8 image.

The image is a tile-based forward pass over 3D Gaussian splats (the definition is tests/render_numpy.py): a
pinhole camera with x right, y down, z forward, pixel samples at integer coordinates (row 0 is the top), splats blended front
to back in the order of (float32 depth, row).  It depends on the rows and the camera alone.
"""
from __future__ import annotations

import math
import re
import struct
import zlib

import numpy as np

XYZ = ("x", "y", "z")
SCALES = ("scale_0", "scale_1", "scale_2")
ROTS = ("rot_0", "rot_1", "rot_2", "rot_3")
GEOMETRY = XYZ + SCALES + ROTS + ("opacity",)
DC = ("f_dc_0", "f_dc_1", "f_dc_2")
RGB = ("red", "green", "blue")
MAX_ROW_BYTES = 512          # csrc/row_tile.h SPZ_MAX_ROW_BYTES
MAX_SIDE = 8192              # GSX_RENDER_MAX_SIDE
DEFAULT_MAX_WORK_BYTES = 4 << 30
UP_AXES = {"+x": (1.0, 0.0, 0.0), "-x": (-1.0, 0.0, 0.0), "+y": (0.0, 1.0, 0.0), "-y": (0.0, -1.0, 0.0), "+z": (0.0, 0.0, 1.0),
           "-z": (0.0, 0.0, -1.0)}


class RenderRefused(ValueError):
    """the scene needs more instance workspace than the plan's ``max_work_bytes``: nothing was allocated for it, no image exists"""


class Camera:
    """A pinhole camera: ``view`` (3, 4) float64 maps a world point to camera coordinates (x right, y down, z forward), ``eye``
    its position, ``fx fy cx cy`` the projection u = fx x / z + cx, ``tan_fovx tan_fovy`` the tangents of the half angles,
    ``near`` the depth at or below which a splat is not drawn, ``width`` x ``height`` the image."""

    def __init__(self, width, height, view, eye, fx, fy, cx, cy, tan_fovx, tan_fovy, near):
        self.width, self.height = int(width), int(height)
        self.view = np.array(view, dtype=np.float64).reshape(3, 4)
        self.eye = np.array(eye, dtype=np.float64).reshape(3)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.tan_fovx, self.tan_fovy, self.near = float(tan_fovx), float(tan_fovy), float(near)


def check_size(size) -> tuple:
    """-> (width, height) as ints; ValueError unless both are whole numbers in 1 ... 8192"""
    try:
        w, h = size
        ok = float(w) == int(w) and float(h) == int(h) and 1 <= int(w) <= MAX_SIDE and 1 <= int(h) <= MAX_SIDE
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"render: the image size must be two whole numbers in 1 ... {MAX_SIDE}, got {size!r}")
    return int(w), int(h)


def up_vector(up) -> np.ndarray:
    """'+x' '-x' '+y' '-y' '+z' '-z' (a bare 'x' is '+x') -> the unit vector"""
    name = str(up).strip().lower()
    name = "+" + name if name in ("x", "y", "z") else name
    if name not in UP_AXES:
        raise ValueError(f"render: up must be one of {' '.join(UP_AXES)}, got {up!r}")
    return np.array(UP_AXES[name], dtype=np.float64)


def look_at(eye, target, up) -> np.ndarray:
    """-> the (3, 4) view matrix of a camera at `eye` that looks at `target`: rows right, down, forward with
    right = forward x up and down = forward x right, each followed by minus its product with the eye.  A forward axis along
    `up` takes the next coordinate axis in its place."""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    f = target - eye
    norm = math.sqrt(float(f @ f))
    if not math.isfinite(norm) or norm == 0:
        raise ValueError("render: the camera's eye and target must be two different finite points")
    f = f / norm
    r = np.cross(f, up)
    if float(r @ r) < 1e-24:
        r = np.cross(f, np.roll(np.abs(up), 1))
    r = r / math.sqrt(float(r @ r))
    d = np.cross(f, r)
    R = np.stack([r, d, f]) + 0.0
    return np.concatenate([R, -(R @ eye).reshape(3, 1)], axis=1)


def plan_camera(lo, hi, size, view=(35, 20), up="-y", fov=50, camera=None) -> Camera:
    """The camera of a preview (host only, float64).  size = (width, height); fov: the vertical field of view in degrees, in
    (0, 170); up: one of +-x +-y +-z, by default -y (COLMAP's and 3DGS's y points down).

    Without `camera`: the target is the centre of the box lo ... hi, the eye stands at azimuth view[0] and elevation view[1]
    (degrees, about `up`) at the distance 1.05 R / sin(min(fovx, fovy) / 2), R the box's half diagonal -- the box's bounding
    sphere lies inside the image --, and near is 1 % of that distance.  An axis whose bounds are not finite (a profile reports
    NaN for an axis that holds one, and infinities for an empty table) counts as the single value 0; R = 0 frames a unit sphere.
    camera = (ex, ey, ez, tx, ty, tz): the eye and the target as given; near is 1 % of their distance."""
    w, h = check_size(size)
    try:
        fov = float(fov)
    except (TypeError, ValueError):
        raise ValueError(f"render: the field of view must be a number of degrees in (0, 170), got {fov!r}") from None
    if not 0.0 < fov < 170.0:
        raise ValueError(f"render: the field of view must be a number of degrees in (0, 170), got {fov!r}")
    upv = up_vector(up)
    tan_y = math.tan(math.radians(fov) / 2.0)
    tan_x = tan_y * w / h
    fx, fy = w / (2.0 * tan_x), h / (2.0 * tan_y)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0           # pixel samples sit at integer coordinates
    if camera is not None:
        try:
            c = [float(v) for v in camera]
        except (TypeError, ValueError):
            c = []
        if len(c) != 6 or not all(math.isfinite(v) for v in c):
            raise ValueError(f"render: the camera must be six finite numbers (eye, then target), got {camera!r}")
        eye, target = np.array(c[:3]), np.array(c[3:])
        dist = math.sqrt(float((eye - target) @ (eye - target)))
    else:
        try:
            az, el = (float(v) for v in view)
        except (TypeError, ValueError):
            raise ValueError(f"render: the view must be two angles in degrees (azimuth, elevation), got {view!r}") from None
        if not math.isfinite(az) or not -90.0 <= el <= 90.0:
            raise ValueError(f"render: the view must be a finite azimuth and an elevation in -90 ... 90 degrees, got {view!r}")
        lo, hi = np.array(lo, dtype=np.float64).reshape(3), np.array(hi, dtype=np.float64).reshape(3)
        bad = ~(np.isfinite(lo) & np.isfinite(hi))
        lo[bad], hi[bad] = 0.0, 0.0
        target = 0.5 * (lo + hi)
        half = 0.5 * (hi - lo)
        R = math.sqrt(float(half @ half))
        R = R if R > 0 else 1.0
        half_min = min(math.atan(tan_x), math.atan(tan_y))
        dist = 1.05 * R / math.sin(half_min)
        # the frame about `up`: e1, e2 are the two other coordinate axes, e1 x e2 = up
        k = int(np.argmax(np.abs(upv)))
        s = float(upv[k])
        e1, e2 = np.zeros(3), np.zeros(3)
        e1[(k + 1) % 3], e2[(k + 2) % 3] = 1.0, s
        a, e = math.radians(az), math.radians(el)
        direction = math.cos(e) * (math.cos(a) * e1 + math.sin(a) * e2) + math.sin(e) * upv
        eye = target + dist * direction
    return Camera(w, h, look_at(eye, target, upv), eye, fx, fy, cx, cy, tan_x, tan_y, 0.01 * dist)


class RenderPlan:
    """What plan_render decides: the camera, the byte offsets of the geometry fields, the colour source -- ``dc`` (f_dc_0..2)
    with ``degree`` and ``rest`` (the f_rest offsets, ``m`` per channel), or ``rgb`` (the three colour bytes) --, the background
    as three float32 and ``max_work_bytes``."""

    def __init__(self):
        self.dtype = None
        self.camera = None
        self.xyz = self.scales = self.dc = self.rgb = (-1, -1, -1)
        self.rots = (-1, -1, -1, -1)
        self.opacity = -1
        self.rest = ()
        self.m = 0
        self.degree = 0
        self.background = (0.0, 0.0, 0.0)
        self.max_work_bytes = DEFAULT_MAX_WORK_BYTES


def plan_render(dtype, camera, sh_degree=None, background=(0, 0, 0), max_work_bytes=DEFAULT_MAX_WORK_BYTES, colour=True) -> RenderPlan:
    """The rendering of a table of `dtype` through `camera` (a Camera).  sh_degree caps the SH degree the table carries (45 / 24
    / 9 / 0 f_rest fields: 3 / 2 / 1 / 0; channel c, coefficient k is f_rest_(c m + k) as in transform.plan_transform);
    background: three numbers in 0 ... 1.  Every refusal is raised here, before any device work: ValueError for a missing
    geometry field, no colour source (f_dc_0..2, or red green blue as u1), f_rest fields that are no whole bands of three
    channels, rows above 512 bytes, an image side outside 1 ... 8192, a camera whose numbers are not finite or whose near is
    not above 0; TypeError, naming the field, for a field the kernels read as float32 that is not '<f4' (no silent casts).
    colour=False: a plan of the geometry alone, for the view scores (views.plan_scores) -- no colour field is asked for or
    read, ``dc`` and ``rgb`` stay (-1, -1, -1)."""
    dtype = np.dtype(dtype)
    fields = dtype.fields or {}
    p = RenderPlan()
    p.dtype = dtype
    for nm in GEOMETRY:
        if nm not in fields:
            raise ValueError(f"render: the table has no field {nm!r}; x y z, scale_0..2, rot_0..3 and opacity are needed")
    has_dc = bool(colour) and all(nm in fields for nm in DC)
    has_rgb = bool(colour) and all(nm in fields and fields[nm][0] == np.dtype("u1") for nm in RGB)
    if colour and not has_dc and not has_rgb:
        raise ValueError("render: the table has no colour source: f_dc_0..2, or red green blue as unsigned bytes, are needed")
    if not 1 <= dtype.itemsize <= MAX_ROW_BYTES:
        raise ValueError(f"render: rows of {dtype.itemsize} bytes (1 ... {MAX_ROW_BYTES} are supported)")
    if not isinstance(camera, Camera):
        raise ValueError("render: a render.Camera is needed (plan_camera makes one)")
    check_size((camera.width, camera.height))
    numbers = [camera.fx, camera.fy, camera.cx, camera.cy, camera.tan_fovx, camera.tan_fovy, camera.near, *camera.view.ravel(), *camera.eye]
    if not all(math.isfinite(v) for v in numbers) or not camera.near > 0 or not (camera.tan_fovx > 0 and camera.tan_fovy > 0):
        raise ValueError("render: the camera's numbers must be finite, near and the field of view above 0")
    rest_ids, degree = [], 0
    if has_dc:
        rest_ids = sorted(int(m.group(1)) for m in (re.fullmatch(r"f_rest_(\d+)", nm) for nm in dtype.names) if m)
        n_rest = len(rest_ids)
        if rest_ids != list(range(n_rest)) or n_rest % 3 or n_rest // 3 not in (0, 3, 8, 15):
            raise ValueError(f"render: {n_rest} f_rest fields are no whole bands of three colour channels (0, 9, 24 or 45 fields "
                             f"named f_rest_0 ... are needed)")
        p.m = n_rest // 3
        degree = {0: 0, 3: 1, 8: 2, 15: 3}[p.m]
    if sh_degree is not None:
        if isinstance(sh_degree, bool) or int(sh_degree) != sh_degree or not 0 <= int(sh_degree) <= 3:
            raise ValueError(f"render: sh_degree must be 0, 1, 2 or 3, got {sh_degree!r}")
        degree = min(degree, int(sh_degree))
    p.degree = degree
    used = (degree + 1) ** 2 - 1
    read = list(GEOMETRY) + (list(DC) + [f"f_rest_{c * p.m + k}" for c in range(3) for k in range(used)] if has_dc else [])
    for nm in read:
        if fields[nm][0] != np.dtype("<f4"):
            raise TypeError(f"render: field {nm!r} is {fields[nm][0].str}, and the renderer reads '<f4' fields only "
                            f"(no silent casts) -- cast the table to float32 first if that is what is wanted")
    try:
        bg = tuple(float(np.float32(v)) for v in background)
    except (TypeError, ValueError):
        bg = ()
    if len(bg) != 3 or not all(0.0 <= v <= 1.0 for v in bg):
        raise ValueError(f"render: the background must be three numbers in 0 ... 1, got {background!r}")
    if isinstance(max_work_bytes, bool) or int(max_work_bytes) != max_work_bytes or int(max_work_bytes) < 0:
        raise ValueError(f"render: max_work_bytes must be a whole number of bytes, got {max_work_bytes!r}")
    off = lambda names: tuple(int(fields[nm][1]) for nm in names)
    p.camera = camera
    p.xyz, p.scales, p.rots, p.opacity = off(XYZ), off(SCALES), off(ROTS), int(fields["opacity"][1])
    if has_dc:
        p.dc = off(DC)
        p.rest = tuple(int(fields[f"f_rest_{i}"][1]) for i in range(3 * p.m))
    elif has_rgb:
        p.rgb = off(RGB)
    p.background, p.max_work_bytes = bg, int(max_work_bytes)
    return p


def _chunk(tag: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xffffffff)


def write_png(path, image, level: int = 6):
    """the (h, w, 3) uint8 `image` as an 8-bit RGB PNG at `path`: one IDAT chunk, filter type 0 on every scanline"""
    img = np.ascontiguousarray(image)
    if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("write_png: an (h, w, 3) uint8 image with at least one pixel")
    h, w = img.shape[:2]
    lines = np.zeros((h, 1 + 3 * w), np.uint8)
    lines[:, 1:] = img.reshape(h, 3 * w)
    data = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
            + _chunk(b"IDAT", zlib.compress(lines.tobytes(), level)) + _chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(data)
