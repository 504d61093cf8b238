"""The view scores' host side (numpy and math only; no device): ``plan_views`` places the cameras a scene is scored from,
``plan_scores`` is the geometry-only rendering plan of one of them, and the ``check_*`` functions raise every refusal of the
options before any device work -- the role decimate.py has for the decimation and render.py for the preview.

A view score says what a splat contributed to the pixels of a set of rendered views (the definition is
tests/view_scores_numpy.py): ``peak``, the largest blending weight alpha * T the splat had in any pixel of any view, and
``total``, the sum of its weights over all pixels and views in 24-bit fixed point.  A splat no view ever blends -- hidden
behind others, outside every image, or with non-finite geometry -- has peak = total = 0.

The ring of views, for k = 0 .. V - 1 (float64): azimuth_k = (k * 137.50776405003785) mod 360 degrees, the golden angle, and
elevation_k = asin(sin(lo) + (k + 0.5) / V * (sin(hi) - sin(lo))), equal-area bands between the two elevations; each pair goes
to render.plan_camera, whose framing, near and box handling are the preview's.  Explicit cameras (eye, then target) replace the
ring: the answer for inside-out captures, where outside views only see the backs of the walls.
"""
from __future__ import annotations

import math

from . import render as _render

GOLDEN_ANGLE = 137.50776405003785
MAX_VIEWS = 1024
DEFAULT_VIEWS = 32
DEFAULT_SIZE = (512, 512)
DEFAULT_ELEVATION = (-10.0, 70.0)
RANKINGS = ("size", "views")
SCORE_BIT = 24                  # total counts units of 2^-24


def check_views(views) -> int:
    """-> the number of ring views as an int; ValueError unless it is a whole number in 1 ... 1024"""
    try:
        ok = not isinstance(views, bool) and float(views) == int(views) and 1 <= int(views) <= MAX_VIEWS
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"views: the number of views must be a whole number in 1 ... {MAX_VIEWS}, got {views!r}")
    return int(views)


def check_min_contribution(w) -> float:
    """-> the threshold as a float; ValueError unless 0 < w < 1"""
    try:
        w = float(w)
    except (TypeError, ValueError):
        raise ValueError(f"views: min_contribution must be a number in (0, 1), got {w!r}") from None
    if not 0.0 < w < 1.0:
        raise ValueError(f"views: min_contribution must be a number in (0, 1), got {w!r}")
    return w


def check_elevation(elevation) -> tuple:
    """-> (lo, hi) in degrees as floats; ValueError unless -90 <= lo <= hi <= 90"""
    try:
        lo, hi = (float(v) for v in elevation)
        ok = -90.0 <= lo <= hi <= 90.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"views: the elevations must be two numbers of degrees with -90 <= lo <= hi <= 90, got {elevation!r}")
    return lo, hi


def check_rank_by(rank_by) -> str:
    if rank_by not in RANKINGS:
        raise ValueError(f"limit_splats: rank_by must be one of {' '.join(RANKINGS)}, got {rank_by!r}")
    return rank_by


def check_cameras(cameras) -> list:
    """-> the explicit cameras as a list of six-float tuples; ValueError unless there are 1 ... 1024 of them (their numbers are
    checked by render.plan_camera)"""
    try:
        cams = [tuple(c) for c in cameras]
    except TypeError:
        cams = []
    if not 1 <= len(cams) <= MAX_VIEWS:
        raise ValueError(f"views: cameras must be a list of 1 ... {MAX_VIEWS} cameras (ex, ey, ez, tx, ty, tz), got {cameras!r}")
    return cams


def ring_angles(views=DEFAULT_VIEWS, elevation=DEFAULT_ELEVATION) -> list:
    """-> [(azimuth_k, elevation_k)] in degrees, k = 0 .. views - 1 (the module docstring's formulas)"""
    V = check_views(views)
    lo, hi = check_elevation(elevation)
    s_lo, s_hi = math.sin(math.radians(lo)), math.sin(math.radians(hi))
    out = []
    for k in range(V):
        s = s_lo + (k + 0.5) / V * (s_hi - s_lo)
        out.append(((k * GOLDEN_ANGLE) % 360.0, math.degrees(math.asin(max(-1.0, min(1.0, s))))))
    return out


def plan_views(lo, hi, views=DEFAULT_VIEWS, size=DEFAULT_SIZE, elevation=DEFAULT_ELEVATION, up="-y", fov=50, cameras=None) -> list:
    """-> the render.Camera of every view of the box lo ... hi: the ring of `views` cameras, or one per explicit camera
    (ex, ey, ez, tx, ty, tz) of `cameras`, which replace the ring.  Every refusal -- the view count, the elevations, and
    render.plan_camera's for the size, the field of view, the up axis and a camera's numbers -- is a ValueError, and none depends
    on the box."""
    if cameras is not None:
        return [_render.plan_camera(lo, hi, size, up=up, fov=fov, camera=c) for c in check_cameras(cameras)]
    return [_render.plan_camera(lo, hi, size, view=angles, up=up, fov=fov) for angles in ring_angles(views, elevation)]


def plan_scores(dtype, camera, max_work_bytes=_render.DEFAULT_MAX_WORK_BYTES):
    """-> the RenderPlan one view is scored with: render.plan_render of the geometry alone (sh_degree 0, no colour source asked
    for: the colour plays no part in the scores, and a table without one is scored all the same), with its refusals"""
    return _render.plan_render(dtype, camera, sh_degree=0, max_work_bytes=max_work_bytes, colour=False)


def check_options(dtype, views=DEFAULT_VIEWS, size=DEFAULT_SIZE, elevation=DEFAULT_ELEVATION, up="-y", fov=50, cameras=None,
                  max_work_bytes=_render.DEFAULT_MAX_WORK_BYTES):
    """every refusal of a scoring pass over a table of `dtype`, raised from the options alone: the cameras are placed on an
    empty box (no refusal depends on the real one; every explicit camera's numbers are checked), the plan is the first one's"""
    cams = plan_views((0, 0, 0), (0, 0, 0), views, size, elevation, up, fov, cameras)
    plan_scores(dtype, cams[0], max_work_bytes)


def describe(views, size, cameras) -> str:
    """the head of the status lines: '32 views, 512 x 512'"""
    n = len(cameras) if cameras is not None else int(views)
    return f"{n} view{'s' if n != 1 else ''}, {int(size[0])} x {int(size[1])}"
