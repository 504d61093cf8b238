"""``--fidelity``: what a conversion cost in image space (the definition of the sums is tests/fidelity_numpy.py).

Two tables -- a reference and a test -- are rendered through the same ring of cameras (views.plan_views, framed on the
reference's bounds), each with the full SH degree it carries, over a mid-grey background, and every pair of images is compared
where the rasteriser left it (csrc/fidelity.hip: gsx_image_compare_dev).  Per pair the device returns nine integers: the squared
error per channel, the number of 8 x 8 windows and the per-channel sums of a 32.32 fixed-point box-window SSIM.  Every figure a
user sees derives from those integers on the host, in float64:

    psnr = 10 log10(255^2 * 3 h w / sum(sse))       inf when the images are identical
    ssim = sum(ssim_fixed) / (3 * windows * 2^32)   None when the image has no window (a side below 8)

and pooled figures over several views use the summed integers, never means of per-view decibels.  The integers are the same
bits on every run, so the report is too.

``check_options`` raises every refusal of the options before any device work; ``summarise`` is host only; ``compare_rows`` and
``compare_tables`` are the device work.
"""
from __future__ import annotations

import math

import numpy as np

from . import render as _render
from . import views as _views

TILE = 32                       # GSX_FIDELITY_TILE: the compare kernel's tile edge (tests/fidelity_cases.py sizes its images by it)
ONE = 1 << 32                   # the fixed point of a window's SSIM
MODES = ("written", "source")
DEFAULT_VIEWS = 8
DEFAULT_SIZE = (512, 512)
BACKGROUND = (0.5, 0.5, 0.5)    # exact in float32; a hole shows against dark and bright scenes alike
MAX_WORK_BYTES = _render.DEFAULT_MAX_WORK_BYTES   # the converter's instance-workspace budget per render (read when it measures)


def check_mode(mode) -> str:
    if mode not in MODES:
        raise ValueError(f"fidelity: the mode must be one of {' '.join(MODES)}, got {mode!r}")
    return mode


def check_options(mode="written", views=None, size=None, elevation=None, up=None, fov=None, cameras=None, merge=None) -> dict:
    """Every refusal of a fidelity measurement, raised from the options alone (ValueError), and the options normalised:
    -> dict(mode, views, size, elevation, up, fov, cameras), None replaced by the defaults.  The mode is 'written' or 'source';
    'source' has no single reference file when further sources are merged; explicit cameras replace the ring, so a view count
    beside them is a contradiction; the view count, the size, the elevations, the up axis, the field of view and every
    camera's numbers are views.plan_views' refusals (the cameras are placed on an empty box: none depends on the real one)."""
    mode = check_mode(mode)
    if mode == "source" and merge:
        raise ValueError("fidelity: 'source' compares against the one input file; a merge of several sources has none (use 'written')")
    if cameras is not None and views is not None:
        raise ValueError("fidelity: explicit cameras replace the ring of views; give fidelity_cameras or fidelity_views, not both")
    opts = {"views": DEFAULT_VIEWS if views is None else views, "size": DEFAULT_SIZE if size is None else size,
            "elevation": _views.DEFAULT_ELEVATION if elevation is None else elevation, "up": "-y" if up is None else up,
            "fov": 50 if fov is None else fov, "cameras": cameras}
    cams = _views.plan_views((0, 0, 0), (0, 0, 0), **opts)
    opts["views"] = len(cams)
    opts["size"] = (cams[0].width, cams[0].height)
    opts["elevation"] = _views.check_elevation(opts["elevation"])
    if cameras is not None:
        opts["cameras"] = _views.check_cameras(cameras)
    return dict(opts, mode=mode)


def psnr_of(sse_total: int, pixels: int) -> float:
    """10 log10(255^2 * (3 * pixels) / sse) from the summed integers; inf for identical images"""
    return math.inf if sse_total == 0 else 10.0 * math.log10(255.0 ** 2 * (3 * pixels) / sse_total)


def ssim_of(fixed_total: int, windows: int):
    """the mean SSIM over windows and channels from the summed integers; None without windows"""
    return None if windows == 0 else fixed_total / (3 * windows * ONE)


def view_figures(words: dict, width: int, height: int) -> dict:
    """the nine integers of one image pair (_lib.image_compare_words) -> the per-view dict: sse, windows, ssim_fixed, width,
    height, psnr, ssim"""
    sse, fixed, windows = tuple(int(v) for v in words["sse"]), tuple(int(v) for v in words["ssim"]), int(words["windows"])
    return {"sse": sse, "windows": windows, "ssim_fixed": fixed, "width": int(width), "height": int(height),
            "psnr": psnr_of(sum(sse), int(width) * int(height)), "ssim": ssim_of(sum(fixed), windows)}


def summarise(per_view) -> dict:
    """The pooled and the worst figures of a list of per-view dicts (view_figures) -> dict(views: the list, sse, ssim_fixed:
    the per-channel sums over the views, windows, psnr, ssim: from those sums, worst_view: the view of the lowest PSNR,
    worst_psnr, worst_ssim_view, worst_ssim: the lowest per-view SSIM (None without windows) -- ties go to the lowest index --,
    size: (width, height) of the first view, report: the figures as the status line shows them)."""
    per_view = list(per_view)
    if not per_view:
        raise ValueError("fidelity: no views to summarise")
    sse = tuple(sum(v["sse"][c] for v in per_view) for c in range(3))
    fixed = tuple(sum(v["ssim_fixed"][c] for v in per_view) for c in range(3))
    windows = sum(v["windows"] for v in per_view)
    pixels = sum(v["width"] * v["height"] for v in per_view)
    worst = min(range(len(per_view)), key=lambda k: (per_view[k]["psnr"], k))
    with_ssim = [k for k in range(len(per_view)) if per_view[k]["ssim"] is not None]
    worst_s = min(with_ssim, key=lambda k: (per_view[k]["ssim"], k)) if with_ssim else None
    out = {"views": per_view, "sse": sse, "ssim_fixed": fixed, "windows": windows, "psnr": psnr_of(sum(sse), pixels),
           "ssim": ssim_of(sum(fixed), windows), "worst_view": worst, "worst_psnr": per_view[worst]["psnr"],
           "worst_ssim_view": worst_s, "worst_ssim": None if worst_s is None else per_view[worst_s]["ssim"],
           "size": (per_view[0]["width"], per_view[0]["height"])}
    n = len(per_view)
    head = f"{n} view{'s' if n != 1 else ''} of {out['size'][0]} x {out['size'][1]}"
    if sum(sse) == 0:
        p = "PSNR inf (identical images)"
    else:
        p = f"PSNR {out['psnr']:.2f} dB (worst {out['worst_psnr']:.2f}, view {worst})"
    s = "SSIM n/a" if out["ssim"] is None else f"SSIM {out['ssim']:.4f} (worst {out['worst_ssim']:.4f}, view {worst_s})"
    out["report"] = f"{head}: {p}, {s}"
    return out


def report_line(result: dict, what: str) -> str:
    """'Fidelity (written table vs out.spz): 8 views of 512 x 512: PSNR 41.23 dB (worst 38.90, view 3), SSIM 0.9871 (...)'"""
    return f"Fidelity ({what}): {result['report']}"


def compare_rows(ref_rows, test_rows, cameras, background=BACKGROUND, max_work_bytes=_render.DEFAULT_MAX_WORK_BYTES, stage_ms=None,
                 ctx=None) -> dict:
    """Two tables in HBM (_lib.ResidentRows, possibly of different dtypes) through the same `cameras` (render.Camera) ->
    summarise() of the per-view figures, each with ``visible_ref`` and ``visible_test``.  Per camera: one render.plan_render
    per table (the full SH degree it carries), ResidentRows.render_dev of each, one gsx_image_compare_dev on the two images
    where they lie, both freed.  Everything runs on `ctx` (the reference rows' own context without one).  Every refusal of
    plan_render is raised before any device work; render.RenderRefused from either render propagates, with nothing left in
    HBM.  stage_ms: the six RENDER_STAGES clocks summed over both tables and all views, and "compare"."""
    from . import _lib
    cameras = list(cameras)
    plans = [(_render.plan_render(ref_rows.dtype, cam, background=background, max_work_bytes=max_work_bytes),
              _render.plan_render(test_rows.dtype, cam, background=background, max_work_bytes=max_work_bytes)) for cam in cameras]
    if not plans:
        raise ValueError("fidelity: no cameras")
    ctx = ctx if ctx is not None else ref_rows._ctx
    per_view = []
    for (plan_a, plan_b), cam in zip(plans, cameras):
        image_a = image_b = None
        try:
            image_a = ref_rows.render_dev(plan_a, ctx=ctx, stage_ms=stage_ms)
            visible_a = ref_rows.render_info["visible"]
            image_b = test_rows.render_dev(plan_b, ctx=ctx, stage_ms=stage_ms)
            visible_b = test_rows.render_info["visible"]
            assert image_a.nbytes == image_b.nbytes == cam.width * cam.height * 3, "shared cameras: two images of one size"
            words = _lib.image_compare_dev(ctx, image_a.ptr, image_b.ptr, cam.width, cam.height, stage_ms=stage_ms)
        finally:
            for buf in (image_b, image_a):
                if buf is not None:
                    buf.free()
        per_view.append(dict(view_figures(words, cam.width, cam.height), visible_ref=visible_a, visible_test=visible_b))
    return summarise(per_view)


def compare_tables(ref, test, views=DEFAULT_VIEWS, size=DEFAULT_SIZE, elevation=_views.DEFAULT_ELEVATION, up="-y", fov=50, cameras=None,
                   lo=None, hi=None, background=BACKGROUND, max_work_bytes=_render.DEFAULT_MAX_WORK_BYTES, stage_ms=None) -> dict:
    """compare_rows of two tables of which each is a host table (1-D structured: uploaded once, freed on every exit path) or
    _lib.ResidentRows (left open), through views.plan_views of the reference's bounding box -- its rows' profile in HBM, else the
    host table's -- or of the box `lo` ... `hi`.  Every refusal of the options and of render.plan_render for either dtype comes
    before any device work.  The result also carries ``cameras``, the list that was used."""
    from . import _lib
    opts = dict(views=views, size=size, elevation=elevation, up=up, fov=fov, cameras=cameras)
    dtypes = [t.dtype for t in (ref, test)]
    probe = _views.plan_views((0, 0, 0), (0, 0, 0), **opts)[0]
    for dt in dtypes:
        _render.plan_render(dt, probe, background=background, max_work_bytes=max_work_bytes)
    temps = []
    try:
        rows = []
        for t in (ref, test):
            if isinstance(t, _lib.ResidentRows):
                rows.append(t)
            else:
                with _lib.stage_clock(stage_ms, "upload"):
                    temps.append(_lib.ResidentRows.from_host(t))
                rows.append(temps[-1])
        if lo is None or hi is None:
            prof = rows[0].profile() if isinstance(ref, _lib.ResidentRows) else _lib.host_table_profile(np.ascontiguousarray(ref))
            lo, hi = prof["lo"], prof["hi"]
        cams = _views.plan_views(lo, hi, **opts)
        out = compare_rows(rows[0], rows[1], cams, background=background, max_work_bytes=max_work_bytes, stage_ms=stage_ms)
        out["cameras"] = cams
        return out
    finally:
        for rr in temps:
            rr.close()


def side_by_side(ref_image: np.ndarray, test_image: np.ndarray) -> np.ndarray:
    """-> (h, 3 w, 3) uint8: the reference, the test and min(255, 4 |A - B|) next to one another"""
    diff = np.abs(ref_image.astype(np.int16) - test_image.astype(np.int16))
    return np.concatenate([ref_image, test_image, np.minimum(255, 4 * diff).astype(np.uint8)], axis=1)
