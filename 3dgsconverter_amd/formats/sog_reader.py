"""``read_sog`` -- the reference's ``SogFormat.read`` (formats/sog.py:23-247) with its per-row decode on the MI355X.

  | step (formats/sog.py)                             | here                                                                |
  |---------------------------------------------------|---------------------------------------------------------------------|
  | :29-37 `is_zipfile`, `meta.json`, `count`         | the same calls, the same exceptions                                 |
  | :60-232 every `meta[...]` access                  | the same accesses in the same order (`parse_meta`): a missing key is |
  |                                                   | the reference's KeyError; a value of another type than the writer's  |
  |                                                   | makes the file one the device path does not take                     |
  | :43-57 `zf.open`, `Image.open`, `convert('RGBA')`,| the same calls per texture on a small thread pool, the texels copied |
  | `np.array`, "Image ... too small"                 | into one page-locked staging buffer; the first error BY TEXTURE      |
  |                                                   | ORDER is raised                                                      |
  | :78-86, :108, :156-158 the float64 position maths,| tables of numpy's own results built on the host (`_lib.sog_read_     |
  | the rotation bytes, the opacity logit             | tables`): the device takes no exp and no log                         |
  | :100-102, :151-153, :208 the codebook gathers     | bytes index a codebook of 256 entries safely; a shorter one is       |
  |                                                   | checked on the host by the reference's own statements in its order   |
  | :190-202 the palette's Python double loop         | none: the kernel reads centroid pixel (label, j) itself             |
  | :221 `palette_flat[labels]`                       | the kernel flags a label >= the palette's size; that statement then  |
  |                                                   | runs on the host texels and raises numpy's own IndexError            |
  | :67-245 the vectorised decode, field by field     | gsx_sog_unpack_dev (csrc/sog_read.hip): one launch, whole rows       |

The rows are the reference's bit for bit ("SOG reader") -- including its reading of a palette above 64 entries, whose
centroid image it indexes by rows of 64 entries where its writer laid the pixels down linearly.  Every error comes before
anything is uploaded, except the label check.  A file with ONE defect raises what the reference raises; which of several
defects shows first is not promised.  Files the device path does not take (``UnsupportedSogError``) go to the reference's own
read when there is one.
"""
from __future__ import annotations

import json
import time
import zipfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .. import _lib
from ..utils import debug_print
from .ksplat_reader import define_dtype

try:
    from PIL import Image
except ImportError:                              # (sog.py:14-20)
    Image = None

NOT_A_ZIP = "SOG Format: Only ZIP-bundled .sog files are supported."                # sog.py:30
MAX_DECODE_THREADS = 8         # seven textures at most; never sized from the machine's CPU count
TEXTURES = _lib.SOG_READ_TEXTURES


class UnsupportedSogError(ValueError):
    """a .sog file the device path does not take, with no reference reader to hand it to"""


class _Unsupported(Exception):
    pass


def _number(v) -> bool:
    return type(v) is float or (type(v) is int and abs(v) < (1 << 53))


def _want(ok: bool, what: str):
    if not ok:
        raise _Unsupported(what)


def _files(section, k: int, what: str):
    files = section["files"]
    _want(isinstance(files, list) and len(files) > k and isinstance(files[k], str), what + ".files")
    return files[k]


def _codebook(section, what: str):
    cb = section["codebook"]
    _want(isinstance(cb, list) and all(_number(v) for v in cb), what + ".codebook")
    return cb


def parse_meta(meta) -> dict:
    """every access of sog.py:37-232 to `meta`, in its order, so that a missing key raises the reference's KeyError ->
    {count, bands, palette, files: {texture: name}, mins, maxs, scale_cb, sh0_cb, shn_cb}; raises _Unsupported for anything
    the device path does not take"""
    _want(isinstance(meta, dict), "meta")
    count = meta["count"]
    _want(type(count) is int and 0 <= count < (1 << 32), "count")
    files = {}
    _want(isinstance(meta["means"], dict), "means")
    files["means_l"] = _files(meta["means"], 0, "means")
    files["means_u"] = _files(meta["means"], 1, "means")
    mins, maxs = meta["means"]["mins"], meta["means"]["maxs"]
    for v in (mins, maxs):
        _want(isinstance(v, list) and len(v) >= 3 and all(_number(x) for x in v[:3]), "means.mins / maxs")
    _want(isinstance(meta["scales"], dict), "scales")
    files["scales"] = _files(meta["scales"], 0, "scales")
    scale_cb = _codebook(meta["scales"], "scales")
    _want(isinstance(meta["quats"], dict), "quats")
    files["quats"] = _files(meta["quats"], 0, "quats")
    _want(isinstance(meta["sh0"], dict), "sh0")
    files["sh0"] = _files(meta["sh0"], 0, "sh0")
    sh0_cb = _codebook(meta["sh0"], "sh0")
    bands, palette, shn_cb = 0, 0, None
    if "shN" in meta:
        shn = meta["shN"]
        _want(isinstance(shn, dict), "shN")
        bands, palette = shn["bands"], shn["count"]
        _want(type(bands) is int and 1 <= bands <= 3, "shN.bands")
        _want(type(palette) is int and 1 <= palette <= 65536, "shN.count")
        files["shN_centroids"] = _files(shn, 0, "shN")
        shn_cb = _codebook(shn, "shN")
        files["shN_labels"] = _files(shn, 1, "shN")
    return dict(count=count, bands=bands, palette=palette, files=files, mins=mins, maxs=maxs, scale_cb=scale_cb, sh0_cb=sh0_cb, shn_cb=shn_cb)


def texture_order(bands: int):
    """the order in which sog.py reads the textures"""
    return ("means_l", "means_u", "scales", "quats", "sh0") + (("shN_centroids", "shN_labels") if bands else ())


def _decode_texture(zf, filename: str, expected: int):
    """sog.py:43-57 (read_webp_to_flat) -> the image's RGBA bytes, flat, at least 4 * expected of them"""
    with zf.open(filename) as f:
        img = Image.open(f)
        width, height = img.size
        if img.mode != "RGBA":
            img = img.convert("RGBA")
        data = np.asarray(img).reshape(-1)
        pixel_count = width * height
        if pixel_count < expected:
            raise ValueError(f"Image {filename} too small: {pixel_count} < {expected}")
        return data


def centroid_indices(pixels: np.ndarray, palette: int, coeffs: int) -> np.ndarray:
    """:183-202 from the staged centroid pixels (pixel (i, j) is number i * coeffs + j there) -> uint8[palette, 3, coeffs]"""
    return np.ascontiguousarray(pixels.reshape(-1, coeffs, 4)[:palette, :, :3].transpose(0, 2, 1))


def _installed_original():
    """the reference's own ``SogFormat.read`` when install() has saved one -> a function path -> rows, or None"""
    from ..install import _saved
    original = _saved.get(("sogformat", "read"))
    if original is None:
        return None

    def fallback(path):
        import gsconverter.formats.sog as mod  # type: ignore
        return original(mod.SogFormat(), path)
    return fallback


def read_sog(path: str, stage_ms: "dict | None" = None, device: int = 0, *, fallback=None, profile: "dict | None" = None, keep: "dict | None" = None) -> np.ndarray:
    """:23-247 -> the reference's structured array: define_dtype(has_scal=False, has_rgb=False) of the file's bands, float32
    fields, packed; nx ny nz zero.

    fallback: a function path -> rows for the files the device path does not take (bands outside 1 ... 3, a palette outside
    1 ... 65 536, a count that is no non-negative int, anything in meta.json of another type than the writer's); by default the
    reference's own read when install() has saved one, else such files raise UnsupportedSogError.  stage_ms: a dict that
    receives the stage clocks parse, decode, upload, kernel, download (tools/probe_sog_read.py).  profile: a dict that receives the returned table's profile
    (_lib.TableProfile.as_dict) from one more pass over the decoded rows before their download (stage clock "profile").  keep: a dict that receives the decoded rows in HBM as keep["rows"] (_lib.ResidentRows; the caller
    closes it) when the returned table's rows are resident; it stays empty otherwise."""
    return _lib.with_keep(keep, lambda: _lib.with_profile(profile, lambda: _read(path, stage_ms, device, fallback, profile, keep)))


def _read(path, stage_ms, device, fallback, profile, keep=None):
    debug_print(f"[DEBUG] Reading .sog file from {path}")
    t0 = time.perf_counter()
    if not Image:
        raise ImportError("Pillow is required to read .sog files. Please install it.")
    if not zipfile.is_zipfile(path):
        raise ValueError(NOT_A_ZIP)
    with zipfile.ZipFile(path, "r") as zf:
        with zf.open("meta.json") as f:
            meta = json.load(f)
        try:
            plan = parse_meta(meta)
        except _Unsupported as e:
            fallback = fallback or _installed_original()
            if fallback is None:
                raise UnsupportedSogError("%s: meta.json's %s is not what the device path takes (count a non-negative int, 1 ... 3 bands, "
                                          "a palette of 1 ... 65536, the writer's types) -- the GPU SOG reader does not take this file and "
                                          "there is no reference reader to hand it to" % (path, e)) from None
            debug_print(f"[DEBUG] SOG: meta.json's {e}; the reference's reader takes it")
            zf.close()
            return fallback(path)
        n, bands, palette = plan["count"], plan["bands"], plan["palette"]
        cpb = _lib.SOG_COEFFS_PER_BAND[bands]
        coeffs = cpb // 3
        image_rows = (palette + 63) // 64                                             # :175 int(np.ceil(palette_size / 64))
        dtype = define_dtype(bands)
        tables = _lib.sog_read_tables(plan["mins"], plan["maxs"], plan["scale_cb"], plan["sh0_cb"], plan["shn_cb"])
        order = texture_order(bands)
        if stage_ms is not None:
            stage_ms["parse"] = round((time.perf_counter() - t0) * 1e3, 3)

        def texels(host, place, name):
            off, nb = place[name]
            return host[off:off + nb].reshape(-1, 4)

        def decode_into(host, place, name):
            off, nb = place[name]
            if name == "shN_centroids":                                               # only the columns :193 reaches
                data = _decode_texture(zf, plan["files"][name], 64 * cpb * image_rows)
                host[off:off + nb].reshape(image_rows, 64 * coeffs, 4)[:] = \
                    data[:4 * 64 * cpb * image_rows].reshape(image_rows, 64 * cpb, 4)[:, :64 * coeffs]
            else:
                host[off:off + nb] = _decode_texture(zf, plan["files"][name], n)[:nb]

        def fill(host, place):
            with ThreadPoolExecutor(max_workers=min(MAX_DECODE_THREADS, len(order))) as pool:
                jobs = [pool.submit(decode_into, host, place, name) for name in order]
            for job in jobs:                         # the first error by texture order, not by completion time
                if job.exception() is not None:
                    raise job.exception()
            # a codebook shorter than the bytes that index it: the reference's own gathers, in its order (:100-102, :151-153, :208)
            for cb, name in ((tables["scale_cb"], "scales"), (tables["sh0_cb"], "sh0")):
                if len(cb) < 256:
                    idx = texels(host, place, name)
                    cb[idx[:, 0]], cb[idx[:, 1]], cb[idx[:, 2]]
            if bands and len(tables["shn_cb"]) < 256:
                tables["shn_cb"][centroid_indices(texels(host, place, "shN_centroids"), palette, coeffs)]

        def on_flag(host, place):                    # :208-221 on the host texels: numpy's own IndexError
            palette_flat = tables["shn_cb"][centroid_indices(texels(host, place, "shN_centroids"), palette, coeffs)].reshape(palette, -1)
            labels_raw = texels(host, place, "shN_labels")
            labels = labels_raw[:, 0].astype(np.uint16) | (labels_raw[:, 1].astype(np.uint16) << 8)
            palette_flat[labels]

        if n == 0:                                   # every read and its errors, no device
            place, total = _lib.sog_texel_layout(0, bands, palette)
            fill(np.empty(total, np.uint8), place)
            return np.zeros(0, dtype)
        rows = _lib.sog_unpack_table(fill, n, bands, palette, tables, dtype, on_flag=on_flag, stage_ms=stage_ms, device=device, **_lib.profile_kw(profile), **_lib.keep_kw(keep))
    debug_print(f"[DEBUG] SOG read completed. {n} splats, {bands} SH bands.")
    return rows


def bind_read(original):
    """-> a replacement for ``SogFormat.read`` that decodes on the device; a file the device path does not take goes to
    `original` (the reference's read)"""
    def read(self, path, **kwargs):
        return read_sog(path, fallback=lambda p: original(self, p, **kwargs))
    read.__wrapped__ = original
    return read
