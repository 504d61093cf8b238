"""The command line: ``python -m 3dgsconverter_amd -i scene.ply -f spz --sor_intensity 5 --force``.

The flags, their types and defaults, the validation messages, the auto-output, no-op, auto-extension and overwrite rules and the
lines of the info block are the reference's (gsconverter/main.py:56-506); the work behind them is this package's.  ``--info``
and the two info blocks of a conversion decode each file once: the bounds and the SH activity come from the profile the reader
took of its rows in HBM (csrc/table_profile.hip), the PLY property names from the header (formats/ply_reader.parse_header) and
the compressed-PLY chunk count from the reader's metadata.  In conversion mode the source info block and ``Converter.run``
share one load.  ``--merge FILE`` (repeatable, with ``--merge_rotate / --merge_scale / --merge_translate`` once per file) adds
further scenes to the input: ``Converter.run(merge=...)``.  ``--preview FILE`` (with ``--preview_size / _view / _up / _camera /
_fov``) renders the table that was written to a PNG on the GPU: ``Converter.run(preview=...)``; it counts as an action in the
no-op check, and the other preview flags are refused without it.  ``--min_contribution W`` and ``--rank_by views`` (with ``--views /
--views_size / _elevation / _up`` or ``--view_camera``) score the splats by what they contribute to rendered views:
``Converter.run(min_contribution=, rank_by=)``; both count as actions, and the other view flags are refused without one of them.
``--fidelity [written|source]`` (with ``--fidelity_views / _size / _up / _image`` or ``--fidelity_camera``) reads the output file
back and reports its PSNR and SSIM over a ring of rendered views against the table that was written (the format's loss) or
against the moved source (everything the run did): ``Converter.run(fidelity=...)``; it counts as an action, and the other fidelity
flags are refused without it.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from . import utils
from .converter import EXTENSIONS, VALID_FORMATS, Converter, degree_of_count

__version__ = "0.1"
RULE = "-" * 60


class AboutAction(argparse.Action):
    def __call__(self, parser, namespace, values, option_string=None):
        print(f"3dgsconverter_amd v{__version__}: 3D Gaussian Splatting conversion on AMD Instinct MI355X (HIP, gfx950)")
        print("Command line, formats and messages after 3dgsconverter (https://github.com/francescofugazzi/3dgsconverter, MIT).")
        parser.exit()


def check_source_extras(path) -> bool:
    """main.py:26-54: does a .ply header declare an element other than vertex and face?  The header's lines only."""
    try:
        if path.lower().endswith(".ply"):
            header = b""
            with open(path, "rb") as f:
                while True:
                    line = f.readline()
                    header += line
                    if b"end_header" in line or not line:
                        break
            for line in header.decode("utf-8", errors="ignore").split("\n"):
                if line.startswith("element"):
                    parts = line.split()
                    if len(parts) >= 2 and parts[1] not in ["vertex", "face"]:
                        return True
    except Exception:   # noqa: BLE001  (:52 any error means no extras)
        pass
    return False


def bounds_lines(data, profile) -> list:
    """main.py:109-114.  The extremes are the profile's; a zero extreme is numpy's own on the strided view (which zero a
    reduction returns depends on the layout it walks: processing.DataProcessor.apply_auto_bbox), an axis that holds a NaN
    prints nan, and a table without rows or without a profile takes the reference's expressions as they are."""
    if profile is None or len(data) == 0 or profile.get("n") != len(data):
        lo = [data[a].min() for a in ("x", "y", "z")]
        hi = [data[a].max() for a in ("x", "y", "z")]
    else:
        lo, hi = list(profile["lo"]), list(profile["hi"])
        for a, nm in enumerate(("x", "y", "z")):
            if lo[a] == 0:
                lo[a] = data[nm].min()
            if hi[a] == 0:
                hi[a] = data[nm].max()
    return [f"Bounds Min: [{lo[0]:.4f}, {lo[1]:.4f}, {lo[2]:.4f}]", f"Bounds Max: [{hi[0]:.4f}, {hi[1]:.4f}, {hi[2]:.4f}]"]


def band_active(data, profile, lo: int, hi: int) -> bool:
    """main.py:182-209: is any of f_rest_lo .. f_rest_(hi-1) active?  From the profile's word; a `scalar_`-named column, which no
    reader of this package returns, from numpy"""
    names = data.dtype.names
    for i in range(lo, hi):
        name = f"f_rest_{i}"
        if name in names:
            if (profile["rest_nonzero"] >> i) & 1 if profile is not None else np.any(data[name]):
                return True
        elif f"scalar_{name}" in names and np.any(data[f"scalar_{name}"]):
            return True
    return False


def ply_sh_messages(input_path, data, profile):
    """main.py:136-218 for a .ply path -> (header_msg, active_msg, raw_fields or None), from the file's header"""
    from .formats.ply_reader import parse_header
    h = parse_header(input_path)
    header_msg = active_msg = "None"
    raw_fields = None
    if h.element("chunk") is not None:
        sh = h.element("sh")
        if sh is not None:
            n_sh = len(sh.props)
            deg = degree_of_count(n_sh)
            return f"Degree {deg} ({n_sh} coeffs)", f"Degree {deg}", None
        return "Degree 0 (DC)", "Degree 0", None
    vertex = h.element("vertex")
    if vertex is not None:
        raw_fields = tuple(vertex.names())
        sh_cols = [p for p in raw_fields if p.startswith("f_rest_") or p.startswith("scalar_f_rest_")]
        if not sh_cols:
            if any(p.startswith("f_dc_") for p in raw_fields):
                header_msg, active_msg = "Degree 0 (DC)", "Degree 0"
        else:
            max_degree = degree_of_count(len(sh_cols))
            header_msg = f"Degree {max_degree} ({len(sh_cols)} coeffs)"
            eff = 0
            if max_degree >= 1 and band_active(data, profile, 0, 9):
                eff = 1
            if max_degree >= 2 and band_active(data, profile, 9, 24):
                eff = 2
            if max_degree >= 3 and band_active(data, profile, 24, 45):
                eff = 3
            active_msg = f"Degree {eff}" + (" (Cropped/Zeroed)" if eff < max_degree else "")
    return header_msg, active_msg, raw_fields


def info_lines(input_path, converter_obj) -> list:
    """the lines main.py:74-250 print for a loaded source"""
    out = []
    data, handler, fmt = converter_obj.data, converter_obj.source_handler, converter_obj.source_format
    profile = getattr(converter_obj, "profile", None)
    if fmt == "ksplat":
        meta = getattr(handler, "metadata", {})
        if meta:
            out.append(f"KSplat Version: {meta.get('v_major')}.{meta.get('v_minor')}")
            out.append(f"Compression Level: {meta.get('compression_level')}")
            if meta.get("compression_level", 0) >= 1 and meta.get("sections"):
                s0 = meta["sections"][0]
                out.append(f"Bucket Size: {s0.get('bucketSize')}")
                out.append(f"Block Size: {s0.get('bucketBlockSize')}")
            if "min_sh" in meta:
                out.append(f"SH Range: [{meta['min_sh']:.2f}, {meta['max_sh']:.2f}]")
    if fmt == "compressed_ply":
        from .formats.ply_reader import parse_header
        out.append("Quantization: Chunk-based (256 splats/chunk)")
        out.append(f"Chunks: {handler.metadata['chunks']:,}")
        out.append("Position/Scale Packing: 11-10-11 bit")
        out.append("Rotation Packing: 2-10-10-10 bit")
        out.append("Color Packing: 8-8-8-8 bit")
        if parse_header(os.path.abspath(input_path)).element("sh") is not None:
            out.append("SH Quantization: 8-bit ([-4, 4] range)")
    extras = [el.name for el in getattr(handler, "extra_elements", None) or []]
    if extras:
        out.append(f"Extra Elements: {', '.join(extras)}")
    out.append(f"Format Detected: {fmt.upper()}")
    out.append(f"Points: {len(data):,}")
    fields = data.dtype.names
    if "x" in fields:
        out.extend(bounds_lines(data, profile))
    attrs = [label for label, f in (("RGB", "red"), ("Opacity", "opacity"), ("Scale", "scale_0"), ("Rotation", "rot_0")) if f in fields]
    out.append(f"Attributes: {', '.join(attrs)}")
    raw_fields, header_msg, active_msg = fields, "None", "None"
    if input_path.lower().endswith(".ply"):
        try:
            header_msg, active_msg, raw = ply_sh_messages(input_path, data, profile)
            raw_fields = raw if raw is not None else raw_fields
        except Exception as e:   # noqa: BLE001  (:220)
            out.append(f"Warning: Could not parse PLY header for SH analysis: {e}")
    if header_msg == "None" and active_msg == "None":                                           # :226-247
        sh_cols_raw = [f for f in raw_fields if "f_rest_" in f]
        dc_cols_raw = [f for f in raw_fields if "f_dc_" in f]
        if dc_cols_raw:
            header_msg, active_msg = "DC (Degree 0)", "DC"
        if sh_cols_raw:
            max_degree_raw = degree_of_count(len(sh_cols_raw))
            if max_degree_raw > 0:
                header_msg = f"Degree {max_degree_raw} ({len(sh_cols_raw)} coeffs)"
            elif dc_cols_raw:
                header_msg = "Degree 0 (DC only)"
            active_msg = header_msg
    out.append(f"SH Headers: {header_msg}")
    out.append(f"SH Content: {active_msg}")
    return out


def report_info(input_path, converter_obj=None):
    """main.py:56-254.  converter_obj: a Converter whose source this block describes; one that has not loaded it yet loads it
    here, and a later run() of it uses that load"""
    abs_path = os.path.abspath(input_path)
    print(f"\n{RULE}")
    print(f"File: {abs_path}")
    try:
        print(f"Size: {os.path.getsize(abs_path) / (1024 * 1024):.2f} MB")
        if converter_obj is None:
            converter_obj = Converter(abs_path, "dummy_out.ply", "3dgs", resident=False)   # (the info block reads the profile alone)
        if converter_obj.data is None:
            converter_obj.load_source_only()
        for line in info_lines(input_path, converter_obj):
            print(line)
    except Exception as e:   # noqa: BLE001  (:252)
        print(f"Error reading info for {input_path}: {e}")
    print(f"3D Gaussian Splatting Converter: {__version__}")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="3dgsconverter_amd",
                                description="Convert 3D Gaussian Splatting scenes between 3DGS PLY, CloudCompare PLY, compressed PLY, .ksplat, "
                                            ".splat, .spz, .sog and Parquet, with the readers, filters and writers running on an AMD Instinct MI355X.")
    p.add_argument("--input", "-i", required=True, help="Source file (with --info: a glob pattern).")
    p.add_argument("--output", "-o", help="Destination file; derived from the input's name and the target format when omitted.")
    p.add_argument("--target_format", "-f", help="One of 3dgs, cc, ksplat, splat, spz, sog, parquet, compressed_ply.")
    p.add_argument("--info", "-I", action="store_true", help="Describe the file(s) and stop: format, points, bounds, attributes, SH content.")
    p.add_argument("--debug", "-d", action="store_true", help="Print the debug lines too.")
    p.add_argument("--about", action=AboutAction, nargs=0, help="Say what this program is and stop.")
    p.add_argument("--force", action="store_true", help="Overwrite an existing output file without asking.")
    p.add_argument("--rgb", action="store_true", help="Add red / green / blue computed from the SH DC term when the table has none.")
    p.add_argument("--bbox", nargs=6, type=float, metavar=("minX", "minY", "minZ", "maxX", "maxY", "maxZ"), help="Keep the splats inside this box.")
    p.add_argument("--rotate", nargs=3, type=float, metavar=("RX", "RY", "RZ"),
                   help="Rotate the scene: degrees about the fixed X axis, then Y, then Z. Positions, orientations, normals and SH bands turn with it.")
    p.add_argument("--scale", type=float, metavar="S", help="Scale the scene uniformly by S > 0 (positions and splat sizes).")
    p.add_argument("--translate", nargs=3, type=float, metavar=("X", "Y", "Z"),
                   help="Shift the scene, after rotation and scale. --bbox and the filters work in the transformed frame.")
    p.add_argument("--merge", action="append", metavar="FILE",
                   help="Add another scene (any readable format) to the input; repeatable. The union is written in the common layout: the widest "
                        "SH degree among the files, colours only when every file has them. The global transform and the filters act on the union.")
    p.add_argument("--merge_rotate", action="append", nargs=3, type=float, metavar=("RX", "RY", "RZ"),
                   help="Rotate a --merge file alone before the union; give it once per --merge file, in their order, or not at all.")
    p.add_argument("--merge_scale", action="append", type=float, metavar="S", help="Scale a --merge file alone; once per --merge file, or not at all.")
    p.add_argument("--merge_translate", action="append", nargs=3, type=float, metavar=("X", "Y", "Z"),
                   help="Shift a --merge file alone, after its rotation and scale; once per --merge file, or not at all.")
    p.add_argument("--auto_bbox", action="store_true", help="Report the tight bounding box of what the filters leave.")
    p.add_argument("--extra_elements", action="store_true", help="Carry a PLY's non-vertex elements over (3dgs and cc targets).")
    p.add_argument("--density_voxel_size", type=float, help=argparse.SUPPRESS)
    p.add_argument("--density_threshold", type=float, help=argparse.SUPPRESS)
    p.add_argument("--sor_k", type=float, help=argparse.SUPPRESS)
    p.add_argument("--sor_sigma", type=float, help=argparse.SUPPRESS)
    p.add_argument("--crop_sh", action="store_true", help="Write only the SH coefficients the scene uses instead of 45 padded columns.")
    p.add_argument("--sh_level", type=int, help="Target SH degree 0-3; never above the source's degree or the target format's limit.")
    p.add_argument("--bucket_size", type=int, help=argparse.SUPPRESS)
    p.add_argument("--block_size", type=float, help=argparse.SUPPRESS)
    p.add_argument("--density_sensitivity", type=float, help="Density filter, 0.0-1.0: higher keeps only denser regions.")
    p.add_argument("--sor_intensity", type=float, help="Statistical outlier removal, 1.0-10.0: higher removes more floaters.")
    p.add_argument("--min_opacity", type=int, help="Drop splats whose opacity is below this value (0-255).")
    p.add_argument("--max_splats", type=int, metavar="N",
                   help="Keep at most N splats: the most visible ones by the .splat writer's metric (size times opacity), after every other filter.")
    p.add_argument("--min_contribution", type=float, metavar="W",
                   help="Render the scene from a ring of views and drop every splat whose largest blending weight (alpha times transmittance) "
                        "over all pixels stays under W, between 0 and 1. Every splat that no view ever blends goes: hidden ones, splats outside "
                        "every view, and splats with non-finite geometry. After --decimate_voxel_size, before --max_splats.")
    p.add_argument("--rank_by", choices=("size", "views"),
                   help="What --max_splats keeps: the largest splats by size times opacity (size, the default), or the splats the views see most, "
                        "by summed blending weight (views). With --min_contribution both come from one scoring pass.")
    p.add_argument("--views", type=int, metavar="N", help="Number of scoring views on a ring about the scene's bounding box, 1-1024 (default 32).")
    p.add_argument("--views_size", nargs=2, type=int, metavar=("W", "H"), help="Scoring image size in pixels, 1-8192 per side (default 512 512).")
    p.add_argument("--views_elevation", nargs=2, type=float, metavar=("LO", "HI"),
                   help="Elevation band of the ring in degrees, -90 <= LO <= HI <= 90 (default -10 70).")
    p.add_argument("--views_up", metavar="AXIS", help="Up axis of the ring: +x -x +y -y +z -z (default -y; write --views_up=-y).")
    p.add_argument("--view_camera", action="append", nargs=6, type=float, metavar=("EX", "EY", "EZ", "TX", "TY", "TZ"),
                   help="Score from this camera (eye and target) instead of the ring; repeatable. For inside-out captures, where outside views "
                        "only see the backs of the walls.")
    p.add_argument("--decimate_voxel_size", type=float, metavar="H",
                   help="Replace all splats of every voxel of side H by one splat with their combined weight, mean and covariance: a lighter "
                        "scene without holes. After SOR, before --max_splats; shares its cells with --density_voxel_size.")
    p.add_argument("--preview", metavar="FILE",
                   help="Render the converted scene on the GPU and save it as an 8-bit RGB PNG. The image shows the table that was written, before "
                        "the target format's quantisation.")
    p.add_argument("--preview_size", nargs=2, type=int, metavar=("W", "H"), help="Preview image size in pixels, 1-8192 per side (default 960 540).")
    p.add_argument("--preview_view", nargs=2, type=float, metavar=("AZ", "EL"),
                   help="Preview camera: azimuth and elevation in degrees about the up axis, framed on the scene's bounding box (default 35 20).")
    p.add_argument("--preview_up", metavar="AXIS", help="Preview up axis: +x -x +y -y +z -z (default -y, the COLMAP convention; write --preview_up=-y).")
    p.add_argument("--preview_camera", nargs=6, type=float, metavar=("EX", "EY", "EZ", "TX", "TY", "TZ"),
                   help="Preview camera given as eye and target points instead of --preview_view.")
    p.add_argument("--preview_fov", type=float, metavar="DEG", help="Preview vertical field of view in degrees, between 0 and 170 (default 50).")
    p.add_argument("--fidelity", nargs="?", const="written", choices=("written", "source"), metavar="written|source",
                   help="After the conversion, read the output file back and report PSNR and SSIM of its rendering over a ring of views: against "
                        "the table that was written (written, the default: the target format's loss alone) or against the input file moved by "
                        "--rotate / --scale / --translate (source: filters, decimation, budget, SH reduction and format together).")
    p.add_argument("--fidelity_views", type=int, metavar="N", help="Number of fidelity views on a ring about the reference's bounding box, 1-1024 (default 8).")
    p.add_argument("--fidelity_size", nargs=2, type=int, metavar=("W", "H"), help="Fidelity image size in pixels, 1-8192 per side (default 512 512).")
    p.add_argument("--fidelity_up", metavar="AXIS", help="Up axis of the fidelity ring: +x -x +y -y +z -z (default -y; write --fidelity_up=-y).")
    p.add_argument("--fidelity_camera", action="append", nargs=6, type=float, metavar=("EX", "EY", "EZ", "TX", "TY", "TZ"),
                   help="Measure from this camera (eye and target) instead of the ring; repeatable.")
    p.add_argument("--fidelity_image", metavar="FILE",
                   help="Save the worst view as one PNG: the reference, the output file and four times their difference side by side.")
    p.add_argument("--keep_multicluster", action="store_true", help="Density filter: keep every dense cluster, not only the largest.")
    p.add_argument("--compression_level", type=int, default=0,
                   help="0-9, per format: .ksplat 0 = float32, 1 = float16 blocks, 2+ = 8-bit SH; .spz the gzip level; .sog the palette size.")
    return p


PREVIEW_OPTIONS = ("preview_size", "preview_view", "preview_up", "preview_camera", "preview_fov")
PREVIEW_UP = ("+x", "-x", "+y", "-y", "+z", "-z")


def check_preview_args(args):
    """-> the error line of the first preview flag that cannot be used, or None (no counterpart in the reference)"""
    given = [name for name in PREVIEW_OPTIONS if getattr(args, name) is not None]
    if args.preview is None:
        return f"Error: --{given[0]} needs --preview FILE." if given else None
    if args.info:
        return "Error: --preview renders a conversion's result; it cannot be combined with --info."
    if args.preview_size is not None and not all(1 <= v <= 8192 for v in args.preview_size):
        return f"Error: --preview_size must be between 1 and 8192 per side. Got {args.preview_size[0]} {args.preview_size[1]}."
    if args.preview_fov is not None and not (0.0 < args.preview_fov < 170.0):
        return f"Error: --preview_fov must be between 0 and 170 (exclusive). Got {args.preview_fov}."
    if args.preview_up is not None and args.preview_up.lower() not in PREVIEW_UP + ("x", "y", "z"):
        return f"Error: --preview_up must be one of {' '.join(PREVIEW_UP)}. Got {args.preview_up}."
    if args.preview_view is not None:
        az, el = args.preview_view
        if not (np.isfinite(az) and -90.0 <= el <= 90.0):
            return f"Error: --preview_view must be a finite azimuth and an elevation between -90 and 90. Got {az} {el}."
        if args.preview_camera is not None:
            return "Error: --preview_view and --preview_camera cannot be combined (angles about the scene, or an explicit eye and target)."
    if args.preview_camera is not None:
        c = args.preview_camera
        if not all(np.isfinite(v) for v in c) or list(c[:3]) == list(c[3:]):
            return f"Error: --preview_camera must be six finite numbers with the eye apart from the target. Got {' '.join(f'{v:g}' for v in c)}."
    return None


VIEW_OPTIONS = ("views", "views_size", "views_elevation", "views_up", "view_camera")


def check_view_args(args):
    """-> the error line of the first view-scoring flag that cannot be used, or None (no counterpart in the reference)"""
    given = [name for name in VIEW_OPTIONS if getattr(args, name) is not None]
    by_views = args.rank_by == "views"
    if by_views and args.max_splats is None:
        return "Error: --rank_by views ranks the splats for --max_splats N; give --max_splats too."
    if args.min_contribution is None and not by_views:
        return f"Error: --{given[0]} needs --min_contribution W or --rank_by views." if given else None
    if args.info:
        return "Error: --min_contribution and --rank_by views act on a conversion; they cannot be combined with --info."
    if args.min_contribution is not None and not (0.0 < args.min_contribution < 1.0):
        return f"Error: --min_contribution must be between 0 and 1 (exclusive). Got {args.min_contribution}."
    if args.views is not None and not (1 <= args.views <= 1024):
        return f"Error: --views must be between 1 and 1024. Got {args.views}."
    if args.views_size is not None and not all(1 <= v <= 8192 for v in args.views_size):
        return f"Error: --views_size must be between 1 and 8192 per side. Got {args.views_size[0]} {args.views_size[1]}."
    if args.views_elevation is not None:
        lo, hi = args.views_elevation
        if not (-90.0 <= lo <= hi <= 90.0):
            return f"Error: --views_elevation must be two angles with -90 <= LO <= HI <= 90. Got {lo} {hi}."
    if args.views_up is not None and args.views_up.lower() not in PREVIEW_UP + ("x", "y", "z"):
        return f"Error: --views_up must be one of {' '.join(PREVIEW_UP)}. Got {args.views_up}."
    for c in args.view_camera or []:
        if not all(np.isfinite(v) for v in c) or list(c[:3]) == list(c[3:]):
            return f"Error: --view_camera must be six finite numbers with the eye apart from the target. Got {' '.join(f'{v:g}' for v in c)}."
    if args.view_camera is not None and (args.views is not None or args.views_elevation is not None):
        return "Error: --view_camera replaces the ring; it cannot be combined with --views or --views_elevation."
    return None


FIDELITY_OPTIONS = ("fidelity_views", "fidelity_size", "fidelity_up", "fidelity_camera", "fidelity_image")


def check_fidelity_args(args):
    """-> the error line of the first fidelity flag that cannot be used, or None (no counterpart in the reference)"""
    given = [name for name in FIDELITY_OPTIONS if getattr(args, name) is not None]
    if args.fidelity is None:
        return f"Error: --{given[0]} needs --fidelity." if given else None
    if args.info:
        return "Error: --fidelity measures a conversion's result; it cannot be combined with --info."
    if args.fidelity == "source" and args.merge:
        return "Error: --fidelity source compares against the one input file; it cannot be combined with --merge (use --fidelity written)."
    if args.fidelity_views is not None and not (1 <= args.fidelity_views <= 1024):
        return f"Error: --fidelity_views must be between 1 and 1024. Got {args.fidelity_views}."
    if args.fidelity_size is not None and not all(1 <= v <= 8192 for v in args.fidelity_size):
        return f"Error: --fidelity_size must be between 1 and 8192 per side. Got {args.fidelity_size[0]} {args.fidelity_size[1]}."
    if args.fidelity_up is not None and args.fidelity_up.lower() not in PREVIEW_UP + ("x", "y", "z"):
        return f"Error: --fidelity_up must be one of {' '.join(PREVIEW_UP)}. Got {args.fidelity_up}."
    for c in args.fidelity_camera or []:
        if not all(np.isfinite(v) for v in c) or list(c[:3]) == list(c[3:]):
            return f"Error: --fidelity_camera must be six finite numbers with the eye apart from the target. Got {' '.join(f'{v:g}' for v in c)}."
    if args.fidelity_camera is not None and args.fidelity_views is not None:
        return "Error: --fidelity_camera replaces the ring; it cannot be combined with --fidelity_views."
    return None


def fidelity_kwargs(args) -> dict:
    """Converter.run's fidelity keywords: none at all without --fidelity, and only the flags that were given"""
    if args.fidelity is None:
        return {}
    out = {"fidelity": args.fidelity}
    out.update({name: getattr(args, name) for name in ("fidelity_views", "fidelity_up", "fidelity_image") if getattr(args, name) is not None})
    if args.fidelity_size is not None:
        out["fidelity_size"] = tuple(args.fidelity_size)
    if args.fidelity_camera is not None:
        out["fidelity_cameras"] = [tuple(c) for c in args.fidelity_camera]
    return out


def view_kwargs(args) -> dict:
    """Converter.run's view-scoring keywords: only the flags that were given"""
    out = {name: getattr(args, name) for name in ("min_contribution", "rank_by", "views", "views_size", "views_elevation", "views_up")
           if getattr(args, name) is not None}
    if args.view_camera is not None:
        out["view_cameras"] = [tuple(c) for c in args.view_camera]
    return out


def preview_kwargs(args) -> dict:
    """Converter.run's preview keywords: none at all without --preview, and only the flags that were given"""
    if args.preview is None:
        return {}
    return dict({"preview": args.preview}, **{name: getattr(args, name) for name in PREVIEW_OPTIONS if getattr(args, name) is not None})


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    utils.DEBUG = args.debug

    if args.density_sensitivity is not None and not (0.0 <= args.density_sensitivity <= 1.0):
        print(f"Error: --density_sensitivity must be between 0.0 and 1.0. Got {args.density_sensitivity}.")
        return
    if args.sor_intensity is not None and not (1.0 <= args.sor_intensity <= 10.0):
        print(f"Error: --sor_intensity must be between 1.0 and 10.0. Got {args.sor_intensity}.")
        return
    if args.min_opacity is not None and not (0 <= args.min_opacity <= 255):
        print(f"Error: --min_opacity must be between 0 and 255. Got {args.min_opacity}.")
        return
    if args.max_splats is not None and args.max_splats < 1:
        print(f"Error: --max_splats must be at least 1. Got {args.max_splats}.")
        return
    if args.scale is not None and not (np.isfinite(args.scale) and args.scale > 0):
        print(f"Error: --scale must be a finite number greater than 0. Got {args.scale}.")
        return
    if args.decimate_voxel_size is not None and not (np.isfinite(args.decimate_voxel_size) and args.decimate_voxel_size > 0):
        print(f"Error: --decimate_voxel_size must be a finite number greater than 0. Got {args.decimate_voxel_size}.")
        return
    if args.compression_level < 0 or args.compression_level > 9:
        print(f"Error: --compression_level must be between 0 and 9. Got {args.compression_level}.")
        return
    preview_error = check_preview_args(args) or check_view_args(args) or check_fidelity_args(args)
    if preview_error:
        print(preview_error)
        return

    if args.info:
        import glob
        input_files = glob.glob(args.input)
        if not input_files:
            print(f"Error: No input files found matching '{args.input}'")
            return
        for input_path in input_files:
            report_info(input_path)
        return

    if not args.target_format:
        parser.error("--target_format is required for conversion mode.")
    if args.target_format.lower() not in VALID_FORMATS:
        print(f"Error: Unknown target format '{args.target_format}'. Supported: {', '.join(VALID_FORMATS)}")
        return

    merge_files = args.merge or []                                                              # (no counterpart in the reference)
    for flag, given in (("--merge_rotate", args.merge_rotate), ("--merge_scale", args.merge_scale), ("--merge_translate", args.merge_translate)):
        if given is not None and len(given) != len(merge_files):
            print(f"Error: {flag} was given {len(given)} times for {len(merge_files)} --merge files (once per file, or not at all).")
            return
    for s in args.merge_scale or []:
        if not (np.isfinite(s) and s > 0):
            print(f"Error: --merge_scale must be a finite number greater than 0. Got {s}.")
            return
    for path in merge_files:
        if not os.path.isfile(path):
            print(f"Error: --merge file '{path}' does not exist.")
            return
    merge_transforms = None
    if merge_files and any(g is not None for g in (args.merge_rotate, args.merge_scale, args.merge_translate)):
        merge_transforms = [{"rotate": args.merge_rotate[k] if args.merge_rotate else None, "scale": args.merge_scale[k] if args.merge_scale else None,
                             "translate": args.merge_translate[k] if args.merge_translate else None} for k in range(len(merge_files))]

    if not args.output:                                                                         # :349-371
        base_name, input_ext = os.path.splitext(args.input)
        target_ext = EXTENSIONS.get(args.target_format, "." + args.target_format)
        suffix = ""
        if input_ext.lower() == target_ext.lower():
            suffix = {"cc": "_cc", "compressed_ply": "_compressed", "3dgs": "_3dgs"}.get(args.target_format, "_processed")
        args.output = f"{base_name}{suffix}{target_ext}"
        print(f"Auto-Output: Destination set to {args.output}")

    in_ext = os.path.splitext(args.input)[1].lower()                                            # :373-442
    has_source_extras = check_source_extras(args.input)
    filters_active = any([args.density_voxel_size, args.density_threshold, args.sor_k, args.sor_sigma, args.crop_sh,
                          args.sh_level is not None, args.min_opacity, args.keep_multicluster,
                          args.rotate is not None, args.scale is not None, args.translate is not None, args.max_splats is not None,
                          args.decimate_voxel_size is not None, bool(merge_files), args.preview is not None,
                          args.min_contribution is not None, args.rank_by == "views", args.fidelity is not None,
                          has_source_extras and not args.extra_elements])
    is_same_extension = in_ext == os.path.splitext(args.output)[1].lower()
    if is_same_extension and args.target_format == "3dgs" and not filters_active and args.compression_level == 0 and not args.force:
        print("\n[INFO] Target is generic 3DGS PLY (same as input extension) and no filters are active.")
        if args.extra_elements and has_source_extras:
            print("       (You are maintaining extra elements, so the output would be identical to input).")
        print("       Refer to --help to apply filters (density, SOR, SH reduction) or remove --extra_elements to strip data.")
        print("       Operation aborted to prevent redundant processing.")
        return

    if not os.path.splitext(args.output)[1]:                                                    # :444-453
        args.output += EXTENSIONS.get(args.target_format, "." + args.target_format)
        print(f"Auto-Extension: Appended extension, new output: {args.output}")

    output_dir = os.path.dirname(args.output)
    if output_dir and not os.path.exists(output_dir):
        os.makedirs(output_dir)

    if os.path.exists(args.output) and not args.force:                                          # :460-466
        print(f"Warning: Output file '{args.output}' already exists.")
        if input("Overwrite? [y/N]: ").strip().lower() != "y":
            print("Operation cancelled.")
            return

    try:
        converter = Converter(args.input, args.output, args.target_format)
        print("\n>>> SOURCE FILE INFO")
        report_info(args.input, converter)                                                      # loads the source: run() uses that load
        converter.run(density_voxel_size=args.density_voxel_size, density_threshold=args.density_threshold,
                      density_sensitivity=args.density_sensitivity, keep_multicluster=args.keep_multicluster, sor_k=args.sor_k,
                      sor_sigma=args.sor_sigma, sor_intensity=args.sor_intensity, min_opacity=args.min_opacity, bbox=args.bbox,
                      rgb=args.rgb, sh_level=args.sh_level, bucket_size=args.bucket_size, block_size=args.block_size,
                      crop_sh=args.crop_sh, auto_bbox=args.auto_bbox, compression_level=args.compression_level,
                      maintain_extra_elements=args.extra_elements, rotate=args.rotate, scale=args.scale, translate=args.translate,
                      max_splats=args.max_splats, **({"merge": merge_files, "merge_transforms": merge_transforms} if merge_files else {}),
                      **({"decimate_voxel_size": args.decimate_voxel_size} if args.decimate_voxel_size is not None else {}),
                      **preview_kwargs(args), **view_kwargs(args), **fidelity_kwargs(args))
        print("\n>>> TARGET FILE INFO")
        report_info(args.output)
    except Exception as e:   # noqa: BLE001  (:502)
        print(f"Error: {e}")
        if utils.DEBUG:
            raise e
        sys.exit(1)


if __name__ == "__main__":
    main()
