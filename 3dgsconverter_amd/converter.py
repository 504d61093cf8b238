"""``Converter`` -- the orchestrator of a conversion (the reference's gsconverter/converter.py:12-294) on this package's own
readers, filter chain and writers: a file is converted on a machine that has this repository and an MI355X, and nothing else.

  | step (converter.py)                               | here                                                                |
  |---------------------------------------------------|---------------------------------------------------------------------|
  | :27-61 format by extension, then the header sniff | detect_format: the same tests, host only                            |
  | :63-72, :112-115 the handler's read               | the format's read_* with ``profile={}``: the decoded rows are       |
  |                                                   | profiled in HBM before their download (csrc/table_profile.hip)      |
  | (none: the reference reads one file)              | run(merge=[...]): the union of several sources, re-laid in HBM      |
  | :121-146 45 strided `np.any(col != 0)` scans      | plan_conversion on the profile's 64-bit word                        |
  | :150-252 DataProcessor, the filters in order      | processing.ChainedDataProcessor: one device-resident chain          |
  | (none: the reference cannot move a scene)         | run(rotate=, scale=, translate=): apply_transform before the filters|
  | :263-288 extra elements, the handler's write      | the format's write_*                                                |
  | (none: the reference renders nothing)             | run(preview=...): the written table as a PNG (_write_preview)       |
  | (none: the reference ranks nothing by visibility) | run(min_contribution=, rank_by="views"): prune_by_views             |
  | (none: the reference measures no loss)            | run(fidelity=...): PSNR and SSIM of the file (_measure_fidelity)    |

The decoded rows stay in HBM from the reader to the end of the run (``Converter(..., resident=True)``, the default; readers'
``keep=``, _lib.ResidentRows): the chain's coordinates, the alpha filter's column and the colours' f_dc are gathered from them
on the device, the survivors are taken there (csrc/resident_rows.hip) and downloaded once, and the .splat writer reads the
result where it lies.  ``resident=False``, or a reader that kept nothing, is the path through the host table.

What the user sees -- the ``status_print`` / ``debug_print`` lines, their order, the exceptions and their messages -- is the
reference's.  A file the device readers do not take raises that reader's ``Unsupported*Error``: there is no second reader to
fall back to.  The reference's SOR branch without Taichi computes its mask and returns the table unfiltered;
``remove_flyers`` here applies it, as everywhere in this package.
"""
from __future__ import annotations

import contextlib

from .utils import debug_print, status_print

VALID_FORMATS = ["3dgs", "cc", "parquet", "splat", "ksplat", "spz", "sog", "compressed_ply"]              # :19
FORMAT_MAX_SH = {"3dgs": 3, "cc": 3, "parquet": 3, "ksplat": 2, "splat": 0, "spz": 3, "sog": 3, "compressed_ply": 3}   # :154-163
EXTENSIONS = {"3dgs": ".ply", "cc": ".ply", "compressed_ply": ".ply", "sog": ".sog", "splat": ".splat", "ksplat": ".ksplat",
              "spz": ".spz", "parquet": ".parquet"}                                                       # main.py:354-358
FORMATS_NEEDING_RGB = ["cc", "splat", "ksplat", "sogs", "sog"]                                             # :244
EXTRA_ELEMENT_FORMATS = ["3dgs", "cc"]                                                                     # :275
CC_MARKERS = ("property float scal_f_dc_0", "property float scalar_scal_f_dc_0", "property float scalar_f_dc_0")   # :56


VIEW_KEYWORDS = {"views": "views", "size": "views_size", "elevation": "views_elevation", "up": "views_up", "cameras": "view_cameras"}
FIDELITY_KEYWORDS = ("views", "size", "up", "cameras", "image")     # run(fidelity_views=, ...): they need fidelity=


def detect_format(path: str):
    """:27-61 -> the format's name, or None: the extension, then for anything else the first 2048 bytes as a PLY header"""
    lower = path.lower()
    for ext, name in ((".parquet", "parquet"), (".splat", "splat"), (".ksplat", "ksplat"), (".spz", "spz"), (".sog", "sog")):
        if lower.endswith(ext):
            return name
    debug_print("[DEBUG] Executing '_text_based_detect'...")
    try:
        with open(path, "rb") as f:
            header = f.read(2048).decode("utf-8", errors="ignore")
        if "element chunk" in header:
            return "compressed_ply"
        if "property float f_dc_0" in header:
            return "3dgs"
        if any(m in header for m in CC_MARKERS):
            return "cc"
    except Exception as e:   # noqa: BLE001  (:58 the reference reports any error and detects nothing)
        debug_print(f"[DEBUG] Error identifying PLY flavor: {e}")
    return None


def degree_of_count(n_rest: int) -> int:
    """:125-127: 45 / 24 / 9 f_rest columns -> degree 3 / 2 / 1"""
    return 3 if n_rest >= 45 else 2 if n_rest >= 24 else 1 if n_rest >= 9 else 0


def plan_conversion(names, rest_nonzero: int, target_format: str, kwargs: dict) -> dict:
    """Every decision :121-188 and :244-252 take, from the table's field names and the profile's word alone (bit i: f_rest_i
    holds a value != 0) -> {"source_degree", "final_degree", "messages": the warning and `SH Reduction` lines in order,
    "add_rgb": add_rgb_from_sh is called, "rgb_message": its status line or None}.

    The column COUNT picks the index the backward search starts from (:125-133): 30 columns search f_rest_23 downward, so a
    value in f_rest_29 is not seen."""
    names = tuple(names)
    source = degree_of_count(sum(1 for f in names if f.startswith("f_rest_")))
    if source > 0:
        last = next((i for i in range({3: 44, 2: 23, 1: 8}[source], -1, -1)
                     if f"f_rest_{i}" in names and (rest_nonzero >> i) & 1), -1)
        source = 3 if last >= 24 else 2 if last >= 9 else 1 if last >= 0 else 0                            # :143-146
    limit = FORMAT_MAX_SH.get(target_format, 3)
    requested = kwargs.get("sh_level")
    final, messages = source, []
    if requested is not None:
        if requested > limit:
            messages.append(f"Warning: Requested SH degree {requested} exceeds limit for '{target_format}' ({limit}). Capping to {limit}.")
        if requested > source:
            messages.append(f"Warning: Requested SH degree {requested} exceeds source data degree ({source}). Capping to {source}.")
        final = min(final, requested)
    final = min(final, limit)
    if final < source:
        messages.append(f"SH Reduction: Source degree {source} -> Target degree {final}")
    has_rgb = "red" in names
    add_rgb = ((target_format in FORMATS_NEEDING_RGB and not has_rgb) or bool(kwargs.get("rgb", False))) and not has_rgb
    return {"source_degree": source, "final_degree": final, "messages": messages, "add_rgb": add_rgb,
            "rgb_message": f"Target format '{target_format}' requires RGB. Auto-calculating from SH..." if add_rgb else None}


def transform_values(rotate, scale, translate):
    """run()'s ``rotate= scale= translate=`` (None: none) -> ((rx, ry, rz), s, (tx, ty, tz)) as floats"""
    rx, ry, rz = (float(v) for v in (rotate if rotate is not None else (0.0, 0.0, 0.0)))
    tx, ty, tz = (float(v) for v in (translate if translate is not None else (0.0, 0.0, 0.0)))
    return (rx, ry, rz), 1.0 if scale is None else float(scale), (tx, ty, tz)


def transform_text(rotate, s, translate) -> str:
    """what the `Transform:` status lines say of transform_values' numbers"""
    (rx, ry, rz), (tx, ty, tz) = rotate, translate
    return f"scale {s:g}, rotate [{rx:g}, {ry:g}, {rz:g}] deg, translate [{tx:g}, {ty:g}, {tz:g}]"


class SourceHandler:
    """what the orchestrator and ``report_info`` use of a reference format handler: ``read`` (with the table's profile beside
    it), ``metadata`` after a .ksplat or compressed-PLY read, ``extra_elements`` after a read of either PLY dialect"""

    def __init__(self, format_name: str):
        if format_name not in VALID_FORMATS:
            raise ValueError(f"Unsupported format: {format_name}")                                         # :92
        self.format_name = format_name
        self.profile = None
        self.opens = 0              # decodes of a source file through this handler
        self.keep = True            # ask the reader to keep the decoded rows in HBM
        self.resident = None        # ... the last read's _lib.ResidentRows (the caller takes them over and closes them), or None

    def read(self, path: str, stage_ms: "dict | None" = None):
        name, profile = self.format_name, {}
        self.opens += 1
        self.close()
        keep = {} if self.keep else None
        kw = {"stage_ms": stage_ms, "profile": profile, **({} if keep is None else {"keep": keep})}
        if name in ("3dgs", "cc"):
            from .formats import ply_reader
            data, self.extra_elements = (ply_reader.read_ply_3dgs if name == "3dgs" else ply_reader.read_ply_cc)(path, ascii_body=True, **kw)
        elif name == "compressed_ply":
            from .formats.compressed_ply_reader import read_compressed_ply
            data, _ = read_compressed_ply(path, on_metadata=lambda m: setattr(self, "metadata", m), **kw)
        elif name == "ksplat":
            from .formats.ksplat_reader import read_ksplat
            data, _ = read_ksplat(path, on_metadata=lambda m: setattr(self, "metadata", m), **kw)
        else:
            from .formats import parquet_reader, sog_reader, splat_reader, spz_reader
            read = {"parquet": parquet_reader.read_parquet, "splat": splat_reader.read_splat, "spz": spz_reader.read_spz,
                    "sog": sog_reader.read_sog}[name]
            data = read(path, **kw)
        self.profile = profile
        self.resident = keep.get("rows") if keep else None
        return data

    def take_resident(self):
        """-> the last read's rows in HBM, which are the caller's from here on (None: nothing was kept)"""
        rr, self.resident = self.resident, None
        return rr

    def close(self):
        """free the rows the last read kept, unless somebody took them over (idempotent)"""
        rr = self.take_resident()
        if rr is not None:
            rr.close()

    def write(self, data, path: str, stage_ms: "dict | None" = None, **kwargs):
        name = self.format_name
        import importlib
        module, function = {"3dgs": ("ply_writer", "write_ply_3dgs"), "cc": ("ply_writer", "write_ply_cc"), "parquet": ("parquet_writer", "write_parquet"),
                            "splat": ("splat_writer", "write_splat"), "ksplat": ("ksplat_writer", "write_ksplat"), "spz": ("spz_writer", "write_spz"),
                            "sog": ("sog_writer", "write_sog"), "compressed_ply": ("compressed_ply_writer", "write_compressed_ply")}[name]
        write = getattr(importlib.import_module(".formats." + module, __package__), function)
        if name == "parquet":       # (the reference's writer ignores every keyword)
            return write(data, path, **({} if stage_ms is None else {"stage_ms": stage_ms}))
        if stage_ms is not None and name not in ("sog", "compressed_ply"):
            kwargs = dict(kwargs, stage_ms=stage_ms)
        if name != "splat":         # (the one writer that reads resident rows)
            kwargs.pop("resident", None)
        return write(data, path, **kwargs)


@contextlib.contextmanager
def progress_bar():
    """:103 the tqdm bar when tqdm is importable, no bar otherwise"""
    try:
        from tqdm import tqdm
    except ImportError:
        class _NoBar:
            def update(self, n):
                pass

            def set_description(self, text):
                pass

            def refresh(self):
                pass
        yield _NoBar()
        return
    with tqdm(total=100, desc="Converting", bar_format="{desc}: {percentage:3.0f}% |{bar}| {n_fmt}/{total_fmt}") as pbar:
        yield pbar


class Converter:
    def __init__(self, input_path, output_path, target_format, resident=True):
        """resident: keep the reader's decoded rows in HBM for the filters, the one materialise and the .splat writer (module
        docstring); False: every stage works from the host table"""
        self.resident = bool(resident)
        self.input_path = input_path
        self.output_path = output_path
        self.target_format = target_format.lower()
        if self.target_format not in VALID_FORMATS:
            raise ValueError(f"Unknown target format '{self.target_format}'. Supported: {', '.join(VALID_FORMATS)}")
        self.data = None
        self.source_format = None
        self.source_handler = None
        self.profile = None
        self.stage_ms = {}          # the last run's stage clocks: read_*, process, write_*
        self.last_preview = {}      # the last run's preview: visible, instances, rows and the render plan (run(preview=...))
        self.last_fidelity = {}     # the last run's fidelity.summarise result (run(fidelity=...)); {}: none asked for, or not measured
        self._loaded = None         # (path, handler, data, profile) of load_source_only: run() decodes the source no second time

    def _detect_format(self, path):
        return detect_format(path)

    def _get_format_handler(self, format_name):
        handler = SourceHandler(format_name)
        handler.keep = self.resident
        return handler

    def close(self):
        """free what a load_source_only() without a run() left in HBM (idempotent; run() closes everything itself)"""
        if self._loaded is not None and hasattr(self._loaded[1], "close"):
            self._loaded[1].close()
        if self.source_handler is not None and hasattr(self.source_handler, "close"):
            self.source_handler.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_source_only(self):
        """:63-72: detect, read, keep -- and remember the table with its profile for a run() on the same path"""
        self.source_format = self._detect_format(self.input_path)
        if not self.source_format:
            raise ValueError("Could not detect source format")
        debug_print(f"[DEBUG] Detected source format: {self.source_format}")
        self.source_handler = self._get_format_handler(self.source_format)
        self.data = self.source_handler.read(self.input_path)
        self.profile = self.source_handler.profile
        self._loaded = (self.input_path, self.source_handler, self.data, self.profile)
        return self.data

    def run(self, **kwargs):
        """the reference's keywords, and ``rotate=(rx, ry, rz)`` (degrees: about the fixed X, then Y, then Z axis), ``scale=s`` and
        ``translate=(tx, ty, tz)``: the scene transform p' = s R p + t, applied right after the SH cap and before every filter;
        and ``decimate_voxel_size=H``: one moment-matched splat per occupied voxel of side H (DataProcessor.decimate), applied
        after SOR and before the budget;
        and ``max_splats=N``: keep the N most visible splats (DataProcessor.limit_splats), applied after every other filter;
        and ``min_contribution=W``: drop every splat whose largest blending weight over a ring of rendered views stays under W
        (DataProcessor.prune_by_views), after the decimation and before the budget; ``rank_by="views"``: the budget keeps the
        splats the views see most instead of the largest ones; both from one scoring pass, whose views are ``views=N``,
        ``views_size=(w, h)``, ``views_elevation=(lo, hi)``, ``views_up=``, or ``view_cameras=[(ex, ey, ez, tx, ty, tz), ...]``;
        and ``merge=[path, ...]`` with ``merge_transforms=[None | {"rotate":, "scale":, "translate":}, ...]``: further sources
        whose rows follow the main source's in one table (_merge_sources), before everything else;
        and ``preview=PATH`` with ``preview_size=(w, h)``, ``preview_view=(azimuth, elevation)``, ``preview_up=``,
        ``preview_camera=(ex, ey, ez, tx, ty, tz)``, ``preview_fov=``: a PNG of the written table, rendered after the writer has
        returned (_write_preview);
        and ``fidelity="written" | "source"`` with ``fidelity_views=N``, ``fidelity_size=(w, h)``, ``fidelity_up=``,
        ``fidelity_cameras=[(ex, ey, ez, tx, ty, tz), ...]``, ``fidelity_image=PATH``: PSNR and SSIM of the output file, read
        back, against the written table or the moved source over a ring of views (_measure_fidelity), after the preview"""
        debug_print(f"[DEBUG] Starting conversion: {self.input_path} -> {self.output_path} ({self.target_format})")
        clocks = self.stage_ms = {}
        held = []                   # the processor of this run: whatever it still holds in HBM is freed on every exit path
        try:
            self._run(clocks, held, kwargs)
        finally:
            for p in held:
                p.close()
            self.close()
        status_print(f"Conversion completed: Saved to {self.output_path}")

    def _merge_sources(self, clocks, paths, transforms):
        """``run(merge=[path, ...], merge_transforms=[None | {"rotate":, "scale":, "translate":}, ...])``: the union of the main
        source and the extra files, in that order, in the common row layout of merge.merged_dtype.  Every extra file is read
        once by a handler of its own and moved by its own transform alone; then every source's rows are re-laid at their row
        offset of one table -- in HBM when every reader kept its rows (ResidentRows.concat: csrc/rows_remap.hip; the host table
        is ONE download of the union, its profile one pass over it there), else on the host (gsx_rows_remap_host).  Afterwards
        ``self.data``, ``self.profile`` and the main handler's resident rows are the union's: the global transform and every
        filter act on it as on a single source.  Clocks: merge_read (the extras' reads, summed), merge_transform, merge_remap,
        and merge_download on the resident path."""
        import time

        import numpy as np

        from . import _lib, merge, transform
        transforms = [None] * len(paths) if transforms is None else list(transforms)
        if len(transforms) != len(paths):
            raise ValueError(f"merge_transforms: one entry per merge source (None: none), got {len(transforms)} for {len(paths)}")
        main = self.source_handler
        tables, rows = [self.data], [main.take_resident() if hasattr(main, "take_resident") else None]
        stale = [False]             # a source's rows in HBM were moved: its host table still holds the old frame
        ms = {}
        try:
            for k, (path, tf) in enumerate(zip(paths, transforms), 1):
                fmt = self._detect_format(path)
                if not fmt:
                    raise ValueError(f"Could not detect source format of merge source '{path}'")
                handler = self._get_format_handler(fmt)
                with _lib.stage_clock(clocks, "merge_read"):
                    table = handler.read(path)
                tables.append(table)
                rows.append(handler.take_resident())
                stale.append(False)
                status_print(f"Merge: {path} ({fmt.upper()}, {len(table):,} splats)")
                if tf:
                    rotate, s, translate = transform_values(tf.get("rotate"), tf.get("scale"), tf.get("translate"))
                    status_print(f"Merge Transform [{k}]: {transform_text(rotate, s, translate)}")
                    plan = transform.plan_transform(table.dtype, transform.rotation_from_euler_deg(*rotate), s, translate)
                    with _lib.stage_clock(clocks, "merge_transform"):
                        if rows[k] is not None:
                            rows[k].transform(plan)
                            stale[k] = not plan.identity and len(table) > 0
                        else:
                            tables[k] = _lib.rows_transform_table(table, plan)
            labels = [repr(p) for p in [self.input_path] + paths]
            merged, notes = merge.merged_dtype([t.dtype for t in tables], labels)
            runs = [merge.remap_runs(t.dtype, merged) for t in tables]
            if all(rr is not None for rr in rows):
                union = _lib.ResidentRows.concat(rows, merged, runs, stage_ms=ms)
                main.resident = union                       # (this run's from here on: run() closes the handler on every path)
                while rows:
                    rows.pop().close()
                with _lib.stage_clock(ms, "download"):
                    self.data = union.download()
                self.profile = union.profile()
            else:
                for k, table in enumerate(tables):
                    if stale[k]:
                        tables[k] = rows[k].download()
                while rows:
                    rr = rows.pop()
                    if rr is not None:
                        rr.close()
                out = np.empty(sum(len(t) for t in tables), merged)
                with _lib.stage_clock(ms, "remap"):
                    row0 = 0
                    for table, table_runs in zip(tables, runs):
                        if table.ndim == 1 and table.flags.c_contiguous and table.dtype.itemsize <= _lib.RESIDENT_MAX_ROW_BYTES:
                            _lib.rows_remap_host(table, table_runs, out, row0)
                        else:
                            merge.remap_fields(table, out, row0)
                        row0 += len(table)
                self.data, self.profile = out, _lib.host_table_profile(out)
        finally:
            for rr in rows:
                if rr is not None:
                    rr.close()
        clocks.update({"merge_" + k: v for k, v in ms.items()})
        n_rest = sum(1 for nm in merged.names if nm.startswith("f_rest_"))
        status_print(f"Merged {len(tables)} sources: {len(self.data):,} splats, {n_rest} SH columns.")
        for line in notes:
            status_print(line)

    def _write_preview(self, processor, path, options, clocks):
        """``run(preview=PATH, preview_size=, preview_view=, preview_up=, preview_camera=, preview_fov=)``: after the writer has
        returned, the table that was written -- the processor's rows in HBM on the resident path, else ``self.data`` uploaded
        once -- is rendered (DataProcessor.render_preview) and stored as an 8-bit RGB PNG.  The image shows the table before the
        target format's quantisation.  Clocks: preview_* (the renderer's stages and preview_png).  A scene that needs more
        instance workspace than the renderer's budget prints a warning and the conversion still completes; any other error
        propagates."""
        from . import _lib, render
        kw = {k: v for k, v in options.items() if v is not None}
        ms = {}
        try:
            image = processor.render_preview(stage_ms=ms, **kw)
        except render.RenderRefused as e:
            status_print(f"Warning: preview not written: {e}")
            return
        with _lib.stage_clock(ms, "png"):
            render.write_png(path, image)
        clocks.update({"preview_" + k: v for k, v in ms.items()})
        info = self.last_preview = getattr(processor, "last_preview", {})
        status_print(f"Preview: {image.shape[1]} x {image.shape[0]}, {info.get('visible', 0):,} of {info.get('rows', len(self.data)):,} splats visible, "
                     f"saved to {path}")

    def _measure_fidelity(self, processor, source_format, opts, image_path, moved, clocks):
        """``run(fidelity="written" | "source", fidelity_views=, fidelity_size=, fidelity_up=, fidelity_cameras=,
        fidelity_image=)``: after the writer (and the preview) the output file is read back by this package's own reader for
        the target format -- a fresh handler, its rows kept in HBM on the resident path -- and compared in image space with a
        reference (fidelity.compare_tables).  'written': the reference is the table that was written, the rows
        _write_preview renders, so the figures are the format's loss alone.  'source': the reference is the input file read a
        second time by a fresh handler (the first load was changed in place), moved by the run's own transform and nothing
        else, so the figures are everything the run did.  The cameras frame the reference's bounds.  ``last_fidelity``: the
        result ({} when nothing was measured); clocks: fidelity_read, fidelity_transform, the render stages summed,
        fidelity_compare.  fidelity_image: the worst view rendered once more for both tables and stored as one PNG of the
        reference, the test and four times their difference side by side.  A view that needs more instance workspace than the
        renderer's budget, or a table the renderer cannot take (render.plan_render's refusals: a missing geometry field, a
        field that is not float32), prints a warning and the conversion still completes; any other error propagates.
        Everything the comparison holds in HBM is freed on every exit path."""
        from . import _lib, fidelity, render, transform, views
        ms = {}
        mode = opts["mode"]
        view_kw = {k: opts[k] for k in ("views", "size", "elevation", "up", "fov", "cameras")}
        handlers = []
        try:
            test_handler = self._get_format_handler(self.target_format)
            handlers.append(test_handler)
            with _lib.stage_clock(ms, "read"):
                test = test_handler.read(self.output_path)
            test = test_handler.resident if test_handler.resident is not None else test
            if mode == "written":
                rr = getattr(processor, "resident", None)
                ref = rr if rr is not None else processor.data
                what = f"written table vs {self.output_path}"
            else:
                ref_handler = self._get_format_handler(source_format)
                handlers.append(ref_handler)
                with _lib.stage_clock(ms, "read"):
                    ref = ref_handler.read(self.input_path)
                if moved is not None:
                    plan = transform.plan_transform(ref.dtype, *moved)
                    with _lib.stage_clock(ms, "transform"):
                        if ref_handler.resident is not None:
                            ref_handler.resident.transform(plan)
                        else:
                            ref = _lib.rows_transform_table(ref, plan)
                ref = ref_handler.resident if ref_handler.resident is not None else ref
                what = f"{self.input_path} vs {self.output_path}"
            try:                    # (what the renderer cannot take of either table: asked before any device work)
                probe = views.plan_views((0, 0, 0), (0, 0, 0), **view_kw)[0]
                for t in (ref, test):
                    render.plan_render(t.dtype, probe, background=fidelity.BACKGROUND)
            except (ValueError, TypeError) as e:
                status_print(f"Warning: fidelity not measured: {e}")
                return
            try:
                res = fidelity.compare_tables(ref, test, stage_ms=ms, max_work_bytes=fidelity.MAX_WORK_BYTES, **view_kw)
                if image_path is not None:
                    cam = res["cameras"][res["worst_view"]]
                    pair = []
                    for t in (ref, test):
                        plan = render.plan_render(t.dtype, cam, background=fidelity.BACKGROUND)
                        pair.append(t.render(plan) if isinstance(t, _lib.ResidentRows) else _lib.render_table(t, plan))
                    with _lib.stage_clock(ms, "png"):
                        render.write_png(image_path, fidelity.side_by_side(*pair))
            except render.RenderRefused as e:
                status_print(f"Warning: fidelity not measured: {e}")
                return
        finally:
            for h in handlers:
                h.close()
            clocks.update({"fidelity_" + k: v for k, v in ms.items()})
        self.last_fidelity = res
        status_print(fidelity.report_line(res, what))
        if image_path is not None:
            status_print(f"Fidelity image: view {res['worst_view']}, reference | test | 4 x difference, saved to {image_path}")

    def _run(self, clocks, held, kwargs):
        import time
        from .processing.data_processor import ChainedDataProcessor
        # the fidelity options are checked first: a refusal comes before any file is read
        fidelity_kw = {k: kwargs.pop("fidelity_" + k, None) for k in FIDELITY_KEYWORDS}
        fidelity_mode = kwargs.pop("fidelity", None)
        self.last_fidelity = {}
        if fidelity_mode is None and any(v is not None for v in fidelity_kw.values()):
            raise ValueError(f"{', '.join('fidelity_' + k for k, v in fidelity_kw.items() if v is not None)} need fidelity='written' or 'source'")
        if fidelity_mode is not None:
            from . import fidelity as _fidelity
            fidelity_image = fidelity_kw.pop("image")
            fidelity_opts = _fidelity.check_options(fidelity_mode, merge=kwargs.get("merge"), **fidelity_kw)
        with progress_bar() as pbar:
            source_format = self._detect_format(self.input_path)
            if not source_format:
                raise ValueError("Could not detect source format")
            debug_print(f"[DEBUG] Detected source format: {source_format}")
            pbar.update(5)

            pbar.set_description("Reading Source")
            if self._loaded is not None and self._loaded[0] == self.input_path:
                _, self.source_handler, self.data, self.profile = self._loaded
            else:
                self.source_handler = self._get_format_handler(source_format)
                read_ms = {}
                self.data = self.source_handler.read(self.input_path, stage_ms=read_ms)
                self.profile = self.source_handler.profile
                clocks.update({"read_" + k: v for k, v in read_ms.items()})
            self._loaded = None     # (the table is about to change in place: cap_sh_degree)
            preview = {k: kwargs.pop("preview_" + k) for k in ("size", "view", "up", "camera", "fov") if "preview_" + k in kwargs}
            preview_path = kwargs.pop("preview", None)
            merge_paths, merge_transforms = kwargs.pop("merge", None), kwargs.pop("merge_transforms", None)
            if merge_paths:
                self._merge_sources(clocks, list(merge_paths), merge_transforms)
            pbar.update(25)

            plan = plan_conversion(self.data.dtype.names, self.profile["rest_nonzero"], self.target_format, kwargs)
            pbar.set_description("Processing")
            t0 = time.perf_counter()
            kept = self.source_handler.take_resident() if hasattr(self.source_handler, "take_resident") else None
            processor = ChainedDataProcessor(self.data, resident=kept) if kept is not None else ChainedDataProcessor(self.data)
            held.append(processor)
            self.format_max_sh = dict(FORMAT_MAX_SH)
            for line in plan["messages"]:
                status_print(line)
            processor.cap_sh_degree(plan["final_degree"])
            # the scene transform is the first processing step: the box, the voxel size and SOR all work in the output frame
            rotate, scale, translate = kwargs.pop("rotate", None), kwargs.pop("scale", None), kwargs.pop("translate", None)
            moved = None            # (rotation, s, translation) of the run's own transform: the fidelity's source reference takes it too
            if rotate is not None or scale is not None or translate is not None:
                from . import transform
                (rx, ry, rz), s, (tx, ty, tz) = transform_values(rotate, scale, translate)
                status_print(f"Transform: {transform_text((rx, ry, rz), s, (tx, ty, tz))}")
                moved = (transform.rotation_from_euler_deg(rx, ry, rz), s, (tx, ty, tz))
                processor.apply_transform(rotation=moved[0], translation=moved[2], scale=s)
            pbar.update(5)

            pbar.set_description("Filtering")
            if kwargs.get("bbox"):
                processor.crop_by_bbox(*kwargs["bbox"])
            min_opacity = kwargs.get("min_opacity")
            if min_opacity is not None and min_opacity > 0:
                processor.apply_alpha_filter(min_opacity)
            d_voxel, d_thresh, d_sens = kwargs.get("density_voxel_size"), kwargs.get("density_threshold"), kwargs.get("density_sensitivity")
            if (d_voxel is not None and d_thresh is not None) or d_sens is not None:
                processor.apply_density_filter(1.0 if d_voxel is None else float(d_voxel), 0.32 if d_thresh is None else float(d_thresh),
                                               sensitivity=d_sens, keep_multicluster=kwargs.get("keep_multicluster", False))
            pbar.update(10)
            s_k, s_sigma, s_intensity = kwargs.get("sor_k"), kwargs.get("sor_sigma"), kwargs.get("sor_intensity")
            if (s_k is not None and s_sigma is not None) or s_intensity is not None:
                pbar.set_description("Filtering (SOR)")
                processor.remove_flyers(25 if s_k is None else int(s_k), 10.5 if s_sigma is None else float(s_sigma), intensity=s_intensity)
            # the decimation follows SOR -- outliers are not averaged into their voxel's splat -- and precedes the budget, which
            # stays the only step that names the final size
            decimate_voxel_size = kwargs.pop("decimate_voxel_size", None)
            if decimate_voxel_size is not None:
                pbar.set_description("Decimating")
                processor.decimate(decimate_voxel_size)
            # the view scores follow the decimation: they belong to the geometry that is written.  With both options one scoring
            # pass serves the threshold and the budget, which ranks the threshold's survivors
            min_contribution, rank_by = kwargs.pop("min_contribution", None), kwargs.pop("rank_by", None)
            view_kw = {name: kwargs.pop(key) for name, key in VIEW_KEYWORDS.items() if kwargs.get(key) is not None}
            for key in VIEW_KEYWORDS.values():
                kwargs.pop(key, None)
            # the splat budget is the last filter: the box that is printed and the colours belong to what is written
            max_splats = kwargs.pop("max_splats", None)
            by_views = rank_by == "views"
            if rank_by not in (None, "size", "views"):
                raise ValueError(f"rank_by must be 'size' or 'views', got {rank_by!r}")
            if by_views and max_splats is None:
                raise ValueError("rank_by='views' ranks the rows for max_splats: give max_splats too")
            if view_kw and min_contribution is None and not by_views:
                raise ValueError(f"{', '.join(VIEW_KEYWORDS[k] for k in view_kw)} need min_contribution or rank_by='views'")
            if min_contribution is not None:
                pbar.set_description("Scoring Views")
                processor.prune_by_views(min_contribution, max_count=max_splats if by_views else None, **view_kw)
            elif by_views:
                pbar.set_description("Scoring Views")
                processor.limit_splats(max_splats, rank_by="views", **view_kw)
            if max_splats is not None and not by_views:
                processor.limit_splats(max_splats)
            pbar.update(10)
            if kwargs.get("auto_bbox"):
                processor.apply_auto_bbox()
            if plan["add_rgb"]:
                status_print(plan["rgb_message"])
                processor.add_rgb_from_sh()
            pbar.update(5)
            self.data = processor.data
            clocks["process"] = round((time.perf_counter() - t0) * 1e3, 3)
            clocks.update({"process_" + k: v for k, v in getattr(processor, "resident_ms", {}).items()})
            if self.target_format == "splat" and getattr(processor, "resident", None) is not None:
                kwargs = dict(kwargs, resident=processor.resident)

            pbar.set_description(f"Writing {self.target_format.upper()}")
            extras = getattr(self.source_handler, "extra_elements", None)
            if kwargs.get("maintain_extra_elements", False):
                if extras:
                    kwargs["extra_elements"] = extras
                    if self.target_format not in EXTRA_ELEMENT_FORMATS:
                        status_print(f"Warning: Target format '{self.target_format}' does not support preserving extra elements. These will be ignored.")
                else:
                    status_print("Warning: --extra_elements passed but no extra elements found in source.")
            elif extras:
                status_print(f"Stripping {len(extras)} extra PLY elements (use --extra_elements to preserve).")
            write_ms = {}
            self._get_format_handler(self.target_format).write(self.data, self.output_path, stage_ms=write_ms, **kwargs)
            clocks.update({"write_" + k: v for k, v in write_ms.items()})
            if preview_path is not None:
                pbar.set_description("Rendering Preview")
                self._write_preview(processor, preview_path, preview, clocks)
            if fidelity_mode is not None:
                pbar.set_description("Measuring Fidelity")
                self._measure_fidelity(processor, source_format, fidelity_opts, fidelity_image, moved, clocks)
            pbar.update(40)
            pbar.refresh()
            pbar.set_description("Completed")
