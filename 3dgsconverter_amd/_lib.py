"""ctypes binding of libgsx_hip.so (C ABI declared in include/gsx_hip.h).

numpy + ctypes only -- no torch, no Taichi.  The library is built in-tree by
``3dgsconverter_amd/build.py`` (hipcc, gfx950).  There is deliberately NO CPU
fallback anywhere in this package: if the library or a GPU is missing the calls
raise ``GsxError`` (a RuntimeError).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import os
import re
import threading
import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GSX_LIB_PATH: an experiment build of build.py (GSX_EXTRA_FLAGS -> 3dgsconverter_amd/variants/), for A/B runs only
LIB_PATH = os.environ.get("GSX_LIB_PATH") or os.path.join(_HERE, "libgsx_hip.so")

KNN_AUTO, KNN_BRUTE, KNN_GRID, KNN_TREE = 0, 1, 2, 3
PROBE_ROOT_DIST2, PROBE_ROOT_DSQRT = 0, 1                                    # gsx_knn_probe_root_dev modes
PROBE_SHORT_ROOT, PROBE_SHORT_SEED = 0, 1                                    # gsx_knn_probe_root_short_dev modes
PROBE_MEAN_NET, PROBE_MEAN_LIST, PROBE_MEAN_LE128, PROBE_MEAN_NP = 0, 1, 2, 3   # gsx_knn_probe_mean_dev forms
T_SOR_KNN, T_SOR_BIN, T_SOR_FALLBACK, T_SOR_STATS, T_DENSITY, T_KMEANS_ASSIGN, T_KMEANS_UPDATE, T_QUANTIZE = range(8)
T_SLAB_PREP, T_SLAB_ROWS, T_SLAB_MEANS, T_SLAB_COLL = range(8, 12)   # multi-GPU slab step (round 5)


class GsxError(RuntimeError):
    """Raised for every failure of the HIP path (missing library, no GPU, HIP error)."""


class SorInfo(C.Structure):
    _fields_ = [("algo", C.c_int32), ("grid_dim", C.c_int32 * 3), ("cell_size", C.c_float),
                ("n_cells", C.c_int64), ("n_bricks", C.c_int64), ("n_fallback", C.c_int64),
                ("n_exhaustive", C.c_int64), ("n_deferred_bricks", C.c_int64), ("n_refined", C.c_int64)]

    def as_dict(self):
        return {"algo": int(self.algo), "grid_dim": tuple(int(v) for v in self.grid_dim),
                "cell_size": float(self.cell_size), "n_cells": int(self.n_cells), "n_bricks": int(self.n_bricks),
                "n_fallback": int(self.n_fallback), "n_exhaustive": int(self.n_exhaustive),
                "n_deferred_bricks": int(self.n_deferred_bricks), "n_refined": int(self.n_refined)}


class SlabPlan(C.Structure):
    """gsx_slab_plan_t (include/gsx_hip.h)"""
    _fields_ = [("status", C.c_int32), ("world", C.c_int32), ("rank", C.c_int32), ("axis", C.c_int32), ("halo_bins", C.c_int32),
                ("lo", C.c_float), ("hi", C.c_float), ("plane_lo", C.c_float), ("plane_hi", C.c_float), ("cut", C.c_int32 * 17),
                ("n_local", C.c_int64), ("n_total", C.c_int64), ("n_own", C.c_int64), ("n_halo", C.c_int64), ("n_send", C.c_int64),
                ("halo_total", C.c_int64), ("sizes", C.c_int64 * 16),
                ("own_cnt", C.c_int64 * 16), ("halo_cnt", C.c_int64 * 16), ("own_off", C.c_int64 * 16), ("halo_off", C.c_int64 * 16),
                ("in_own", C.c_int64 * 16), ("in_halo", C.c_int64 * 16), ("r_own_off", C.c_int64 * 16), ("r_halo_off", C.c_int64 * 16)]

    def as_dict(self):
        g = int(self.world)
        out = {k: (int(getattr(self, k)) if k not in ("lo", "hi", "plane_lo", "plane_hi") else float(getattr(self, k)))
               for k in ("status", "world", "rank", "axis", "halo_bins", "lo", "hi", "plane_lo", "plane_hi", "n_local", "n_total", "n_own",
                         "n_halo", "n_send", "halo_total")}
        out["cut"] = [int(v) for v in self.cut[:g + 1]]
        for k in ("sizes", "own_cnt", "halo_cnt", "own_off", "halo_off", "in_own", "in_halo", "r_own_off", "r_halo_off"):
            out[k] = [int(v) for v in getattr(self, k)[:g]]
        return out


class RefineSizingIn(C.Structure):
    """gsx_refine_sizing_in (include/gsx_hip.h)"""
    _fields_ = [("qb_lo", C.c_float * 3), ("qb_hi", C.c_float * 3), ("sub_queries", C.c_uint32), ("n_sub", C.c_uint32),
                ("pts_per_cell", C.c_double), ("parent_h", C.c_float), ("adaptive", C.c_int32), ("hist", C.c_uint32 * 32),
                ("bin_vol", C.c_double)]


class RefineSizingOut(C.Structure):
    """gsx_refine_sizing_out (include/gsx_hip.h)"""
    _fields_ = [("nd3", C.c_int32), ("probe_g", C.c_int32), ("h_est", C.c_double), ("margin", C.c_double), ("cert", C.c_double),
                ("clip_lo", C.c_float * 3), ("clip_hi", C.c_float * 3), ("r_cert", C.c_float), ("h_hint", C.c_double)]


class SlabStep(C.Structure):
    """gsx_slab_step_t (include/gsx_hip.h)"""
    _fields_ = [("status", C.c_int32), ("plan", SlabPlan), ("mask_dev", C.c_void_p), ("mean_dists_dev", C.c_void_p),
                ("stats_dev", C.c_void_p), ("uncertain_dev", C.c_void_p)]


class DensityInfo(C.Structure):
    """gsx_density_info (include/gsx_hip.h)"""
    _fields_ = [("status", C.c_int32), ("n_unique", C.c_int64), ("n_dense", C.c_int64), ("n_kept_voxels", C.c_int64),
                ("kept_clusters", C.c_int64), ("largest", C.c_int64)]


SOG_FIELDS = 59   # GSX_SOG_FIELDS: x y z | rot_0..3 | scale_0..2 | f_dc_0..2 | opacity | f_rest_0..44
SOG_FIELD_NAMES = (["x", "y", "z", "rot_0", "rot_1", "rot_2", "rot_3", "scale_0", "scale_1", "scale_2", "f_dc_0", "f_dc_1", "f_dc_2", "opacity"]
                   + ["f_rest_%d" % i for i in range(45)])


class SogLayout(C.Structure):
    """gsx_sog_layout (include/gsx_hip.h): where the writer's float32 fields sit inside a row of the structured table"""
    _fields_ = [("row_bytes", C.c_int64), ("n_rest", C.c_int32), ("offset", C.c_int32 * SOG_FIELDS)]


class SpzLayout(C.Structure):
    """gsx_spz_layout (include/gsx_hip.h): the SPZ writer's fields inside a row, -1 = absent"""
    _fields_ = [("row_bytes", C.c_int64), ("offset", C.c_int32 * SOG_FIELDS)]


CPLY_READ_MAX_SH = 256   # GSX_CPLY_READ_MAX_SH


class CplyReadLayout(C.Structure):
    """gsx_cply_read_layout (include/gsx_hip.h): where the compressed-PLY reader's properties sit inside the file's rows"""
    _fields_ = [("chunk_stride", C.c_int64), ("vertex_stride", C.c_int64), ("sh_stride", C.c_int64), ("chunk_offset", C.c_int32 * 18),
                ("vertex_offset", C.c_int32 * 4), ("n_sh", C.c_int32), ("sh_offset", C.c_int32 * CPLY_READ_MAX_SH)]


PLY_READ_MAX_FIELDS = 128   # GSX_PLY_READ_MAX_FIELDS
PLY_READ_MAX_STRIDE = 512   # bytes per input or output row (csrc/row_tile.h SPZ_MAX_ROW_BYTES)
PLY_TYPE_CODES = {"i1": 0, "u1": 1, "i2": 2, "u2": 3, "i4": 4, "u4": 5, "f4": 6, "f8": 7}   # GSX_PLY_T_*: convert to float32 by value
PLY_T_RAW = 8               # GSX_PLY_T_RAW: copy dst_bytes bytes


class PlyReadLayout(C.Structure):
    """gsx_ply_read_layout (include/gsx_hip.h): the 3DGS / CloudCompare PLY readers' field descriptors"""
    _fields_ = [("in_stride", C.c_int32), ("out_stride", C.c_int32), ("n_fields", C.c_int32), ("big_endian", C.c_int32),
                ("src_offset", C.c_int32 * PLY_READ_MAX_FIELDS), ("src_type", C.c_int32 * PLY_READ_MAX_FIELDS),
                ("dst_offset", C.c_int32 * PLY_READ_MAX_FIELDS), ("dst_bytes", C.c_int32 * PLY_READ_MAX_FIELDS)]


PLY_TEXT_MAX_PROPS = 512    # GSX_PLY_TEXT_MAX_PROPS
PLY_TEXT_RESULT_WORDS = 6   # GSX_PLY_TEXT_TOKENS, _LINES, _ROWS, _BAD_LINE, _FLAGGED, _END
DEC_FLAGGED = 2             # GSX_DEC_FLAGGED


class PlyTextLayout(C.Structure):
    """gsx_ply_text_layout (include/gsx_hip.h): the properties of an ASCII PLY element, one token each"""
    _fields_ = [("n_props", C.c_int32), ("in_stride", C.c_int32), ("offset", C.c_int32 * PLY_TEXT_MAX_PROPS),
                ("type", C.c_int32 * PLY_TEXT_MAX_PROPS)]


PLY_WRITE_MAX_RUNS = 128    # GSX_PLY_WRITE_MAX_RUNS
PLY_WRITE_MAX_STRIDE = 512  # bytes per row of the table or of the file (csrc/row_tile.h SPZ_MAX_ROW_BYTES)


class PlyWriteLayout(C.Structure):
    """gsx_ply_write_layout (include/gsx_hip.h): the 3DGS / CloudCompare PLY writers' run table"""
    _fields_ = [("in_stride", C.c_int32), ("out_stride", C.c_int32), ("n_runs", C.c_int32), ("reserved", C.c_int32),
                ("src_offset", C.c_int32 * PLY_WRITE_MAX_RUNS), ("dst_offset", C.c_int32 * PLY_WRITE_MAX_RUNS),
                ("bytes", C.c_int32 * PLY_WRITE_MAX_RUNS)]


PARQUET_MAX_FIELDS = 128    # GSX_PARQUET_MAX_FIELDS
PARQUET_MAX_STRIDE = 512    # bytes per row of the table (csrc/row_tile.h SPZ_MAX_ROW_BYTES)
PARQUET_TYPE_CODES = dict(PLY_TYPE_CODES, i8=9, u8=10, f2=11)   # + GSX_PARQUET_T_I8 / _U8 / _F2: convert to float32 by value
PARQUET_TYPE_BYTES = {0: 1, 1: 1, 2: 2, 3: 2, 4: 4, 5: 4, 6: 4, 7: 8, 9: 8, 10: 8, 11: 2}


class ParquetRowsLayout(C.Structure):
    """gsx_parquet_rows_layout (include/gsx_hip.h): the Parquet reader's field descriptors"""
    _fields_ = [("out_stride", C.c_int32), ("n_fields", C.c_int32),
                ("src_type", C.c_int32 * PARQUET_MAX_FIELDS), ("dst_offset", C.c_int32 * PARQUET_MAX_FIELDS),
                ("dst_bytes", C.c_int32 * PARQUET_MAX_FIELDS), ("col_offset", C.c_int64 * PARQUET_MAX_FIELDS),
                ("valid_offset", C.c_int64 * PARQUET_MAX_FIELDS)]


class ParquetColumnsLayout(C.Structure):
    """gsx_parquet_columns_layout (include/gsx_hip.h): the Parquet writer's field descriptors"""
    _fields_ = [("in_stride", C.c_int32), ("n_fields", C.c_int32),
                ("src_offset", C.c_int32 * PARQUET_MAX_FIELDS), ("bytes", C.c_int32 * PARQUET_MAX_FIELDS),
                ("kind", C.c_int32 * PARQUET_MAX_FIELDS), ("col_offset", C.c_int64 * PARQUET_MAX_FIELDS),
                ("valid_offset", C.c_int64 * PARQUET_MAX_FIELDS)]


class KsplatReadSection(C.Structure):
    """gsx_ksplat_read_section (include/gsx_hip.h): one section of a .ksplat file as the reader's kernel walks it"""
    _fields_ = [("rows_offset", C.c_int64), ("centres_offset", C.c_int64), ("n_rows", C.c_int64), ("out_row", C.c_int64),
                ("full_rows", C.c_int64), ("prefix_offset", C.c_int64), ("bucket_size", C.c_uint32), ("n_full", C.c_uint32),
                ("n_partial", C.c_uint32), ("n_buckets", C.c_uint32), ("sh_count", C.c_int32), ("scale_range", C.c_float),
                ("scale_factor", C.c_float)]


class SogScan(C.Structure):
    """gsx_sog_scan (include/gsx_hip.h)"""
    _fields_ = [("vmin", C.c_float * 3), ("vmax", C.c_float * 3), ("nonfinite", C.c_uint32), ("reserved", C.c_uint32),
                ("rest_nonzero", C.c_uint64)]


class ProfileLayout(C.Structure):
    """gsx_profile_layout (include/gsx_hip.h): where x y z and f_rest_0..44 sit inside a row, -1 = absent"""
    _fields_ = [("row_bytes", C.c_int64), ("xyz_offset", C.c_int32 * 3), ("rest_offset", C.c_int32 * 45)]


class TableProfile(C.Structure):
    """gsx_table_profile (include/gsx_hip.h)"""
    _fields_ = [("rest_nonzero", C.c_uint64), ("lo", C.c_float * 3), ("hi", C.c_float * 3), ("nan_axes", C.c_uint32), ("n", C.c_int64)]

    def as_dict(self):
        """what a reader's ``profile=`` dict receives: an axis that holds a NaN reports nan for both bounds"""
        nan = float("nan")
        return {"rest_nonzero": int(self.rest_nonzero),
                "lo": tuple(nan if (self.nan_axes >> a) & 1 else float(self.lo[a]) for a in range(3)),
                "hi": tuple(nan if (self.nan_axes >> a) & 1 else float(self.hi[a]) for a in range(3)),
                "nan_axes": int(self.nan_axes), "n": int(self.n)}


class TransformLayout(C.Structure):
    """gsx_transform_layout (include/gsx_hip.h): the parts a scene transform rewrites, where their fields sit inside a row, and
    the numbers -- M = s R, R, t, q_R, the band matrices D1..D3 (row-major float64) and float32 log(s)"""
    _fields_ = [("parts", C.c_uint32), ("rest_m", C.c_int32), ("xyz_offset", C.c_int32 * 3), ("normal_offset", C.c_int32 * 3),
                ("scale_offset", C.c_int32 * 3), ("rot_offset", C.c_int32 * 4), ("rest_offset", C.c_int32 * 45), ("log_scale", C.c_float),
                ("M", C.c_double * 9), ("R", C.c_double * 9), ("t", C.c_double * 3), ("q", C.c_double * 4), ("D1", C.c_double * 9),
                ("D2", C.c_double * 25), ("D3", C.c_double * 49)]


DECIMATE_MAX_MEAN, DECIMATE_MAX_ZERO, DECIMATE_INFO_WORDS = 51, 128, 5   # GSX_DECIMATE_*
DECIMATE_STAGES = ("keys", "order", "heads", "sums", "finish")        # GSX_DECIMATE_STAGES clocks, in gsx_rows_decimate_*_dev's order
DECIMATE_OK, DECIMATE_CELL_RANGE, DECIMATE_BAD_LIST = range(3)


class DecimateLayout(C.Structure):
    """gsx_decimate_layout (include/gsx_hip.h): the voxel size and where the fields of a row sit -- geometry, averaged float32
    fields, colour bytes, zeroed fields"""
    _fields_ = [("voxel_size", C.c_double), ("xyz_offset", C.c_int32 * 3), ("scale_offset", C.c_int32 * 3), ("rot_offset", C.c_int32 * 4),
                ("opacity_offset", C.c_int32), ("n_mean", C.c_int32), ("mean_offset", C.c_int32 * DECIMATE_MAX_MEAN), ("n_u8", C.c_int32),
                ("u8_offset", C.c_int32 * 3), ("n_zero", C.c_int32), ("zero_offset", C.c_int32 * DECIMATE_MAX_ZERO)]


RENDER_INFO_WORDS, RENDER_RECORD_WORDS = 4, 16                          # GSX_RENDER_*
RENDER_STAGES = ("project", "count", "emit", "sort", "ranges", "blend")   # GSX_RENDER_STAGES clocks, in gsx_rows_render_*_dev's order
RENDER_OK, RENDER_TOO_MANY = range(2)
# a record of gsx_rows_render_plan_dev's workspace, one per row (include/gsx_hip.h)
RENDER_RECORD = np.dtype([("u", "<f4"), ("v", "<f4"), ("a", "<f4"), ("b", "<f4"), ("c", "<f4"), ("opac", "<f4"), ("r", "<f4"), ("g", "<f4"),
                          ("bl", "<f4"), ("depth", "<f4"), ("x0", "<i4"), ("x1", "<i4"), ("y0", "<i4"), ("y1", "<i4"), ("visible", "<u4"),
                          ("pad", "<u4")])


class RenderLayout(C.Structure):
    """gsx_render_layout (include/gsx_hip.h): where the fields the rasteriser reads sit inside a row, the SH degree, the image
    size, the camera and the background"""
    _fields_ = [("xyz_offset", C.c_int32 * 3), ("scale_offset", C.c_int32 * 3), ("rot_offset", C.c_int32 * 4), ("opacity_offset", C.c_int32),
                ("dc_offset", C.c_int32 * 3), ("rgb_offset", C.c_int32 * 3), ("degree", C.c_int32), ("rest_m", C.c_int32),
                ("rest_offset", C.c_int32 * 45), ("width", C.c_int32), ("height", C.c_int32), ("view", C.c_double * 12),
                ("eye", C.c_double * 3), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("tan_fovx", C.c_double), ("tan_fovy", C.c_double), ("near", C.c_double), ("background", C.c_float * 3)]


FIDELITY_WORDS, FIDELITY_TILE, FIDELITY_MAX_SIDE = 9, 32, 8192            # GSX_FIDELITY_*

DENSITY_OK, DENSITY_EMPTY, DENSITY_HOST = range(3)
DENSITY_STAGES = ("table", "init", "hook", "flatten", "reduce", "membership")   # GSX_DENSITY_STAGES
SLAB_OK, SLAB_EMPTY, SLAB_NONFINITE, SLAB_SMALL_SHARD, SLAB_NO_STRUCTURE = range(5)
COMM_F32_MAX, COMM_F32_SUM, COMM_I64_SUM, COMM_F64_MAX, COMM_I64_MIN = range(5)

# name -> (restype, argtypes); every symbol include/gsx_hip.h declares
_P, _I64, _I, _D = C.c_void_p, C.c_int64, C.c_int, C.c_double
SIGNATURES = {
    "gsx_version": (C.c_char_p, []),
    "gsx_last_error": (C.c_char_p, []),
    "gsx_device_count": (_I, []),
    "gsx_device_uid": (_I, [_I, C.c_char_p, _I]),
    "gsx_ctx_create": (_I, [_I, C.POINTER(_P)]),
    "gsx_ctx_destroy": (None, [_P]),
    "gsx_ctx_set_stream": (_I, [_P, _P]),
    "gsx_ctx_own_stream": (_I, [_P]),
    "gsx_ctx_last_knn_algo": (_I, [_P]),
    "gsx_ctx_synchronize": (_I, [_P]),
    "gsx_ctx_check": (_I, [_P]),
    "gsx_ctx_set_timing": (_I, [_P, _I]),
    "gsx_ctx_reset_timing": (_I, [_P]),
    "gsx_ctx_get_timing": (_I, [_P, _I, C.POINTER(C.c_uint64), C.POINTER(_D)]),
    "gsx_ctx_set_param": (_I, [_P, C.c_char_p, _D]),
    "gsx_dev_malloc": (_I, [_P, C.c_size_t, C.POINTER(_P)]),
    "gsx_dev_free": (_I, [_P, _P]),
    "gsx_dev_upload": (_I, [_P, _P, _P, C.c_size_t]),
    "gsx_dev_download": (_I, [_P, _P, _P, C.c_size_t]),
    "gsx_dev_copy": (_I, [_P, _P, _P, C.c_size_t]),
    "gsx_dev_upload_async": (_I, [_P, _P, _P, C.c_size_t]),
    "gsx_dev_memset": (_I, [_P, _P, _I, C.c_size_t]),
    "gsx_fields_nonzero_dev": (_I, [_P, _P, _I64, _I64, _I, C.POINTER(C.c_uint64)]),
    "gsx_rows_repack_dev": (_I, [_P, _P, _I64, _I64, _P, _I64]),
    "gsx_host_pinned_alloc": (_I, [_P, C.c_size_t, C.POINTER(C.c_void_p)]),
    "gsx_host_pinned_free": (_I, [_P, _P]),
    "gsx_dev_upload_staged": (_I, [_P, _P, _P, C.c_size_t]),
    "gsx_dev_download_staged": (_I, [_P, _P, _P, C.c_size_t]),
    "gsx_host_gather_f32": (_I, [_P, _I64, _I64, C.POINTER(_I64), _I, _P]),
    "gsx_host_gather_columns_f32": (_I, [_P, _I64, _I64, C.POINTER(_I64), _I, _P]),
    "gsx_host_compact_rows": (_I, [_P, _I64, _I64, _P, _P, _I64, C.POINTER(_I64)]),
    "gsx_host_take_rows": (_I, [_P, _I64, _I64, _P, _I64, _P]),
    "gsx_host_zero_columns": (_I, [_P, _I64, _I64, C.POINTER(_I64), _I]),
    "gsx_host_append_columns": (_I, [_P, _I64, _I64, _P, _I64, _P, _I64]),
    "gsx_host_take_rows_append": (_I, [_P, _I64, _I64, _P, _I64, _P, _I64, _P, _I64]),
    "gsx_host_take_rows_shape": (_I, [_P, _I64, _I64, _P, _I64, _P, _I64, C.POINTER(_I64), _I, _P, _I64]),
    "gsx_rgb_from_sh": (_I, [_P, _I64, _P, _P]),
    "gsx_rgb_from_sh_dev": (_I, [_P, _P, _I64, _P, _P]),
    "gsx_rgb_from_sh_list": (_I, [_P, _I64, _P, _P, _I64, C.POINTER(_I64)]),
    "gsx_rgb_from_sh_list_dev": (_I, [_P, _P, _I64, _P, _P, _I64, _P]),
    "gsx_compact_rows_dev": (_I, [_P, _P, _P, _P, _I64, _P, _P, C.POINTER(_I64)]),
    "gsx_mask_bbox_dev": (_I, [_P, _P, _I64, _P, _P]),
    "gsx_mask_ge_dev": (_I, [_P, _P, _P, _I64, _D, _P]),
    "gsx_sor_knn_dev": (_I, [_P, _P, _P, _P, _I64, _I64, _I64, _I64, _I, _I, _P, C.POINTER(SorInfo)]),
    "gsx_sor_knn_share_dev": (_I, [_P, _P, _P, _P, _I64, _I64, _I, _I, _I, _I, _P, C.POINTER(SorInfo)]),
    "gsx_sor_debug_brick_plan": (_I, [_P, _P, _P, _P, _I64]),
    "gsx_sor_debug_work_queue": (_I, [_P, _P, _P, _P]),
    "gsx_sor_debug_tree": (_I, [_P, _P, _P, _P, _I64, C.POINTER(_I64), C.POINTER(_I64)]),
    "gsx_sor_debug_wave_stamps": (_I, [_P, _I, _P, _I64, _P]),
    "gsx_sor_debug_points_per_cell": (_D, [_I, _I64, _I]),
    "gsx_sor_debug_group_bricks": (_I, [_P, _I64, _I, _I, _I, _P, C.POINTER(C.c_int32)]),
    "gsx_sor_debug_refine_sizing": (_I, [C.POINTER(RefineSizingIn), C.POINTER(RefineSizingOut)]),
    "gsx_knn_probe_root_dev": (_I, [_P, _P, _I64, _I, _P]),
    "gsx_knn_probe_root_short_dev": (_I, [_P, _P, _I64, _I, _P]),
    "gsx_knn_probe_mean_dev": (_I, [_P, _P, _I64, _I64, _I, _I, _I, _P]),
    "gsx_sor_stats_dev": (_I, [_P, _P, _I64, _D, _P]),
    "gsx_sor_mask_dev": (_I, [_P, _P, _I64, _P, _P]),
    "gsx_comm_unique_id": (_I, [_P]),
    "gsx_comm_init": (_I, [_P, _I, _I, _P]),
    "gsx_comm_destroy": (_I, [_P]),
    "gsx_comm_all_reduce": (_I, [_P, _P, _I64, _I]),
    "gsx_comm_all_gather": (_I, [_P, _P, _P, _I64]),
    "gsx_comm_all_to_all_v": (_I, [_P, _P, _P, _P, _P, _P, _P, _I]),
    "gsx_comm_all_to_all_segs": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _I]),
    "gsx_comm_abort": (_I, [_P]),
    "gsx_comm_transport": (_I, [_P]),
    "gsx_comm_rank": (_I, [_P, C.POINTER(_I), C.POINTER(_I)]),
    "gsx_comm_barrier": (_I, [_P]),
    "gsx_slab_plan": (_I, [_P, _I, _I, _I64, _I, _D, C.POINTER(SlabPlan)]),
    "gsx_sor_slab_step_dev": (_I, [_P, _P, _I64, _I, _D, _D, _P, C.POINTER(SlabStep)]),
    "gsx_slab_bbox_dev": (_I, [_P, _P, _P, _P, _I64, _I64, _P]),
    "gsx_slab_hist_dev": (_I, [_P, _P, _P, _P, _I64, _I64, _P, _P]),
    "gsx_slab_partition_dev": (_I, [_P, _P, _P, _P, _I64, _I64, _I, _I, C.c_float, C.c_float, _P, _I, _P, _P, _P, _P, _P]),
    "gsx_sor_knn_slab_dev": (_I, [_P, _P, _I64, _I64, _I, _P, _P]),
    "gsx_slab_certify_dev": (_I, [_P, _P, _I64, _I64, _P, C.c_float, C.c_float, _P]),
    "gsx_slab_unpermute_dev": (_I, [_P, _P, _P, _I64, _P]),
    "gsx_sor_piece_sums_dev": (_I, [_P, _P, _I64, _P, _P]),
    "gsx_sor_stats_from_pieces_dev": (_I, [_P, _P, _I64, _I64, _I, _D, _P]),
    "gsx_sor_filter": (_I, [_P, _P, _P, _I64, _I64, _I, _D, _I, _P, _P, _P, C.POINTER(SorInfo)]),
    "gsx_density_voxels": (_I, [_P, _P, _P, _I64, _I64, _D, _I64, _I64, C.POINTER(_I64), C.POINTER(_I64), _P, _P]),
    "gsx_density_mask": (_I, [_P, _P, _P, _I64, _I64, _D, _P, _I64, _P]),
    "gsx_kmeans_lloyd": (_I, [_P, _I64, _I, _I, _I, _P, _P, _P]),
    "gsx_quantize_sorted_codebook": (_I, [_P, _I64, _P, _I, _P]),
    "gsx_kmeans_pp": (_I, [_P, _I64, _I, _I, _P, _I, _P]),
    "gsx_kmeans_pp_dev": (_I, [_P, _P, _I64, _I, _I, _P, _I, _P]),
    "gsx_kmeans1d": (_I, [_P, _I64, _I, _I, _P, _P, _P]),
    "gsx_kmeans1d_dev": (_I, [_P, _P, _I64, _I, _I, _I, _P, _P, _P]),
    "gsx_lexsort3": (_I, [_P, _P, _P, _I64, _P]),
    "gsx_lexsort3_dev": (_I, [_P, _P, _P, _P, _I64, _I64, _P]),
    "gsx_sog_quats": (_I, [_P, _I64, _P]),
    "gsx_sog_positions": (_I, [_P, _I64, C.c_float, C.c_float, _P, _P]),
    "gsx_sog_positions_dev": (_I, [_P, _P, _I64, C.c_float, C.c_float, _P, _P]),
    "gsx_sog_alpha": (_I, [_P, _I64, _P, _P]),
    "gsx_sog_alpha_dev": (_I, [_P, _P, _I64, _P, _P]),
    "gsx_sog_quats_dev": (_I, [_P, _P, _I64, _P]),
    "gsx_sog_scan_dev": (_I, [_P, _P, C.POINTER(SogLayout), _I64, _P, C.POINTER(SogScan)]),
    "gsx_sog_extremes_dev": (_I, [_P, _P, _I64, _P, _P, _I, _P, _P]),
    "gsx_sog_order_dev": (_I, [_P, _P, _I64, _P]),
    "gsx_sog_gather_dev": (_I, [_P, _P, C.POINTER(SogLayout), _P, _I64, _I, _P, _P, _P, _P, _P, _P]),
    "gsx_sog_means_texels_dev": (_I, [_P, _P, _I64, _I64, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "gsx_sog_quats_texels_dev": (_I, [_P, _P, _I64, _I64, _P]),
    "gsx_sog_codes_texels_dev": (_I, [_P, _P, _I64, _I64, _P, _I, _P, _P, _P, _I64, _P]),
    "gsx_sog_labels_texels_dev": (_I, [_P, _P, _I64, _I64, _I64, _I, _P]),
    "gsx_gather_rows_dev": (_I, [_P, _P, _I, _P, _I64, _P]),
    "gsx_morton_order_dev": (_I, [_P, _P, _P, _P, _I64, _I64, _P, C.POINTER(_I)]),
    "gsx_cply_pack_dev": (_I, [_P, _P, _P, _I64, _P, _P]),
    "gsx_cply_sh_dev": (_I, [_P, _P, _I, _I64, _P, _I64, _P]),
    "gsx_cply_pack_strided_dev": (_I, [_P, _P, _P, _P, _I64, _P, _P]),
    "gsx_cply_pack_opacity_dev": (_I, [_P, _P, _P, _P, _I64, _P, _P, _P, _I64, _P]),
    "gsx_cply_sh_strided_dev": (_I, [_P, _P, _I, _I64, _I64, _P, _I64, _P]),
    "gsx_density_voxels_dev": (_I, [_P, _P, _P, _P, _I64, _I64, _D, _I64, _I64, C.POINTER(_I64), C.POINTER(_I64), _P, _P]),
    "gsx_density_mask_dev": (_I, [_P, _P, _P, _P, _I64, _I64, _D, _P, _I64, _P]),
    "gsx_density_filter_dev": (_I, [_P, _P, _P, _P, _I64, _I64, _D, _I64, _I, _P, _P, C.POINTER(DensityInfo)]),
    "gsx_density_filter_large_dev": (_I, [_P, _P, _P, _P, _I64, _I64, _D, _I64, _I, _P, _P, C.POINTER(DensityInfo)]),
    "gsx_voxel_clusters": (_I, [_P, _I64, _I, _P, C.POINTER(DensityInfo)]),
    "gsx_voxel_clusters_dev": (_I, [_P, _P, _I64, _I, _P, C.POINTER(DensityInfo)]),
    "gsx_density_stage_clocks": (_I, [_P, C.POINTER(_D)]),
    "gsx_density_hist_dev": (_I, [_P, _P, _P, _P, _I64, _I64, _D, _I64, C.POINTER(_I64), _P, _P]),
    "gsx_density_merge_dev": (_I, [_P, _P, _P, _I64, _I64, _I64, C.POINTER(_I64), C.POINTER(_I64), _P, _P]),
    "gsx_kmeans_lloyd_dev": (_I, [_P, _P, _I64, _I, _I, _I, _P, _P]),
    "gsx_kmeans_lloyd_batch_dev": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "gsx_quantize_sorted_codebook_dev": (_I, [_P, _P, _I64, _P, _I, _P]),
    "gsx_spz_rest_nonzero_dev": (_I, [_P, _P, C.POINTER(SpzLayout), _I64, C.c_uint64, C.POINTER(C.c_uint64)]),
    "gsx_spz_pack_dev": (_I, [_P, _P, C.POINTER(SpzLayout), _I64, _I, _P, _P, _I64, _P]),
    "gsx_ksplat_centres_dev": (_I, [_P, _P, C.POINTER(SpzLayout), _I64, _I64, _P, _P, _I64, _P]),
    "gsx_ksplat_pack_dev": (_I, [_P, _P, C.POINTER(SpzLayout), _I64, _I, _I, _I64, C.c_float, _P, _P, _I64, _P, _I64, _P]),
    "gsx_ksplat_math_dev": (_I, [_P, _P, _I64, _P, _P]),
    "gsx_np_expf_host": (_I, [_P, _P, _I64]),
    "gsx_splat_pack_dev": (_I, [_P, _P, C.POINTER(SpzLayout), _I, _I, _I, _I64, _P, _P, _P]),
    "gsx_splat_keys_dev": (_I, [_P, _P, _I64, _P]),
    "gsx_splat_order_dev": (_I, [_P, _P, _I64, _P]),
    "gsx_splat_permute_dev": (_I, [_P, _P, _P, _I64, _P]),
    "gsx_cply_unpack_dev": (_I, [_P, _P, _I64, _P, _I64, _P, C.POINTER(CplyReadLayout), _P, _P]),
    "gsx_ksplat_unpack_dev": (_I, [_P, _P, _I64, _I, C.POINTER(KsplatReadSection), _I, _P, _I64, _P, _I, _P, _I64]),
    "gsx_spz_unpack_dev": (_I, [_P, _P, _I64, _I, _I, _I, _P, _P, _I64]),
    "gsx_sog_unpack_dev": (_I, [_P, _P, _I64, C.POINTER(_I64), _I, _I64, _P, _P, _I64, _P]),
    "gsx_splat_unpack_dev": (_I, [_P, _P, _I64, _P, _P]),
    "gsx_np_log_math_dev": (_I, [_P, _P, _I64, _P]),
    "gsx_np_logf_host": (_I, [_P, _P, _I64]),
    "gsx_ply_unpack_dev": (_I, [_P, _P, _I64, _I64, C.POINTER(PlyReadLayout), _P]),
    "gsx_ply_unpack_host": (_I, [_P, _I64, C.POINTER(PlyReadLayout), _P]),
    "gsx_ply_text_padded_bytes": (_I64, [_I64]),
    "gsx_ply_text_work_bytes": (_I64, [_I64]),
    "gsx_ply_text_scan_dev": (_I, [_P, _P, _I64, _P, _I64]),
    "gsx_ply_text_parse_dev": (_I, [_P, _P, _I64, _I64, C.POINTER(PlyTextLayout), _P, _P, _I64, _P, _I64, C.POINTER(_I64)]),
    "gsx_ply_text_host": (_I, [_P, _I64, _I64, C.POINTER(PlyTextLayout), _P, _P, _I64, C.POINTER(_I64)]),
    "gsx_dec_to_f64": (_I, [_P, C.c_int32, C.POINTER(C.c_uint64)]),
    "gsx_dec_pow5_entry": (_I, [C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),
    "gsx_ply_pack_dev": (_I, [_P, _P, _I64, C.POINTER(PlyWriteLayout), _P]),
    "gsx_ply_pack_host": (_I, [_P, _I64, C.POINTER(PlyWriteLayout), _P]),
    "gsx_ply_rest_nonzero_dev": (_I, [_P, _P, _I64, _I64, C.POINTER(C.c_int32), C.c_uint64, C.POINTER(C.c_uint64)]),
    "gsx_parquet_rows_dev": (_I, [_P, _P, _I64, _I64, C.POINTER(ParquetRowsLayout), _P]),
    "gsx_parquet_rows_host": (_I, [_P, _I64, _I64, C.POINTER(ParquetRowsLayout), _P]),
    "gsx_parquet_columns_dev": (_I, [_P, _P, _I64, C.POINTER(ParquetColumnsLayout), _P, _I64, _P]),
    "gsx_parquet_columns_host": (_I, [_P, _I64, C.POINTER(ParquetColumnsLayout), _P, _I64, _P]),
    "gsx_table_profile_dev": (_I, [_P, _P, _I64, _I64, C.POINTER(ProfileLayout), C.POINTER(TableProfile)]),
    "gsx_table_profile_host": (_I, [_P, _I64, C.POINTER(ProfileLayout), _I, C.POINTER(TableProfile)]),
    "gsx_rows_columns_f32_dev": (_I, [_P, _P, _I64, _I64, _I64, C.POINTER(C.c_int32), _I, _P]),
    "gsx_rows_take_dev": (_I, [_P, _P, _I64, _I64, _I64, _P, _I64, C.POINTER(C.c_int32), _I, _P, _I, _P, _I64]),
    "gsx_rows_transform_dev": (_I, [_P, _P, _I64, _I64, _I64, C.POINTER(TransformLayout), _P]),
    "gsx_rows_transform_host": (_I, [_P, _I64, _I64, C.POINTER(TransformLayout), _P]),
    "gsx_rows_remap_dev": (_I, [_P, _P, _I64, _I64, _I64, C.POINTER(C.c_int32), _I, _P, _I64, _I64, _I64, _I64]),
    "gsx_rows_remap_host": (_I, [_P, _I64, _I64, _I64, C.POINTER(C.c_int32), _I, _P, _I64, _I64, _I64, _I64]),
    "gsx_dev_patch_u8": (_I, [_P, _P, _I64, _P, _P, _I64]),
    "gsx_limit_keys_dev": (_I, [_P, _P, _I64, _P]),
    "gsx_limit_select_dev": (_I, [_P, _P, _P, _I64, _I64, _P, _P]),
    "gsx_limit_select_host": (_I, [_P, _P, _I64, _I64, _P, _P]),
    "gsx_rows_decimate_work_dev": (_I, [_P, _I64, C.POINTER(_I64)]),
    "gsx_rows_decimate_plan_dev": (_I, [_P, _P, _I64, _I64, _I64, _P, _I64, C.POINTER(DecimateLayout), _P, _I64, C.POINTER(_I64),
                                        C.POINTER(C.c_float)]),
    "gsx_rows_decimate_write_dev": (_I, [_P, _P, _I64, _I64, _I64, _P, _I64, C.POINTER(DecimateLayout), _P, _I64, _P, _I64, _I64,
                                         C.POINTER(C.c_float)]),
    "gsx_rows_render_work_dev": (_I, [_P, _I64, C.c_int32, C.c_int32, C.POINTER(_I64)]),
    "gsx_rows_render_plan_dev": (_I, [_P, _P, _I64, _I64, _I64, C.POINTER(RenderLayout), _P, _I64, C.POINTER(_I64), C.POINTER(C.c_float)]),
    "gsx_rows_render_draw_dev": (_I, [_P, _I64, C.POINTER(RenderLayout), _P, _I64, _P, _I64, _P, C.POINTER(C.c_float)]),
    "gsx_rows_render_score_dev": (_I, [_P, _I64, C.POINTER(RenderLayout), _P, _I64, _P, _I64, _P, _P, C.POINTER(C.c_float)]),
    "gsx_image_compare_dev": (_I, [_P, _P, _P, C.c_int32, C.c_int32, C.POINTER(_I64), C.POINTER(C.c_float)]),
    "gsx_image_compare_host": (_I, [_P, _P, C.c_int32, C.c_int32, C.POINTER(_I64)]),
    "gsx_view_keys_dev": (_I, [_P, _P, _I64, _P]),
    "gsx_view_keys_host": (_I, [_P, _I64, _P]),
}

_lib = None


def load() -> C.CDLL:
    """dlopen the in-tree library and bind every declared symbol (raises GsxError if absent)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GsxError("libgsx_hip.so is not built: run `python 3dgsconverter_amd/build.py` "
                       "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # e.g. libamdhip64 missing
        raise GsxError("cannot load %s: %s" % (LIB_PATH, e)) from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise GsxError("libgsx_hip.so does not export %s (stale build?)" % name) from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error() -> str:
    return (load().gsx_last_error() or b"").decode("utf-8", "replace")


def check(rc: int, what: str):
    if rc != 0:
        raise GsxError("%s failed: %s" % (what, last_error()))


def device_count() -> int:
    try:
        return int(load().gsx_device_count())
    except GsxError:
        return 0


def device_uid(device: int) -> str:
    """PCI bus id of a visible device: equal strings <=> the same physical GPU"""
    buf = C.create_string_buffer(64)
    check(load().gsx_device_uid(device, buf, 64), "gsx_device_uid")
    return buf.value.decode()


def has_hip() -> bool:
    return device_count() > 0


def require_hip():
    lib = load()
    if lib.gsx_device_count() <= 0:
        raise GsxError("no MI355X (gfx950) device visible to HIP; the HIP path has no CPU fallback")
    return lib


def _xyz_pointers(xyz_or_cols):
    """Accept an (N,3) float32 C-contiguous array (the reference's `coords`, data_processor.py:139)
    or a tuple of three contiguous float32 columns. -> (keepalive, px, py, pz, stride, n)"""
    if isinstance(xyz_or_cols, (tuple, list)):
        cols = [np.ascontiguousarray(c, dtype=np.float32) for c in xyz_or_cols]
        if len(cols) != 3 or len({len(c) for c in cols}) != 1:
            raise ValueError("expected three equally long columns")
        return cols, cols[0].ctypes.data, cols[1].ctypes.data, cols[2].ctypes.data, 1, len(cols[0])
    a = np.ascontiguousarray(xyz_or_cols, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("Requires 3D data")  # same message as gpu_ops.py:198
    base = a.ctypes.data
    return a, base, base + 4, base + 8, 3, a.shape[0]


def is_f4(dt: np.dtype) -> bool:
    """a float32 field of either byte order: its float32 copy is the same numbers"""
    return dt.kind == "f" and dt.itemsize == 4


def f32_inexact_field(vertices: np.ndarray, names):
    """The first field of `names` (those the table has) whose values float32 does not hold exactly -> (name, dtype), or None.
    float32 fields of either byte order and float16 fields hold float32 values by their dtype; a float64 field is checked value
    by value (one host pass: back from float32 it must be the column again, NaN for NaN).  Any other dtype counts as inexact."""
    fields = vertices.dtype.fields or {}
    for nm in names:
        if nm not in fields:
            continue
        dt = fields[nm][0]
        if dt.kind == "f" and dt.itemsize in (2, 4):
            continue
        if dt.kind == "f" and dt.itemsize == 8:
            col = vertices[nm]
            with np.errstate(over="ignore", invalid="ignore"):
                if np.array_equal(col.astype(np.float32).astype(np.float64), col, equal_nan=True):
                    continue
        return nm, dt
    return None


def require_f4_fields(data: np.ndarray, names, who: str):
    """TypeError naming the first field of `names` (those the table has) that is not float32: a writer whose arithmetic the
    reference does in the table's own dtype refuses other dtypes instead of casting them"""
    fields = data.dtype.fields or {}
    for nm in names:
        if nm in fields and not is_f4(fields[nm][0]):
            raise TypeError(f"{who}: field {nm!r} is {fields[nm][0].str}; the GPU writer computes in float32 as the reference does for "
                            f"float32 fields, and takes float32 ('<f4' or '>f4') fields only")


def native_f4(data: np.ndarray, names) -> np.ndarray:
    """`data` with its big-endian float32 fields among `names` made little-endian (a new table, same layout, same numbers), or
    `data` itself when it has none"""
    fields = data.dtype.fields or {}
    flip = [nm for nm in names if nm in fields and fields[nm][0] == np.dtype(">f4")]
    if not flip:
        return data
    dt = np.dtype({"names": list(data.dtype.names),
                   "formats": [np.dtype("<f4") if nm in flip else fields[nm][0] for nm in data.dtype.names],
                   "offsets": [fields[nm][1] for nm in data.dtype.names], "itemsize": data.dtype.itemsize})
    return np.ascontiguousarray(data.astype(dt))


def host_gather_xyz(vertices: np.ndarray, names=("x", "y", "z"), out: "np.ndarray | None" = None, exact: bool = True) -> np.ndarray:
    """coords = np.column_stack((v['x'], v['y'], v['z'])) (data_processor.py:38,139) as float32 (N,3),
    threaded (C ABI gsx_host_gather_f32).  Any layout the C routine cannot take goes through numpy.  out: a C-contiguous
    (N, len(names)) float32 array to fill (a pinned staging buffer).  exact: a field whose values float32 does not hold raises
    TypeError (f32_inexact_field); False = cast it (DeviceChain: the caller decides where the copy may stand in for the table)"""
    fields = vertices.dtype.fields or {}
    ok = (vertices.ndim == 1 and vertices.flags.c_contiguous and
          all(nm in fields and fields[nm][0] == np.dtype("<f4") for nm in names))
    if not ok:
        bad = f32_inexact_field(vertices, names) if exact else None
        if bad is not None:
            raise TypeError(f"field {bad[0]!r} is {bad[1].str} and holds values float32 does not; the device computes on float32 "
                            f"coordinates")
        res = np.column_stack([np.asarray(vertices[nm], dtype=np.float32) for nm in names])
        if out is not None:
            out[...] = res
            return out
        return res
    n = len(vertices)
    if out is None:
        out = np.empty((n, len(names)), dtype=np.float32)
    elif out.shape != (n, len(names)) or out.dtype != np.float32 or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous (n, %d) float32 array" % len(names))
    if n == 0:
        return out
    offs = (_I64 * len(names))(*[int(fields[nm][1]) for nm in names])
    check(load().gsx_host_gather_f32(vertices.ctypes.data, vertices.dtype.itemsize, n, offs, len(names), out.ctypes.data),
          "gsx_host_gather_f32")
    return out


def host_gather_columns(vertices: np.ndarray, names) -> np.ndarray:
    """(len(names), n) float32, row c = np.ascontiguousarray(vertices[names[c]]): every column a writer uploads, in ONE threaded
    pass over the table (C ABI gsx_host_gather_columns_f32) instead of one strided numpy copy per column"""
    names = list(names)
    fields = vertices.dtype.fields or {}
    n = len(vertices)
    ok = (vertices.ndim == 1 and vertices.flags.c_contiguous and 1 <= len(names) <= 64 and
          all(nm in fields and fields[nm][0] == np.dtype("<f4") for nm in names))
    if not ok or n == 0:
        out = np.empty((len(names), n), dtype=np.float32)
        for i, nm in enumerate(names):
            out[i] = vertices[nm]
        return out
    out = np.empty((len(names), n), dtype=np.float32)
    offs = (_I64 * len(names))(*[int(fields[nm][1]) for nm in names])
    check(load().gsx_host_gather_columns_f32(vertices.ctypes.data, vertices.dtype.itemsize, n, offs, len(names), out.ctypes.data),
          "gsx_host_gather_columns_f32")
    return out


SPZ_HEADER_BYTES = 16   # <IIIBBBB: magic, version, n, SH degree, fractional bits, flags, reserved (spz.py:95-97)
SPZ_SH_DIM = {0: 0, 1: 3, 2: 8, 3: 15}   # spz.py _dim_for_degree


def spz_layout(dtype: np.dtype) -> SpzLayout:
    """gsx_spz_layout of a structured dtype: byte offsets of the fields in SOG_FIELD_NAMES' order, -1 where absent"""
    fields = dtype.fields or {}
    lay = SpzLayout()
    lay.row_bytes = dtype.itemsize
    for i, nm in enumerate(SOG_FIELD_NAMES):
        lay.offset[i] = int(fields[nm][1]) if nm in fields else -1
    return lay


def spz_alpha_bytes(opacity: np.ndarray) -> np.ndarray:
    """spz.py:121 with numpy's own float32 exp, for the rows the device lists"""
    with np.errstate(all="ignore"):
        return (1.0 / (1.0 + np.exp(-np.clip(opacity, -20, 20))) * 255.0).astype(np.uint8)


def spz_patch_rotations(rot: np.ndarray, rows: np.ndarray, quats: np.ndarray) -> None:
    """spz.py:298-343 for the rows the device lists (a component other than the largest is NaN).  rot: the body's n packed
    words, the other rows already final; quats: (len(rows), 4) float32 rot_0..3 of the listed rows.

    The reference quantises component j of every row whose largest component is not j in ONE array, and numpy's float32 ->
    uint32 cast of a NaN gives a value that depends on the position in that array (vector lanes and scalar remainder
    differ).  The position comes from the largest-component index of every row (bits 30-31 of the words), the value from
    numpy's own cast of a NaN array of that length."""
    rows = np.asarray(rows, dtype=np.int64)
    w, x, y, z = (np.ascontiguousarray(quats[:, c], dtype=np.float32) for c in range(4))
    with np.errstate(all="ignore"):
        norm = np.sqrt(w * w + x * x + y * y + z * z + 1e-9)
        r = np.column_stack((x / norm, y / norm, z / norm, w / norm))
    mi = np.argmax(np.abs(r), axis=1)
    mi_all = rot >> np.uint32(30)
    mi_all[rows] = mi
    should_neg = r[np.arange(len(rows)), mi] < 0
    packed = mi.astype(np.uint32) << np.uint32(30)
    scale = 511.0 / 0.707106781186547524401
    for j in range(4):
        m = mi != j
        if not np.any(m):
            continue
        val = r[m, j]
        with np.errstate(all="ignore"):
            mag_f = np.clip(np.abs(val) * scale + 0.5, 0, 511)
            mag = mag_f.astype(np.uint32)
        nan = np.isnan(mag_f)
        if np.any(nan):
            ne = mi_all != j
            pos = np.cumsum(ne, dtype=np.int64)[rows[m][nan]] - 1
            with np.errstate(all="ignore"):
                probe = np.full(int(np.count_nonzero(ne)), np.nan, np.float32).astype(np.uint32)
            mag[nan] = probe[pos]
        negbit = ((val < 0) != should_neg[m]).astype(np.uint32)
        shift = ((2 - (j - (mi[m] < j))) * 10).astype(np.uint32)
        packed[m] |= ((negbit << np.uint32(9)) | mag) << shift
    rot[rows] = packed


def host_compact_rows(rows: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """rows[mask] (data_processor.py:114,149) for a 1-D array of any (structured) dtype, threaded
    (C ABI gsx_host_compact_rows).  Same result as numpy's boolean indexing: a new array, order kept."""
    mask = np.asarray(mask)
    if rows.ndim != 1 or mask.shape != rows.shape or mask.dtype != np.bool_ or rows.dtype.hasobject:
        return rows[mask]
    src = np.ascontiguousarray(rows)
    m8 = np.ascontiguousarray(mask).view(np.uint8)
    keep = int(np.count_nonzero(m8))
    out = np.empty(keep, dtype=rows.dtype)
    n_out = _I64()
    if len(src):
        check(load().gsx_host_compact_rows(src.ctypes.data, src.dtype.itemsize, len(src), m8.ctypes.data, out.ctypes.data,
                                           keep, C.byref(n_out)), "gsx_host_compact_rows")
        assert n_out.value == keep
    return out


def host_take_rows(rows: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """rows[idx] for a strictly ascending uint32 index list (the device chain's survivor list) == rows[mask], threaded
    (C ABI gsx_host_take_rows): a new array, order kept, no boolean mask in between"""
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    if rows.ndim != 1 or rows.dtype.hasobject:
        return rows[idx]
    src = np.ascontiguousarray(rows)
    out = np.empty(len(idx), dtype=rows.dtype)
    if len(idx):
        check(load().gsx_host_take_rows(src.ctypes.data, src.dtype.itemsize, len(src), idx.ctypes.data, len(idx), out.ctypes.data),
              "gsx_host_take_rows")
    return out


def host_zero_columns(rows: np.ndarray, names) -> None:
    """rows[name] = 0.0 for every float32 field in `names`, in place (data_processor.py:310-313), one threaded pass"""
    fields = rows.dtype.fields or {}
    names = [nm for nm in names if nm in fields]
    if not names or len(rows) == 0:
        return
    ok = rows.ndim == 1 and rows.flags.c_contiguous and rows.flags.writeable and all(fields[nm][0].itemsize == 4 for nm in names)
    if not ok:
        for nm in names:
            rows[nm] = 0.0
        return
    offs = (_I64 * len(names))(*[int(fields[nm][1]) for nm in names])
    check(load().gsx_host_zero_columns(rows.ctypes.data, rows.dtype.itemsize, len(rows), offs, len(names)), "gsx_host_zero_columns")


def host_append_u8_columns(rows: np.ndarray, names, columns: np.ndarray) -> np.ndarray:
    """a new structured array = every field of `rows` + the u1 fields `names` filled from columns (n, len(names)) uint8
    (data_processor.py:262-274), one threaded pass over the rows"""
    new_dtype = np.dtype(rows.dtype.descr + [(nm, "u1") for nm in names])
    cols = np.ascontiguousarray(columns, dtype=np.uint8).reshape(len(rows), len(names))
    out = np.empty(len(rows), dtype=new_dtype)
    tail_ok = all(new_dtype.fields[nm][1] == rows.dtype.itemsize + i for i, nm in enumerate(names))
    if rows.ndim != 1 or not rows.flags.c_contiguous or rows.dtype.hasobject or not tail_ok or len(rows) == 0:
        for nm in rows.dtype.names:
            out[nm] = rows[nm]
        for i, nm in enumerate(names):
            out[nm] = cols[:, i]
        return out
    check(load().gsx_host_append_columns(rows.ctypes.data, rows.dtype.itemsize, len(rows), cols.ctypes.data, len(names),
                                         out.ctypes.data, new_dtype.itemsize), "gsx_host_append_columns")
    return out


def host_take_rows_shape(rows: np.ndarray, idx: np.ndarray, names=(), columns: "np.ndarray | None" = None, zero_names=()) -> np.ndarray:
    """rows[idx] with the float32 fields `zero_names` set to 0.0 and, when `names` / `columns` are given, the u1 fields `names`
    appended from columns[idx] -- compaction, cap_sh_degree and add_rgb_from_sh (data_processor.py:114,149 / :310-313 / :262-274) in
    ONE threaded pass (C ABI gsx_host_take_rows_shape)"""
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    names = tuple(names)
    fields = rows.dtype.fields or {}
    zero_names = [nm for nm in zero_names if nm in fields]
    new_dtype = np.dtype(rows.dtype.descr + [(nm, "u1") for nm in names]) if names else rows.dtype
    tail_ok = all(new_dtype.fields[nm][1] == rows.dtype.itemsize + i for i, nm in enumerate(names))
    plain = (rows.ndim == 1 and rows.flags.c_contiguous and not rows.dtype.hasobject and tail_ok
             and all(fields[nm][0].itemsize == 4 for nm in zero_names))
    if not plain:
        out = host_take_rows_append_u8(rows, idx, names, columns) if names else host_take_rows(rows, idx)
        host_zero_columns(out, zero_names)
        return out
    cols = np.ascontiguousarray(columns, dtype=np.uint8).reshape(len(rows), len(names)) if names else None
    out = np.empty(len(idx), dtype=new_dtype)
    if len(idx):
        offs = (_I64 * max(len(zero_names), 1))(*[int(fields[nm][1]) for nm in zero_names])
        check(load().gsx_host_take_rows_shape(rows.ctypes.data, rows.dtype.itemsize, len(rows), idx.ctypes.data, len(idx),
                                              cols.ctypes.data if names else None, len(names), offs, len(zero_names), out.ctypes.data,
                                              new_dtype.itemsize), "gsx_host_take_rows_shape")
    return out


def host_take_rows_append_u8(rows: np.ndarray, idx: np.ndarray, names, columns: np.ndarray) -> np.ndarray:
    """host_append_u8_columns(host_take_rows(rows, idx), names, columns[idx]) in ONE threaded pass (C ABI gsx_host_take_rows_append):
    the filters' compaction and add_rgb_from_sh's widened copy (data_processor.py:114,149 + :262-274) without the table in between.
    columns: (len(rows), len(names)) uint8, indexed like `rows`"""
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    new_dtype = np.dtype(rows.dtype.descr + [(nm, "u1") for nm in names])
    cols = np.ascontiguousarray(columns, dtype=np.uint8).reshape(len(rows), len(names))
    tail_ok = all(new_dtype.fields[nm][1] == rows.dtype.itemsize + i for i, nm in enumerate(names))
    if rows.ndim != 1 or not rows.flags.c_contiguous or rows.dtype.hasobject or not tail_ok:
        return host_append_u8_columns(host_take_rows(rows, idx), names, cols[idx])
    out = np.empty(len(idx), dtype=new_dtype)
    if len(idx):
        check(load().gsx_host_take_rows_append(rows.ctypes.data, rows.dtype.itemsize, len(rows), idx.ctypes.data, len(idx), cols.ctypes.data,
                                               len(names), out.ctypes.data, new_dtype.itemsize), "gsx_host_take_rows_append")
    return out


def nonzero_bytes(flags: np.ndarray) -> np.ndarray:
    """np.flatnonzero of a SPARSE uint8 flag array, eight flags per look (the uncertain-element flags of the certificate kernels:
    a few hundred set bytes in 30M; numpy's byte-wise scan takes 5x as long)"""
    flags = np.ascontiguousarray(flags).reshape(-1)
    n = len(flags)
    m = n // 8 if flags.ctypes.data % 8 == 0 else 0
    parts = []
    if m:
        words = np.flatnonzero(flags[:8 * m].view(np.uint64))
        if len(words):
            r, c = np.nonzero(flags[:8 * m].reshape(m, 8)[words])
            parts.append(words[r] * 8 + c)
    tail = np.flatnonzero(flags[8 * m:])
    if len(tail):
        parts.append(tail + 8 * m)
    return np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)


def rgb_from_sh(f_dc: np.ndarray, stats: dict | None = None) -> np.ndarray:
    """one channel of data_processor.py:316-343 -> u8[n], byte-identical to numpy (C ABI gsx_rgb_from_sh: float64 power on
    the GPU + rounding certificate; numpy's own expression for the flagged elements)"""
    lib = require_hip()
    v = np.ascontiguousarray(f_dc, dtype=np.float32)
    n = len(v)
    out = np.empty(n, dtype=np.uint8)
    if n == 0:
        return out
    # the uncertain elements as a compact index list (about 1e-4 of the values); a table with more of them than the list holds (NaNs by
    # the million) takes the flag-per-element form
    cap = n // 64 + 4096
    lst = np.empty(cap, dtype=np.uint32)
    cnt = _I64(0)
    check(lib.gsx_rgb_from_sh_list(v.ctypes.data, n, out.ctypes.data, lst.ctypes.data, cap, C.byref(cnt)), "gsx_rgb_from_sh_list")
    if cnt.value <= cap:
        idx = np.sort(lst[:cnt.value]).astype(np.int64)
    else:
        unc = np.empty(n, dtype=np.uint8)
        check(lib.gsx_rgb_from_sh(v.ctypes.data, n, out.ctypes.data, unc.ctypes.data), "gsx_rgb_from_sh")
        idx = nonzero_bytes(unc)
    if len(idx):
        with np.errstate(all="ignore"):
            lin = np.clip(0.5 + v[idx] * 0.28209479177387814, 0.0, 1.0)
            out[idx] = (np.power(lin, 1.0 / 2.2) * 255).astype(np.uint8)
    if stats is not None:
        stats["uncertain"] = stats.get("uncertain", 0) + int(len(idx))
        stats["n"] = stats.get("n", 0) + n
    return out


_numpy_reduction_checked = None


def numpy_reduction_selfcheck(ctx: "Context | None" = None) -> bool:
    """The SOR threshold is bit-exact only if the device reproduces THIS process's numpy float32 reductions
    (csrc/sor_stats.hip restates numpy 2.2's rule: 8192-element buffer pieces added sequentially, pairwise inside a piece).
    The reference does not pin numpy, so the rule is probed once per process: np.mean / np.std of a 20 001-element
    float32 array with a wide dynamic range against gsx_sor_stats_dev.  A mismatch is reported with a RuntimeWarning (masks
    can then differ from this numpy's for mean distances within one ulp of the threshold) -- or, under GSX_STRICT_NUMPY=1
    (what tests/conftest.py sets), raised as a GsxError; nothing falls back.  Supported: numpy 1.22 ... 2.2 reduce this way."""
    global _numpy_reduction_checked
    if _numpy_reduction_checked is not None:
        return _numpy_reduction_checked
    import warnings
    rng = np.random.default_rng(8192)
    a = (rng.standard_normal(20001) * np.exp(rng.uniform(-6, 6, 20001))).astype(np.float32)
    a = np.abs(a) + np.float32(1e-3)
    own = ctx is None
    ctx = ctx or Context(0)
    try:
        d, st = ctx.alloc(a.nbytes + 16).upload(a), ctx.alloc(16)
        ctx.sor_stats(d.ptr, len(a), 1.5, st.ptr)
        got = st.download(np.float32, 3)
        d.free()
        st.free()
    finally:
        if own:
            ctx.close()
    m, sd = np.mean(a), np.std(a)
    want = np.array([m, sd, m + 1.5 * sd], dtype=np.float32)
    _numpy_reduction_checked = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
    if not _numpy_reduction_checked:
        msg = ("numpy %s reduces float32 arrays in a different order than the one libgsx_hip reproduces (numpy 2.2: 8192-element "
               "pieces, pairwise inside): SOR thresholds would differ from this numpy's in the last bit, hence masks for mean "
               "distances within one ulp of the threshold (device %r, numpy %r).  GSX_STRICT_NUMPY=1 turns this warning into an error."
               % (np.__version__, got.tolist(), want.tolist()))
        # a drop-in keeps running where the reference runs: a warning by default; the bit-exact-mask contract
        # cannot be kept on this numpy, so tests / CI / anyone who needs the contract opt into the hard error
        if os.environ.get("GSX_STRICT_NUMPY") == "1":
            _numpy_reduction_checked = None
            raise GsxError(msg)
        warnings.warn(msg, RuntimeWarning, stacklevel=2)
    return _numpy_reduction_checked


def sor_filter(xyz, k: int, threshold_factor: float, algo: int = KNN_AUTO, want_mean: bool = True,
               want_info: bool = False):
    """Whole SOR on one GPU from host buffers (C ABI gsx_sor_filter).
    -> dict(mask bool[N], mean_dists f32[N] | None, mean, std, threshold (np.float32), info | None)"""
    lib = require_hip()
    numpy_reduction_selfcheck()
    keep, px, py, pz, stride, n = _xyz_pointers(xyz)
    mask = np.empty(n, dtype=np.uint8)
    mean = np.empty(n, dtype=np.float32) if want_mean else None
    stats = np.empty(3, dtype=np.float32)
    info = SorInfo() if want_info else None
    rc = lib.gsx_sor_filter(px, py, pz, stride, n, int(k), float(threshold_factor), int(algo),
                            mask.ctypes.data, mean.ctypes.data if want_mean else None, stats.ctypes.data,
                            C.byref(info) if want_info else None)
    check(rc, "gsx_sor_filter")
    del keep
    return {"mask": mask.view(np.bool_), "mean_dists": mean, "mean": stats[0], "std": stats[1],
            "threshold": stats[2], "info": info.as_dict() if want_info else None}


def density_voxels(xyz, voxel_size: float, min_points: int, dense_cap: int | None = None):
    """Voxel occupancy on the GPU (C ABI gsx_density_voxels).
    -> dict(n_unique, dense_keys int64[M,3] in np.unique(axis=0) order, dense_counts int64[M])"""
    lib = require_hip()
    keep, px, py, pz, stride, n = _xyz_pointers(xyz)
    if dense_cap is None:
        # count >= min_points  =>  at most n / max(min_points,1) dense voxels
        dense_cap = int(min(n, n // max(int(min_points), 1) + 1))
    keys = np.empty((max(dense_cap, 1), 3), dtype=np.int64)
    counts = np.empty(max(dense_cap, 1), dtype=np.int64)
    n_unique = C.c_int64()
    n_dense = C.c_int64()
    rc = lib.gsx_density_voxels(px, py, pz, stride, n, float(voxel_size), int(min_points), int(dense_cap),
                                C.byref(n_unique), C.byref(n_dense), keys.ctypes.data, counts.ctypes.data)
    check(rc, "gsx_density_voxels")
    del keep
    m = int(n_dense.value)
    return {"n_unique": int(n_unique.value), "dense_keys": keys[:m].copy(), "dense_counts": counts[:m].copy()}


def density_mask(xyz, voxel_size: float, kept_keys: np.ndarray) -> np.ndarray:
    """mask[i] = voxel(i) in kept_keys (C ABI gsx_density_mask)."""
    lib = require_hip()
    keep, px, py, pz, stride, n = _xyz_pointers(xyz)
    kk = np.ascontiguousarray(kept_keys, dtype=np.int64).reshape(-1, 3)
    mask = np.empty(n, dtype=np.uint8)
    check(lib.gsx_density_mask(px, py, pz, stride, n, float(voxel_size), kk.ctypes.data, len(kk), mask.ctypes.data),
          "gsx_density_mask")
    del keep
    return mask.view(np.bool_)


def voxel_clusters(keys, keep_multicluster: bool):
    """6-connected clusters of distinct absolute voxel keys and the keep rule (C ABI gsx_voxel_clusters)
    -> dict(status, keep bool[M] in input order, kept_clusters, largest); status DENSITY_HOST: a tie for the largest cluster
    without keep_multicluster -- ``keep`` decides nothing, take the host steps (processing/clusters.py)"""
    lib = require_hip()
    kk = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1, 3)
    keep = np.zeros(len(kk), dtype=np.uint8)
    info = DensityInfo()
    check(lib.gsx_voxel_clusters(kk.ctypes.data, len(kk), 1 if keep_multicluster else 0, keep.ctypes.data, C.byref(info)),
          "gsx_voxel_clusters")
    return {"status": int(info.status), "keep": keep.view(np.bool_), "kept_clusters": int(info.kept_clusters),
            "largest": int(info.largest)}


def kmeans_lloyd(data: np.ndarray, init_centroids: np.ndarray, max_iter: int):
    """max_iter x (assign, update) on the GPU (C ABI gsx_kmeans_lloyd) -> (centroids f32[K,D], labels i32[N])."""
    lib = require_hip()
    data = np.ascontiguousarray(data, dtype=np.float32)
    init = np.ascontiguousarray(init_centroids, dtype=np.float32)
    n, d = data.shape
    k = init.shape[0]
    if init.shape[1] != d:
        raise ValueError("init_centroids has the wrong dimensionality")
    cent = np.empty((k, d), dtype=np.float32)
    labels = np.empty(n, dtype=np.int32)
    check(lib.gsx_kmeans_lloyd(data.ctypes.data, n, d, k, int(max_iter), init.ctypes.data, cent.ctypes.data,
                               labels.ctypes.data), "gsx_kmeans_lloyd")
    return cent, labels


def kmeans_pp_trials(k: int) -> int:
    """scikit-learn's n_local_trials (_kmeans_plusplus)"""
    return 2 + int(np.log(k))


def kmeans_pp(data: np.ndarray, k: int, uniforms: np.ndarray, n_local_trials: int | None = None) -> np.ndarray:
    """greedy k-means++ seeding on the GPU (C ABI gsx_kmeans_pp); uniforms: 1 + (k-1) * n_local_trials numbers in [0,1)
    (np.random.random_sample) -> initial centroids f32[k, d]"""
    lib = require_hip()
    data = np.ascontiguousarray(data, dtype=np.float32)
    n, d = data.shape
    L = kmeans_pp_trials(k) if n_local_trials is None else int(n_local_trials)
    u = np.ascontiguousarray(uniforms, dtype=np.float64)
    if u.shape != (1 + (int(k) - 1) * L,):
        raise ValueError("expected 1 + (k-1) * n_local_trials uniform numbers")
    cent = np.empty((int(k), d), dtype=np.float32)
    check(lib.gsx_kmeans_pp(data.ctypes.data, n, d, int(k), u.ctypes.data, L, cent.ctypes.data), "gsx_kmeans_pp")
    return cent


def kmeans1d(vals: np.ndarray, k: int, iters: int = 50, want_labels: bool = False, want_inertia: bool = False):
    """Scalar K-Means codebook (C ABI gsx_kmeans1d: sort + prefix sums + Lloyd on run boundaries from two companded starts).
    -> centroids f32[k] ascending (, labels i32[n]) (, inertia f64[3]: chosen, start A, start B).  Deterministic."""
    lib = require_hip()
    v = np.ascontiguousarray(vals, dtype=np.float32).reshape(-1)
    if not 1 <= int(k) <= 1024:
        raise ValueError("kmeans1d: 1 <= k <= 1024")
    cent = np.empty(int(k), dtype=np.float32)
    labels = np.empty(len(v), dtype=np.int32) if want_labels else None
    inertia = np.zeros(3, dtype=np.float64)
    check(lib.gsx_kmeans1d(v.ctypes.data, len(v), int(k), int(iters), cent.ctypes.data,
                           labels.ctypes.data if want_labels else None, inertia.ctypes.data), "gsx_kmeans1d")
    out = (cent,)
    if want_labels:
        out += (labels,)
    if want_inertia:
        out += (inertia,)
    return out[0] if len(out) == 1 else out


PALETTE_LANES = 8   # concurrent contexts for independent K-Means problems (bench.py config4 at 10M splats: 1 lane 72.8 ms,
                    # 2: 57.1, 4: 54.9, 8: 50.7 -- profiles/r03_variants.txt)


def kmeans_lloyd_many(problems, max_iter: int, lanes: int = PALETTE_LANES, device: int = 0):
    """Independent Lloyd problems -- the SOG palette's chunks, formats/sog.py:536-552 -- on `lanes` contexts with streams of
    their own: while one chunk's ~100 kernels run, the next chunks' rows are uploaded and their kernels fill the tails.
    problems: list of (data f32[n,d], init f32[k,d]); -> list of (centroids f32[k,d], labels i32[n]).  Same kernels and
    launch order per problem as kmeans_lloyd, hence the same results."""
    require_hip()
    if not problems:
        return []
    shapes = {(p[0].shape[1], p[1].shape[0], p[1].shape[1]) for p in problems}
    batched = len(shapes) == 1 and next(iter(shapes))[0] in (9, 24, 45) and next(iter(shapes))[1] >= 64
    if batched and len(problems) > 1 and all(len(p[0]) > 0 for p in problems):
        # the palette's usual case: every chunk the same d and k -> one batched call, the problem is a grid dimension
        # (round 5: gsx_kmeans_lloyd_batch_dev; per problem the same kernels, launch order and arithmetic).  Only the shapes
        # of the matrix-core path batch on the device (d in 9/24/45, k >= 64: the C side's `batched` condition); for the
        # others the batch entry point would loop the problems on ONE stream, so they keep the concurrent lanes below.
        return kmeans_lloyd_batch(problems, max_iter, device)
    lanes = max(1, min(int(lanes), len(problems)))
    ctxs = [Context(device, own_stream=True) for _ in range(lanes)]
    out = [None] * len(problems)
    bufs = []
    try:
        cap_d = max(p[0].size for p in problems) * 4
        cap_c = max(p[1].size for p in problems) * 4
        cap_l = max(len(p[0]) for p in problems) * 4
        bufs = [(c.alloc(cap_d), c.alloc(cap_c), c.alloc(cap_l + 16)) for c in ctxs]
        for base in range(0, len(problems), lanes):
            live = []
            for lane in range(min(lanes, len(problems) - base)):
                data = np.ascontiguousarray(problems[base + lane][0], dtype=np.float32)
                init = np.ascontiguousarray(problems[base + lane][1], dtype=np.float32)
                n, d = data.shape
                k = init.shape[0]
                c = ctxs[lane]
                bd, bc, bl = bufs[lane]
                check(c.lib.gsx_dev_upload_async(c.handle, bd.ptr, data.ctypes.data, data.nbytes), "gsx_dev_upload_async")
                check(c.lib.gsx_dev_upload_async(c.handle, bc.ptr, init.ctypes.data, init.nbytes), "gsx_dev_upload_async")
                check(c.lib.gsx_dev_memset(c.handle, bl.ptr, 0, 4 * n), "gsx_dev_memset")   # max_iter == 0: labels stay 0
                check(c.lib.gsx_kmeans_lloyd_dev(c.handle, bd.ptr, n, d, k, int(max_iter), bc.ptr, bl.ptr), "gsx_kmeans_lloyd_dev")
                live.append((lane, data, init, n, d, k))   # (keeps the host arrays alive until the lane has been drained)
            for lane, _, _, n, d, k in live:
                bd, bc, bl = bufs[lane]
                out[base + lane] = (bc.download(np.float32, k * d).reshape(k, d), bl.download(np.int32, n))
    finally:
        for trio in bufs:
            for b in trio:
                b.free()
        for c in ctxs:
            c.close()
    return out


def kmeans_lloyd_batch(problems, max_iter: int, device: int = 0):
    """problems of ONE shape (same d, same k): rows concatenated in HBM, gsx_kmeans_lloyd_batch_dev runs every iteration of
    all of them as one set of launches -> list of (centroids f32[k,d], labels i32[n_p]) like kmeans_lloyd_many"""
    require_hip()
    d, k = problems[0][0].shape[1], problems[0][1].shape[0]
    rows = [len(p[0]) for p in problems]
    off = np.zeros(len(problems) + 1, dtype=np.int64)
    np.cumsum(rows, out=off[1:])
    n_total = int(off[-1])
    ctx = Context(device)
    bd = bc = bl = None
    try:
        bd, bc, bl = ctx.alloc(4 * n_total * d), ctx.alloc(4 * len(problems) * k * d), ctx.alloc(4 * n_total + 16)
        keep = []
        for i, (data, init) in enumerate(problems):   # chunk by chunk: no second host copy of the whole table
            a = np.ascontiguousarray(data, dtype=np.float32)
            b = np.ascontiguousarray(init, dtype=np.float32)
            keep.append((a, b))
            check(ctx.lib.gsx_dev_upload_async(ctx.handle, bd.ptr + 4 * d * int(off[i]), a.ctypes.data, a.nbytes), "gsx_dev_upload_async")
            check(ctx.lib.gsx_dev_upload_async(ctx.handle, bc.ptr + 4 * k * d * i, b.ctypes.data, b.nbytes), "gsx_dev_upload_async")
        check(ctx.lib.gsx_dev_memset(ctx.handle, bl.ptr, 0, 4 * n_total), "gsx_dev_memset")   # max_iter == 0: labels stay 0
        check(ctx.lib.gsx_kmeans_lloyd_batch_dev(ctx.handle, bd.ptr, off.ctypes.data, len(problems), d, k, int(max_iter), bc.ptr, bl.ptr),
              "gsx_kmeans_lloyd_batch_dev")
        cent = bc.download(np.float32, len(problems) * k * d).reshape(len(problems), k, d)
        lab = bl.download(np.int32, n_total)
        del keep
        return [(cent[i].copy(), lab[int(off[i]):int(off[i + 1])].copy()) for i in range(len(problems))]
    finally:
        for b in (bd, bc, bl):
            if b is not None:
                b.free()
        ctx.close()


def quantize_sorted_codebook(vals: np.ndarray, codebook: np.ndarray) -> np.ndarray:
    lib = require_hip()
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    cb = np.ascontiguousarray(codebook, dtype=np.float32)
    if len(cb) > 256:
        raise ValueError("codebook indices are uint8: at most 256 entries")
    out = np.empty(vals.shape, dtype=np.uint8)
    check(lib.gsx_quantize_sorted_codebook(vals.ctypes.data, vals.size, cb.ctypes.data, len(cb), out.ctypes.data),
          "gsx_quantize_sorted_codebook")
    return out


def lexsort3(k0: np.ndarray, k1: np.ndarray, k2: np.ndarray) -> np.ndarray:
    """np.lexsort((k0, k1, k2)) for float32 keys on the GPU (C ABI gsx_lexsort3) -> int64 indices"""
    lib = require_hip()
    cols = [np.ascontiguousarray(c, dtype=np.float32) for c in (k0, k1, k2)]
    n = len(cols[0])
    out = np.empty(n, dtype=np.uint32)
    if n:
        check(lib.gsx_lexsort3(cols[0].ctypes.data, cols[1].ctypes.data, cols[2].ctypes.data, n, out.ctypes.data), "gsx_lexsort3")
    return out.astype(np.int64)


def sog_quats(rot_rows: np.ndarray) -> np.ndarray:
    """formats/sog.py:315-386 on the GPU (C ABI gsx_sog_quats): (n,4) float32 -> (n,4) uint8 (c0, c1, c2, 252 + argmax)"""
    lib = require_hip()
    q = np.ascontiguousarray(rot_rows, dtype=np.float32)
    if q.ndim != 2 or q.shape[1] != 4:
        raise ValueError("expected (n,4) quaternion rows")
    out = np.empty((len(q), 4), dtype=np.uint8)
    if len(q):
        check(lib.gsx_sog_quats(q.ctypes.data, len(q), out.ctypes.data), "gsx_sog_quats")
    return out


def _log_transform(v):
    return np.sign(v) * np.log(np.abs(v) + 1.0)          # formats/sog.py:280-281, numpy's own float32 arithmetic


def sog_positions(v: np.ndarray, stats: dict | None = None):
    """formats/sog.py:279-309 for one axis -> (u16[n], np.float32 min, np.float32 max of the log-transformed axis), byte-identical
    to the reference's numpy expression.  The transcendental runs on the GPU (C ABI gsx_sog_positions, rounding certificate);
    numpy evaluates (i) the few values next to the extremes of v -- the transform is monotone, a relative window of 1e-3
    around min / max of v holds every candidate for np.min / np.max of the transformed axis -- and (ii) the flagged texels."""
    lib = require_hip()
    v = np.ascontiguousarray(v, dtype=np.float32)
    n = len(v)
    if n == 0:
        return np.zeros(0, np.uint16), np.float32(0), np.float32(0)
    vmin, vmax = np.min(v), np.max(v)
    span = np.float32(1e-3) * np.maximum(np.abs(vmin), np.abs(vmax)) + np.float32(1e-30)
    lo_c, hi_c = v[v <= vmin + span], v[v >= vmax - span]
    if not (np.isfinite(vmin) and np.isfinite(vmax)) or len(lo_c) + len(hi_c) > max(4096, n // 8):
        t = _log_transform(v)                              # degenerate input: the reference's expression as is
        mn, mx = np.min(t), np.max(t)
    else:
        mn, mx = np.min(_log_transform(lo_c)), np.max(_log_transform(hi_c))
    out = np.empty(n, dtype=np.uint16)
    unc = np.empty(n, dtype=np.uint8)
    check(lib.gsx_sog_positions(v.ctypes.data, n, float(mn), float(mx), out.ctypes.data, unc.ctypes.data), "gsx_sog_positions")
    idx = np.flatnonzero(unc)
    if len(idx):
        with np.errstate(all="ignore"):
            t = (_log_transform(v[idx]) - mn) / (mx - mn)
            out[idx] = np.clip(t * 65535, 0, 65535).astype(np.uint16)
    if stats is not None:
        stats["uncertain"] = stats.get("uncertain", 0) + int(len(idx))
        stats["n"] = stats.get("n", 0) + n
    return out, mn, mx


def sog_alpha(opacity: np.ndarray, stats: dict | None = None) -> np.ndarray:
    """formats/sog.py:457-459 -> u8[n], byte-identical to numpy (C ABI gsx_sog_alpha + numpy for the flagged texels)"""
    lib = require_hip()
    o = np.ascontiguousarray(opacity, dtype=np.float32)
    n = len(o)
    out = np.empty(n, dtype=np.uint8)
    if n == 0:
        return out
    unc = np.empty(n, dtype=np.uint8)
    check(lib.gsx_sog_alpha(o.ctypes.data, n, out.ctypes.data, unc.ctypes.data), "gsx_sog_alpha")
    idx = np.flatnonzero(unc)
    if len(idx):
        with np.errstate(all="ignore"):
            out[idx] = np.clip(1.0 / (1.0 + np.exp(-o[idx])) * 255, 0, 255).astype(np.uint8)
    if stats is not None:
        stats["uncertain"] = stats.get("uncertain", 0) + int(len(idx))
        stats["n"] = stats.get("n", 0) + n
    return out


def morton_order(x: np.ndarray, y: np.ndarray, z: np.ndarray, ctx: "Context | None" = None, keep_device: bool = False):
    """formats/compressed_ply.py:245-291 on the GPU (C ABI gsx_morton_order_dev) -> (uint32 order, recursion levels).
    Stable inside runs of equal Morton code.  keep_device: also return the device copy of the order (caller frees)."""
    require_hip()
    cols = [np.ascontiguousarray(c, dtype=np.float32) for c in (x, y, z)]
    n = len(cols[0])
    own = ctx is None
    ctx = ctx or Context(0)
    bufs = []
    try:
        bufs = [ctx.alloc(max(c.nbytes, 16)).upload(c) for c in cols]
        order = ctx.alloc(max(4 * n, 16))
        levels = C.c_int()
        check(ctx.lib.gsx_morton_order_dev(ctx.handle, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, 1, n, order.ptr, C.byref(levels)),
              "gsx_morton_order_dev")
        host = order.download(np.uint32, n) if n else np.zeros(0, np.uint32)
        if keep_device:
            return host, int(levels.value), order
        order.free()
        return host, int(levels.value)
    finally:
        for b in bufs:
            b.free()
        if own:
            ctx.close()


CPLY_COLUMNS = ("x", "y", "z", "scale_0", "scale_1", "scale_2", "f_dc_0", "f_dc_1", "f_dc_2", "alpha", "rot_0", "rot_1", "rot_2", "rot_3")


def cply_pack(columns: dict, order: "np.ndarray | None", sh_columns=(), ctx: "Context | None" = None):
    """formats/compressed_ply.py:205-241 on the GPU (C ABI gsx_cply_pack_dev / gsx_cply_sh_dev).
    columns: the 14 float32 columns named in CPLY_COLUMNS (original table order; 'alpha' = numpy's sigmoid of the opacity);
    order: uint32 Morton order or None.  -> (chunks (ceil(n/256), 18) f32, vertices (n, 4) u32, sh (n, m) u8 or None)"""
    for name, c in [(nm, columns[nm]) for nm in CPLY_COLUMNS] + [("sh_columns[%d]" % i, c) for i, c in enumerate(sh_columns)]:
        if not is_f4(np.asarray(c).dtype):
            raise TypeError(f"cply_pack: column {name!r} is {np.asarray(c).dtype.str}; float32 columns only (the reference computes in "
                            f"the column's dtype)")
    require_hip()
    cols = [np.ascontiguousarray(columns[name], dtype=np.float32) for name in CPLY_COLUMNS]     # (byte order only)
    n = len(cols[0])
    nchunks = (n + 255) // 256
    own = ctx is None
    ctx = ctx or Context(0)
    bufs = []
    try:
        bufs = [ctx.alloc(max(c.nbytes, 16)).upload(c) for c in cols]
        ptrs = (C.c_void_p * 14)(*[b.ptr for b in bufs])
        d_order = None
        if order is not None:
            d_order = ctx.alloc(max(4 * n, 16)).upload(np.ascontiguousarray(order, dtype=np.uint32))
            bufs.append(d_order)
        d_chunk, d_vert = ctx.alloc(max(72 * nchunks, 16)), ctx.alloc(max(16 * n, 16))
        bufs += [d_chunk, d_vert]
        check(ctx.lib.gsx_cply_pack_dev(ctx.handle, ptrs, d_order.ptr if d_order else None, n, d_chunk.ptr, d_vert.ptr), "gsx_cply_pack_dev")
        chunks = d_chunk.download(np.float32, 18 * nchunks).reshape(nchunks, 18)
        verts = d_vert.download(np.uint32, 4 * n).reshape(n, 4)
        sh = None
        m = len(sh_columns)
        if m:
            flat = np.empty((m, n), dtype=np.float32)
            for i, c in enumerate(sh_columns):
                flat[i] = c
            d_sh, d_out = ctx.alloc(max(flat.nbytes, 16)).upload(flat), ctx.alloc(max(n * m, 16))
            bufs += [d_sh, d_out]
            check(ctx.lib.gsx_cply_sh_dev(ctx.handle, d_sh.ptr, m, n, d_order.ptr if d_order else None, n, d_out.ptr), "gsx_cply_sh_dev")
            sh = d_out.download(np.uint8, n * m).reshape(n, m)
        return chunks, verts, sh
    finally:
        for b in bufs:
            b.free()
        if own:
            ctx.close()


def prefault(large: bool, *arrays):
    """touch every page of freshly allocated result arrays on a helper thread WHILE the device works (numpy's strided fill releases
    the GIL; the caller sits in ctypes calls anyway): the download that follows then writes into mapped pages -- 610 MB of texels
    / vertices arrive at 28-34 GB/s through the staging lanes when every 8 MiB chunk first has to fault its 2048 pages in, at link
    rate when the pages are there.  Only when `large` (the caller's rule: a thread costs more than a small result's faults) and
    for the arrays that are not None.  -> join(), to be called before the download (nothing to wait for when nothing was started)"""
    arrays = [a for a in arrays if a is not None]
    if not large or not arrays:
        return lambda: None

    def run():
        for a in arrays:
            flat = a.reshape(-1).view(np.uint8)
            flat[::4096] = 0
    th = threading.Thread(target=run, name="gsx-prefault", daemon=True)
    th.start()
    return th.join


def prefault_parallel(a: np.ndarray, threads: int = 8):
    """prefault() for one large array on `threads` helper threads, each touching a contiguous share of its pages (numpy's strided
    fill releases the GIL): where nothing else runs meanwhile -- the resident materialise has only a few milliseconds of device
    work to hide the faults of a 2.5 GB table behind -- one thread's 100 ms of page faults are the whole stage.  -> join()"""
    flat = a.reshape(-1).view(np.uint8)
    n = flat.size
    if n < (1 << 22):
        return lambda: None
    cuts = [(n * i // threads) & ~4095 for i in range(threads)] + [n]

    def run(lo, hi):
        flat[lo:hi:4096] = 0
    ths = [threading.Thread(target=run, args=(lo, hi), name="gsx-prefault", daemon=True) for lo, hi in zip(cuts, cuts[1:]) if hi > lo]
    for th in ths:
        th.start()
    return lambda: [th.join() for th in ths] and None


def stage_in(s: "ArenaSession", out: np.ndarray, nbytes: int, fill, stage: str):
    """A table reader's host half, all of it before any device work: prefault `out` when it is at least 4 MiB, take the
    session's staging buffer "in" of `nbytes`, let ``fill(host)`` put the file's bytes there and mark `stage`.  What `fill`
    raises leaves the block as it is: no device buffer has been asked for by then, nothing uploaded or launched.  A function of
    the session and no method of it, because the SPZ and SOG host tests run it on a stand-in session that has staging() and
    nothing else.  -> (host, join); ArenaSession.upload_in and .download_rows are the device half"""
    join = prefault(out.nbytes >= (1 << 22), out)
    host = s.staging("in", nbytes)
    fill(host)
    s.mark(stage)
    return host, join


def file_backed(a) -> bool:
    """is this array a view of a memory-mapped FILE (np.memmap, np.frombuffer over an mmap)?  Pinning such pages in place would
    either fail (read-only mapping) or, for a copy-on-write mapping, make the kernel copy every page first"""
    import mmap
    seen = 0
    while a is not None and seen < 16:
        if isinstance(a, (np.memmap, mmap.mmap)):
            return True
        a = a.base if isinstance(a, np.ndarray) else (a.obj if isinstance(a, memoryview) else None)
        seen += 1
    return False


def upload_table(lib, ctx, dev_ptr: int, rows: np.ndarray):
    """the writers' one upload of a whole table: anonymous memory goes through gsx_dev_upload_staged (pages pinned in place ahead of
    the DMA), a view of a mapped file through the runtime's plain copy"""
    if file_backed(rows):
        check(lib.gsx_dev_upload(ctx.handle, dev_ptr, rows.ctypes.data, rows.nbytes), "gsx_dev_upload")
    else:
        check(lib.gsx_dev_upload_staged(ctx.handle, dev_ptr, rows.ctypes.data, rows.nbytes), "gsx_dev_upload_staged")


def narrow_rows(data: np.ndarray, extra=()) -> np.ndarray:
    """the table a writer uploads: rows wider than 512 bytes (the kernels' limit) keep only the fields the writer reads -- those of
    SOG_FIELD_NAMES, at most 59 x 4 bytes per row, and `extra`; C-contiguous either way"""
    if data.dtype.itemsize > 512:
        import numpy.lib.recfunctions as rfn
        data = rfn.repack_fields(data[[nm for nm in SOG_FIELD_NAMES if nm in data.dtype.fields] + list(extra)])
    return np.ascontiguousarray(data)


def rest_nonzero_word(lib, ctx, d_rows, lay: SpzLayout, n: int, scan_fields) -> int:
    """one device pass over resident rows -> bit i set when field f_rest_i, i in `scan_fields`, holds a value != 0"""
    word = C.c_uint64(0)
    want = sum(1 << int(i) for i in scan_fields)
    check(lib.gsx_spz_rest_nonzero_dev(ctx.handle, d_rows.ptr, C.byref(lay), n, want, C.byref(word)), "gsx_spz_rest_nonzero_dev")
    return word.value


PROFILE_AXES = ("x", "y", "z")
PROFILE_REST = tuple("f_rest_%d" % i for i in range(45))
PROFILE_MAX_ROW_BYTES = 512   # csrc/row_tile.h SPZ_MAX_ROW_BYTES


def profile_layout(dtype: np.dtype):
    """gsx_profile_layout of a structured dtype -> (layout, foreign): the '<f4' fields among x y z and f_rest_0..44 take part;
    `foreign` names the fields of another type, which stay absent in the layout (the caller takes the reference's numpy
    expressions for those quantities: profile_foreign)"""
    fields = dtype.fields or {}
    lay, foreign = ProfileLayout(), []
    lay.row_bytes = dtype.itemsize
    for k, nm in enumerate(PROFILE_AXES + PROFILE_REST):
        ok = nm in fields and fields[nm][0] == np.dtype("<f4")
        if nm in fields and not ok:
            foreign.append(nm)
        if k < 3:
            lay.xyz_offset[k] = int(fields[nm][1]) if ok else -1
        else:
            lay.rest_offset[k - 3] = int(fields[nm][1]) if ok else -1
    return lay, foreign


def profile_foreign(prof: dict, table: np.ndarray, foreign) -> dict:
    """the quantities of `foreign` fields (profile_layout) from the reference's own numpy expressions on `table`, into `prof`"""
    with np.errstate(all="ignore"):
        for nm in foreign:
            col = table[nm]
            if nm in PROFILE_AXES:
                a = PROFILE_AXES.index(nm)
                lo, hi = float(np.min(col)), float(np.max(col))
                isnan = lo != lo or hi != hi
                prof["lo"] = prof["lo"][:a] + (float("nan") if isnan else lo,) + prof["lo"][a + 1:]
                prof["hi"] = prof["hi"][:a] + (float("nan") if isnan else hi,) + prof["hi"][a + 1:]
                prof["nan_axes"] |= int(isnan) << a
            elif bool(np.any(col != 0)):
                prof["rest_nonzero"] |= 1 << PROFILE_REST.index(nm)
    return prof


def empty_profile() -> dict:
    """the profile of a table without rows"""
    return {"rest_nonzero": 0, "lo": (float("inf"),) * 3, "hi": (float("-inf"),) * 3, "nan_axes": 0, "n": 0}


def table_profile_dev(ctx: "Context", d_rows, first_byte: int, n: int, dtype: np.dtype) -> dict:
    """gsx_table_profile_dev: one device pass over `n` resident rows of `dtype` (row 0 at byte `first_byte` of `d_rows`, a
    DeviceArray or a device address; 15 readable bytes behind the last row) -> the profile dict of the '<f4' fields"""
    lay, _ = profile_layout(np.dtype(dtype))
    res = TableProfile()
    ptr = d_rows.ptr if hasattr(d_rows, "ptr") else int(d_rows)
    check(load().gsx_table_profile_dev(ctx.handle, ptr, int(first_byte), int(n), C.byref(lay), C.byref(res)), "gsx_table_profile_dev")
    return res.as_dict()


def host_table_profile(table: np.ndarray, threads: int = 0) -> dict:
    """The profile of a host table: gsx_table_profile_host's threaded pass over the rows for the '<f4' fields, the reference's
    numpy expressions for fields of another type, for a table wider than 512 bytes or not C-contiguous, and none at all for an
    empty one"""
    n = len(table)
    if n == 0:
        return empty_profile()
    lay, foreign = profile_layout(table.dtype)
    if table.ndim != 1 or not table.flags.c_contiguous or table.dtype.itemsize > PROFILE_MAX_ROW_BYTES:
        prof = dict(empty_profile(), n=n)
        return profile_foreign(prof, table, [nm for nm in PROFILE_AXES + PROFILE_REST if nm in (table.dtype.fields or {})])
    res = TableProfile()
    check(load().gsx_table_profile_host(table.ctypes.data, n, C.byref(lay), int(threads), C.byref(res)), "gsx_table_profile_host")
    return profile_foreign(res.as_dict(), table, foreign)


def finish_profile(profile: "dict | None", table: np.ndarray):
    """A public reader's last step with a `profile` dict, which it emptied before the read: the session has filled it and only
    the fields that are not '<f4' are added from numpy; or no rows were resident -- the canonical PLY read on the host, an empty
    file, a row over 512 bytes, a fallback's table -- and host_table_profile fills it."""
    if profile is None:
        return
    if "rest_nonzero" in profile and profile.get("n") == len(table):
        foreign = profile_layout(table.dtype)[1]
        if foreign:
            profile_foreign(profile, table, foreign)
    else:
        profile.clear()
        profile.update(host_table_profile(table))


def with_profile(profile: "dict | None", read):
    """A public reader with its ``profile=`` keyword: read() -> a table or (table, ...), handed on as it is; a given dict is
    emptied before the read and holds the returned table's profile after it (finish_profile)"""
    if profile is None:
        return read()
    profile.clear()
    res = read()
    finish_profile(profile, res[0] if isinstance(res, tuple) else res)
    return res


def profile_kw(profile: "dict | None") -> dict:
    """the keyword a public reader hands to its *_unpack_table: none at all without a profile dict (the call is then the one it
    was before the keyword existed)"""
    return {} if profile is None else {"profile": profile}


def profile_slack(profile: "dict | None") -> int:
    """bytes a reader adds behind its decoded rows when it is asked for a profile: the pass's 16-byte loads reach up to 15 bytes
    past the last row"""
    return 0 if profile is None else 16


def session_profile(s: "ArenaSession", profile: "dict | None", d_rows, n_dev: int, n: int, dtype: np.dtype):
    """A reader's hook between its decode launch and download_rows: with a `profile` dict, the device pass over the `n_dev`
    decoded rows of `d_rows`, the stage mark "profile", and the dict filled for the table of `n` rows the reader returns (the
    rows past n_dev are zero: the compressed-PLY reader's tail).  Without one, nothing."""
    if profile is None:
        return
    prof = table_profile_dev(s.ctx, d_rows, 0, n_dev, dtype)
    if n > n_dev:
        fields = dtype.fields or {}
        axes = [nm in fields and fields[nm][0] == np.dtype("<f4") for nm in PROFILE_AXES]
        prof["lo"] = tuple(min(v, 0.0) if on else v for v, on in zip(prof["lo"], axes))   # (nan stays nan)
        prof["hi"] = tuple(max(v, 0.0) if on else v for v, on in zip(prof["hi"], axes))
        prof["n"] = n
    s.mark("profile")
    profile.update(prof)


RESIDENT_MAX_ROW_BYTES = 512   # csrc/row_tile.h SPZ_MAX_ROW_BYTES


@contextlib.contextmanager
def stage_clock(stage_ms: "dict | None", name: str, ctx: "Context | None" = None):
    """``with stage_clock(stage_ms, "take"):`` adds the block's milliseconds to stage_ms[name] (no dict: no clock), after a
    synchronisation of `ctx` when one is given.  A block that raises records nothing."""
    t0 = time.perf_counter()
    yield
    if stage_ms is not None:
        if ctx is not None:
            ctx.synchronize()
        stage_ms[name] = round(stage_ms.get(name, 0.0) + (time.perf_counter() - t0) * 1e3, 3)


def resident_take_dtype(dtype, extra_names=()) -> "np.dtype | None":
    """The dtype of the rows ResidentRows.take writes: `dtype`'s fields and one 'u1' field per extra name, or None when
    gsx_rows_take_dev cannot write them -- it appends the extra bytes to the source row, so the widened row has to END in exactly
    those bytes (numpy may place them elsewhere: `descr` of a dtype with padding names the gaps) and stay within
    RESIDENT_MAX_ROW_BYTES.  A pure function of the dtype and the names."""
    dtype = np.dtype(dtype)
    names = tuple(extra_names)
    new = np.dtype(dtype.descr + [(nm, "u1") for nm in names]) if names else dtype
    at_the_end = all(new.fields[nm][1] == dtype.itemsize + i for i, nm in enumerate(names))
    if not at_the_end or new.itemsize != dtype.itemsize + len(names) or new.itemsize > RESIDENT_MAX_ROW_BYTES:
        return None
    return new


class ResidentRows:
    """A table's rows in HBM, as a reader decoded them, beyond the reader's call: `n` packed rows of `dtype` from byte
    `first_byte` (0 ... 15) of the 16-byte aligned device address `ptr`, with 16 readable bytes behind the last row -- what
    gsx_table_profile_dev, gsx_rows_columns_f32_dev and gsx_rows_take_dev take.

    The buffer is an allocation of a Context this object owns, and no named arena buffer: those are overwritten by the next call
    of their lease group and freed by release_arenas().  A device address is valid in every context of this process on the same
    device, so a reader's session writes into it and a chain's or a writer's context reads it.  ``close()`` frees the buffer and
    the context (idempotent; ``__del__`` calls it).  ``ResidentRows.open_count`` counts the objects not closed yet.

    The rows own the device work on their bytes: ``take()`` is the one gsx_rows_take_dev into new rows -- its dtype, the rule that
    refuses it (resident_take_dtype), the field offsets -- and ``download_into()`` the copy to the host."""

    open_count = 0

    def __init__(self, n: int, dtype, device: int = 0, first_byte: int = 0):
        self.n, self.dtype, self.device, self.first_byte = int(n), np.dtype(dtype), int(device), int(first_byte)
        self.ptr = None
        self._ctx = self._buf = None
        if not 0 <= self.first_byte <= 15 or not 1 <= self.dtype.itemsize <= RESIDENT_MAX_ROW_BYTES or self.n < 0:
            raise ValueError("ResidentRows: %d rows of %d bytes from byte %d" % (self.n, self.dtype.itemsize, self.first_byte))
        self._ctx = Context(self.device)
        try:
            self._buf = self._ctx.alloc(self.first_byte + self.nbytes + 16)
        except BaseException:
            self._ctx.close()
            self._ctx = None
            raise
        self.ptr = self._buf.ptr
        ResidentRows.open_count += 1

    @classmethod
    def from_host(cls, table: np.ndarray, device: int = 0, first_byte: int = 0) -> "ResidentRows":
        """the rows of a host table (1-D, structured or not, rows of up to 512 bytes) uploaded: for a caller that has no reader's
        ``keep=`` at hand, and the tests"""
        table = np.ascontiguousarray(table)
        if table.ndim != 1:
            raise ValueError("ResidentRows.from_host: a 1-D table")
        rr = cls(len(table), table.dtype, device, first_byte)
        try:
            if table.nbytes:
                upload_table(rr._ctx.lib, rr._ctx, rr.ptr + rr.first_byte, table)
        except BaseException:
            rr.close()
            raise
        return rr

    @property
    def nbytes(self) -> int:
        return self.n * self.dtype.itemsize

    @property
    def closed(self) -> bool:
        return self.ptr is None

    def download(self) -> np.ndarray:
        """-> a new host table of the `n` rows"""
        if self.ptr is None:
            raise ValueError("ResidentRows: closed")
        out = np.empty(self.n, self.dtype)
        return self.download_into(out)

    def download_into(self, out: np.ndarray) -> np.ndarray:
        """the rows into the host table `out` (n rows of dtype, C-contiguous), through the staging lanes -> out"""
        if self.ptr is None:
            raise ValueError("ResidentRows: closed")
        if out.shape != (self.n,) or out.dtype != self.dtype or not out.flags.c_contiguous:
            raise ValueError("ResidentRows.download_into: a table of %d rows of %s" % (self.n, self.dtype))
        if self.n:
            check(self._ctx.lib.gsx_dev_download_staged(self._ctx.handle, out.view(np.uint8).ctypes.data, self.ptr + self.first_byte, self.nbytes),
                  "gsx_dev_download_staged")
        return out

    def take(self, idx_ptr, n_out: int, zero_names=(), extra_ptr=None, extra_names=(), ctx: "Context | None" = None,
             stage_ms: "dict | None" = None) -> "ResidentRows | None":
        """-> NEW rows (the caller's to close) of resident_take_dtype(dtype, extra_names): row j is this object's row idx[j] --
        `idx_ptr`: the device address of `n_out` ascending uint32 row numbers, None: row j itself -- with the '<f4' fields among
        `zero_names` that the rows have zeroed, and behind it the len(extra_names) bytes of row idx[j] of the (n, len(extra_names))
        uint8 device array at `extra_ptr`.  One gsx_rows_take_dev on `ctx` (this object's own context without one), which returns
        when the rows are written; stage_ms["take"] is that call alone.  n_out == 0 launches nothing.  None, and nothing done,
        when the widened dtype cannot be written (resident_take_dtype).  These rows stay as they are and open."""
        if self.ptr is None:
            raise ValueError("ResidentRows: closed")
        extra_names = tuple(extra_names)
        new_dtype = resident_take_dtype(self.dtype, extra_names)
        if new_dtype is None:
            return None
        fields = self.dtype.fields or {}
        out = ResidentRows(n_out, new_dtype, self.device)
        try:
            if out.n:
                with stage_clock(stage_ms, "take"):
                    rows_take_dev(ctx if ctx is not None else self._ctx, self.ptr, self.first_byte, self.dtype.itemsize, self.n, idx_ptr, out.n,
                                  [fields[nm][1] for nm in zero_names if nm in fields], extra_ptr, len(extra_names), out.ptr)
        except BaseException:
            out.close()
            raise
        return out

    def transform(self, plan, stage_ms: "dict | None" = None, ctx: "Context | None" = None):
        """the scene transform `plan` (transform.plan_transform of this dtype) applied to these rows where they lie: one
        gsx_rows_transform_dev in place on `ctx` (this object's own context without one), joined; stage_ms["transform"] is that
        call alone.  A plan without work, or no rows, launches nothing."""
        if self.ptr is None:
            raise ValueError("ResidentRows: closed")
        if np.dtype(plan.dtype) != self.dtype:
            raise ValueError("ResidentRows.transform: a plan for %s, rows of %s" % (plan.dtype, self.dtype))
        if plan.identity or not self.n:
            return
        ctx = ctx if ctx is not None else self._ctx
        with stage_clock(stage_ms, "transform"):
            rows_transform_dev(ctx, self.ptr, self.first_byte, self.dtype.itemsize, self.n, transform_layout(plan), self.ptr)
            ctx.synchronize()

    def decimate(self, plan, idx_ptr=None, n_idx=None, zero_names=(), ctx: "Context | None" = None,
                 stage_ms: "dict | None" = None) -> "ResidentRows":
        """-> NEW rows (the caller's to close) of the same dtype: the voxel decimation `plan` (decimate.plan_decimate of this
        dtype) of these rows, or of the rows idx[0 .. n_idx) -- `idx_ptr`: the device address of `n_idx` ascending uint32 row
        numbers, as in take() -- with the fields among `zero_names` zeroed in every output row.  ``decimate_info`` of the new
        rows: groups, merged_groups, passed_through.  gsx_rows_decimate_plan_dev and gsx_rows_decimate_write_dev on `ctx` (this
        object's own context without one) with a workspace that lives for the call; stage_ms: the five DECIMATE_STAGES clocks,
        joined.  ValueError, and no row written, when a cell index leaves +-2^20 (the voxel size is too small for the scene's
        coordinates).  These rows stay as they are and open."""
        from . import decimate as _decimate
        if self.ptr is None:
            raise ValueError("ResidentRows: closed")
        if np.dtype(plan.dtype) != self.dtype:
            raise ValueError("ResidentRows.decimate: a plan for %s, rows of %s" % (plan.dtype, self.dtype))
        n = self.n if n_idx is None else int(n_idx)
        if not 0 <= n <= self.n or (idx_ptr is None and n not in (0, self.n)) or (idx_ptr is not None and n_idx is None):
            raise ValueError("ResidentRows.decimate: %d of %d rows (a survivor list and its length go together)" % (n, self.n))
        lay = decimate_layout(plan, _decimate.zero_fields(self.dtype, zero_names))
        ctx = ctx if ctx is not None else self._ctx
        info = {"groups": 0, "merged_groups": 0, "passed_through": 0}
        if n == 0:
            out = ResidentRows(0, self.dtype, self.device)
            out.decimate_info = info
            return out
        clocks = (C.c_float * len(DECIMATE_STAGES))() if stage_ms is not None else None
        words = (C.c_int64 * DECIMATE_INFO_WORDS)()
        work_bytes = C.c_int64(0)
        check(ctx.lib.gsx_rows_decimate_work_dev(ctx.handle, n, C.byref(work_bytes)), "gsx_rows_decimate_work_dev")
        work = ctx.alloc(work_bytes.value)
        out = None
        try:
            check(ctx.lib.gsx_rows_decimate_plan_dev(ctx.handle, self.ptr, self.first_byte, self.dtype.itemsize, self.n, idx_ptr, n, C.byref(lay),
                                                     work.ptr, work_bytes.value, words, clocks), "gsx_rows_decimate_plan_dev")
            if words[0] == DECIMATE_CELL_RANGE:
                raise ValueError("decimate: the voxel size %r is too small for the scene's coordinates (a cell index leaves +-2^20)"
                                 % (plan.voxel_size,))
            if words[0] != DECIMATE_OK:
                raise GsxError("gsx_rows_decimate_plan_dev: the index list is not strictly ascending inside [0, n)")
            out = ResidentRows(int(words[1]), self.dtype, self.device)
            check(ctx.lib.gsx_rows_decimate_write_dev(ctx.handle, self.ptr, self.first_byte, self.dtype.itemsize, self.n, idx_ptr, n, C.byref(lay),
                                                      work.ptr, work_bytes.value, out.ptr, out.first_byte, out.n, clocks),
                  "gsx_rows_decimate_write_dev")
            ctx.synchronize()
        except BaseException:
            try:
                ctx.synchronize()       # (a launch before the failure may still write into what is freed next)
            except GsxError:
                pass
            if out is not None:
                out.close()
            raise
        finally:
            work.free()
        if stage_ms is not None:
            for name, ms in zip(DECIMATE_STAGES, clocks):
                stage_ms[name] = round(stage_ms.get(name, 0.0) + float(ms), 3)
        out.decimate_info = {"groups": int(words[1]), "merged_groups": int(words[2]), "passed_through": int(words[4])}
        return out

    def _render_plan(self, ctx, plan, clocks):
        """gsx_rows_render_plan_dev of these rows into a workspace of its own -> (layout, workspace, its bytes, the info words);
        the workspace is the caller's to free.  RenderRefused for 2^31 instances or more."""
        if self.ptr is None:
            raise ValueError("ResidentRows: closed")
        if np.dtype(plan.dtype) != self.dtype:
            raise ValueError("ResidentRows.render: a plan for %s, rows of %s" % (plan.dtype, self.dtype))
        lay = render_layout(plan)
        words = (C.c_int64 * RENDER_INFO_WORDS)()
        work_bytes = C.c_int64(0)
        check(ctx.lib.gsx_rows_render_work_dev(ctx.handle, self.n, lay.width, lay.height, C.byref(work_bytes)), "gsx_rows_render_work_dev")
        work = ctx.alloc(work_bytes.value)
        try:
            check(ctx.lib.gsx_rows_render_plan_dev(ctx.handle, self.ptr, self.first_byte, self.dtype.itemsize, self.n, C.byref(lay), work.ptr,
                                                   work_bytes.value, words, clocks), "gsx_rows_render_plan_dev")
        except BaseException:
            work.free()
            raise
        return lay, work, work_bytes.value, words

    def render_records(self, plan, ctx: "Context | None" = None) -> np.ndarray:
        """-> the per-splat records of the rasteriser's first stage (RENDER_RECORD, one per row; an invisible row's is all zero):
        gsx_rows_render_plan_dev alone and one download of the workspace's head.  For the tests of that stage on its own."""
        ctx = ctx if ctx is not None else self._ctx
        _, work, _, _ = self._render_plan(ctx, plan, None)
        try:
            return work.download(RENDER_RECORD, self.n) if self.n else np.zeros(0, RENDER_RECORD)
        finally:
            work.free()

    def render(self, plan, stage_ms: "dict | None" = None, ctx: "Context | None" = None) -> np.ndarray:
        """-> the (height, width, 3) uint8 image of these rows under `plan` (render.plan_render of this dtype):
        gsx_rows_render_plan_dev and gsx_rows_render_draw_dev on `ctx` (this object's own context without one) with workspaces
        that live for the call, and one download of the image.  The instance workspace is sized by the plan call's total; a size
        above plan.max_work_bytes raises render.RenderRefused, naming the image size and the instance count, before that
        workspace or the image is allocated.  ``render_info``: visible, instances, rows.  stage_ms: the six RENDER_STAGES
        clocks, joined, and "download".  These rows stay as they are and open."""
        ctx = ctx if ctx is not None else self._ctx
        image_dev = self.render_dev(plan, ctx=ctx, stage_ms=stage_ms)
        try:
            cam = plan.camera
            with stage_clock(stage_ms, "download"):
                image = image_dev.download(np.uint8, cam.width * cam.height * 3).reshape(cam.height, cam.width, 3)
        finally:
            image_dev.free()
        return image

    def render_dev(self, plan, ctx: "Context | None" = None, stage_ms: "dict | None" = None) -> "DeviceArray":
        """render() up to and including gsx_rows_render_draw_dev, without the download: -> the image where the rasteriser left
        it, height * width * 3 bytes of HBM allocated on `ctx` (this object's own context without one), which the caller frees
        (``.free()``) -- for a consumer on the device (fidelity.compare_rows).  The workspaces live for the call; the refusal,
        ``render_info`` and the six RENDER_STAGES clocks are render()'s.  These rows stay as they are and open."""
        from . import render as _render
        ctx = ctx if ctx is not None else self._ctx
        clocks = (C.c_float * len(RENDER_STAGES))() if stage_ms is not None else None
        lay, work, work_bytes, words = self._render_plan(ctx, plan, clocks)
        inst = image_dev = None
        try:
            visible, instances, inst_bytes = int(words[1]), int(words[2]), int(words[3])
            if words[0] != RENDER_OK or inst_bytes > plan.max_work_bytes:
                raise _render.RenderRefused("render: an image of %d x %d needs %d (tile, splat) instances and %d bytes of workspace for them; "
                                            "max_work_bytes is %d" % (lay.width, lay.height, instances, inst_bytes, plan.max_work_bytes))
            inst = ctx.alloc(inst_bytes) if inst_bytes else None
            image_dev = ctx.alloc(lay.width * lay.height * 3)
            check(ctx.lib.gsx_rows_render_draw_dev(ctx.handle, self.n, C.byref(lay), work.ptr, work_bytes, inst.ptr if inst else None, inst_bytes,
                                                   image_dev.ptr, clocks), "gsx_rows_render_draw_dev")
        except BaseException:
            try:
                ctx.synchronize()       # (a launch before the failure may still write into what is freed next)
            except GsxError:
                pass
            if image_dev is not None:
                image_dev.free()
            raise
        finally:
            for buf in (inst, work):
                if buf is not None:
                    buf.free()
        if stage_ms is not None:
            for name, ms in zip(RENDER_STAGES, clocks):
                stage_ms[name] = round(stage_ms.get(name, 0.0) + float(ms), 3)
        self.render_info = {"visible": visible, "instances": instances, "rows": self.n}
        return image_dev

    def view_scores_into(self, plans, peak_ptr, total_ptr, stage_ms: "dict | None" = None, ctx: "Context | None" = None) -> dict:
        """The view scores of these rows under every plan of `plans` (views.plan_scores of this dtype, one per
        view) ADDED into the caller's device arrays: `peak_ptr` n uint32 (float32 bits), `total_ptr` n uint64, both zeroed
        before the first view -- the variant that leaves the scores in HBM for a chain.  Per view gsx_rows_render_plan_dev
        and gsx_rows_render_score_dev on `ctx` (this object's own context without one).  The fixed workspace is allocated
        once, for the largest image; the instance workspace grows to the largest view.  A view whose instances exceed its
        plan's max_work_bytes raises render.RenderRefused before anything of that view is allocated (the arrays then hold the
        views before it: the caller drops them).  -> dict(views, visible: per view, instances: per view, rows).  stage_ms: the
        six RENDER_STAGES clocks summed over the views, "blend" being the score kernel's."""
        from . import render as _render
        if self.ptr is None:
            raise ValueError("ResidentRows: closed")
        plans = list(plans)
        ctx = ctx if ctx is not None else self._ctx
        lays = []
        for plan in plans:
            if np.dtype(plan.dtype) != self.dtype:
                raise ValueError("ResidentRows.view_scores: a plan for %s, rows of %s" % (plan.dtype, self.dtype))
            lays.append(render_layout(plan))
        clocks = (C.c_float * len(RENDER_STAGES))() if stage_ms is not None else None
        info = {"views": len(plans), "visible": [], "instances": [], "rows": self.n}
        work_bytes = 0
        for lay in lays:
            need = C.c_int64(0)
            check(ctx.lib.gsx_rows_render_work_dev(ctx.handle, self.n, lay.width, lay.height, C.byref(need)), "gsx_rows_render_work_dev")
            work_bytes = max(work_bytes, int(need.value))
        work = ctx.alloc(work_bytes) if plans else None
        inst = None
        try:
            for plan, lay in zip(plans, lays):
                words = (C.c_int64 * RENDER_INFO_WORDS)()
                check(ctx.lib.gsx_rows_render_plan_dev(ctx.handle, self.ptr, self.first_byte, self.dtype.itemsize, self.n, C.byref(lay), work.ptr,
                                                       work_bytes, words, clocks), "gsx_rows_render_plan_dev")
                visible, instances, inst_bytes = int(words[1]), int(words[2]), int(words[3])
                if words[0] != RENDER_OK or inst_bytes > plan.max_work_bytes:
                    raise _render.RenderRefused("view %d of %d: an image of %d x %d needs %d (tile, splat) instances and %d bytes of workspace "
                                                "for them; max_work_bytes is %d" % (len(info["visible"]) + 1, len(plans), lay.width, lay.height,
                                                                                   instances, inst_bytes, plan.max_work_bytes))
                if inst_bytes and (inst is None or inst.nbytes < inst_bytes):
                    if inst is not None:
                        inst.free()
                        inst = None
                    inst = ctx.alloc(inst_bytes)
                check(ctx.lib.gsx_rows_render_score_dev(ctx.handle, self.n, C.byref(lay), work.ptr, work_bytes, inst.ptr if inst_bytes else None,
                                                        inst.nbytes if inst_bytes else 0, peak_ptr, total_ptr, clocks),
                      "gsx_rows_render_score_dev")
                info["visible"].append(visible)
                info["instances"].append(instances)
        except BaseException:
            try:
                ctx.synchronize()       # (a launch before the failure may still write into what is freed next)
            except GsxError:
                pass
            raise
        finally:
            for buf in (inst, work):
                if buf is not None:
                    buf.free()
        if stage_ms is not None:
            for name, ms in zip(RENDER_STAGES, clocks):
                stage_ms[name] = round(stage_ms.get(name, 0.0) + float(ms), 3)
        return info

    def view_scores(self, plans, stage_ms: "dict | None" = None, ctx: "Context | None" = None):
        """-> (peak float32[n], total uint64[n]) of these rows over the views `plans`: the largest blending weight of every row
        and the sum of its weights in units of 2^-24 (view_scores_into on two arrays that live for the call, and one download
        of each).  ``view_scores_info``: views, visible and instances per view, rows.  These rows stay as they are and open."""
        if self.ptr is None:
            raise ValueError("ResidentRows: closed")
        ctx = ctx if ctx is not None else self._ctx
        n = self.n
        d_peak, d_total = ctx.alloc(max(4 * n, 16)), None
        try:
            d_total = ctx.alloc(max(8 * n, 16))
            check(ctx.lib.gsx_dev_memset(ctx.handle, d_peak.ptr, 0, d_peak.nbytes), "gsx_dev_memset")
            check(ctx.lib.gsx_dev_memset(ctx.handle, d_total.ptr, 0, d_total.nbytes), "gsx_dev_memset")
            self.view_scores_info = self.view_scores_into(plans, d_peak.ptr, d_total.ptr, stage_ms=stage_ms, ctx=ctx)
            with stage_clock(stage_ms, "download"):
                return d_peak.download(np.float32, n), d_total.download(np.uint64, n)
        finally:
            for buf in (d_total, d_peak):
                if buf is not None:
                    buf.free()

    def profile(self) -> dict:
        """-> the profile dict of these rows: one gsx_table_profile_dev where they lie (no rows: empty_profile)"""
        if self.ptr is None:
            raise ValueError("ResidentRows: closed")
        return table_profile_dev(self._ctx, self.ptr, self.first_byte, self.n, self.dtype) if self.n else empty_profile()

    @classmethod
    def concat(cls, parts, dtype, runs_per_part, ctx: "Context | None" = None, stage_ms: "dict | None" = None) -> "ResidentRows":
        """-> NEW rows (the caller's to close) of `dtype`: the rows of every part, one behind the other, each re-laid by its
        runs (merge.remap_runs of the part's dtype and `dtype`).  One gsx_rows_remap_dev per part that has rows, at its running
        row offset, on `ctx` (the new rows' own context without one), all of them joined once at the end; stage_ms["remap"] is
        those launches and the join alone.  The parts stay as they are and open; when anything raises, the new rows are closed."""
        parts, runs_per_part = list(parts), list(runs_per_part)
        if len(parts) != len(runs_per_part):
            raise ValueError("ResidentRows.concat: %d parts, runs for %d" % (len(parts), len(runs_per_part)))
        if any(p.ptr is None for p in parts):
            raise ValueError("ResidentRows: closed")
        device = parts[0].device if parts else 0
        if any(p.device != device for p in parts):
            raise ValueError("ResidentRows.concat: parts on several devices")
        out = cls(sum(p.n for p in parts), dtype, device)
        use = ctx if ctx is not None else out._ctx
        try:
            with stage_clock(stage_ms, "remap"):
                row0 = 0
                for p, runs in zip(parts, runs_per_part):
                    if p.n:
                        rows_remap_dev(use, p.ptr, p.first_byte, p.dtype.itemsize, p.n, runs, out.ptr, out.first_byte, out.dtype.itemsize,
                                       row0, out.n)
                    row0 += p.n
                use.synchronize()
        except BaseException:
            try:
                use.synchronize()   # (a remap launched before the failure still writes into the rows that are freed next)
            finally:
                out.close()
            raise
        return out

    def close(self):
        if self.ptr is None:
            return
        self.ptr = None
        ResidentRows.open_count -= 1
        buf, ctx, self._buf, self._ctx = self._buf, self._ctx, None, None
        if buf is not None:
            buf.free()
        if ctx is not None:
            ctx.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


RESIDENT_F4_FIELDS = ("x", "y", "z", "opacity", "f_dc_0", "f_dc_1", "f_dc_2") + PROFILE_REST   # what DataProcessor reads or zeroes as words


def resident_same_rows(rr_dtype, rr_n: int, dtype, n: int) -> bool:
    """are `rr_n` resident rows of `rr_dtype` the rows of a host table of `n` rows of `dtype`, as far as shapes tell?  The same
    count, at least one row, the same structured dtype, rows of up to 512 bytes (the .splat writer's rule for its `resident`)"""
    if rr_dtype is None or dtype is None:
        return False
    rr_dtype, dtype = np.dtype(rr_dtype), np.dtype(dtype)
    return (int(rr_n) == int(n) and int(n) >= 1 and rr_dtype == dtype and dtype.fields is not None
            and 1 <= dtype.itemsize <= RESIDENT_MAX_ROW_BYTES)


def resident_eligible(rr_dtype, rr_n: int, dtype, n: int) -> bool:
    """DataProcessor's rule for its `resident` rows: resident_same_rows, x y z present, and every field the processor reads or
    zeroes as 32-bit words (RESIDENT_F4_FIELDS: x y z opacity f_dc_* f_rest_*) that the table has is '<f4'.  A pure function of
    the two dtypes and the two counts: no device, no table."""
    if not resident_same_rows(rr_dtype, rr_n, dtype, n):
        return False
    fields = np.dtype(dtype).fields
    f4 = np.dtype("<f4")
    return all(nm in fields for nm in ("x", "y", "z")) and all(fields[nm][0] == f4 for nm in RESIDENT_F4_FIELDS if nm in fields)


def resident_matches(resident, data) -> bool:
    """does the ResidentRows `resident` (or None) hold the rows of the host table `data`, by count and dtype?"""
    return (resident is not None and not resident.closed and isinstance(data, np.ndarray) and data.ndim == 1
            and resident_same_rows(resident.dtype, resident.n, data.dtype, len(data)))


def keep_kw(keep: "dict | None") -> dict:
    """the keyword a public reader hands to its *_unpack_table: none at all without a keep dict (profile_kw's rule)"""
    return {} if keep is None else {"keep": keep}


def with_keep(keep: "dict | None", read):
    """A public reader with its ``keep=`` keyword: a given dict is emptied before the read; after it, keep["rows"] stays only when
    it holds the rows of the very table the reader returns (a fallback's table, or a failed read, closes and drops it)"""
    if keep is None:
        return read()
    keep.clear()
    try:
        res = read()
    except BaseException:
        rr = keep.pop("rows", None)
        keep.clear()
        if rr is not None:
            rr.close()
        raise
    table = res[0] if isinstance(res, tuple) else res
    rr, of = keep.pop("rows", None), keep.pop("table", None)
    keep.clear()
    if rr is not None:
        if of is table and resident_matches(rr, table):
            keep["rows"] = rr
        else:
            rr.close()
    return res


def session_out(s: "ArenaSession", keep: "dict | None", n_dev: int, n: int, dtype: np.dtype, profile: "dict | None"):
    """The buffer a reader's decode kernel writes its `n_dev` rows into: the session's "out" (with the profile pass's slack), or --
    with a `keep` dict, for rows of up to 512 bytes -- the buffer of a new ResidentRows of all `n` rows, the `n - n_dev` rows
    behind the decoded ones zeroed on the device (the compressed-PLY reader's tail).  The session closes it when its block ends
    with an exception.  -> an object with .ptr"""
    rb = dtype.itemsize
    if keep is None or rb > RESIDENT_MAX_ROW_BYTES or n < 1:
        return s.buf("out", n_dev * rb + profile_slack(profile))
    rr = s.kept = ResidentRows(n, dtype, s.device)
    if n > n_dev:
        check(s.ctx.lib.gsx_dev_memset(s.ctx.handle, rr.ptr + n_dev * rb, 0, (n - n_dev) * rb), "gsx_dev_memset")
    return rr


def session_keep(s: "ArenaSession", keep: "dict | None", out: np.ndarray):
    """A reader's last step in its session: with a `keep` dict and rows that session_out() put into a ResidentRows, the session's
    stream is joined (every byte of the rows is written) and the dict receives them as keep["rows"], with the table they belong
    to as keep["table"] (with_keep checks it against what the public reader returns, and drops it).  Without, nothing."""
    rr, s.kept = s.kept, None
    if rr is None:
        return
    s.ctx.synchronize()
    keep["rows"], keep["table"] = rr, out


def rows_columns_dev(ctx: "Context", rows_ptr: int, first_byte: int, dtype: np.dtype, n: int, names, out_ptr: int):
    """gsx_rows_columns_f32_dev: the '<f4' fields `names` (1 ... 4) of `n` resident rows -> a dense (n, len(names)) array of words
    at the device address `out_ptr` (16-byte aligned).  Asynchronous."""
    fields = np.dtype(dtype).fields
    offs = (C.c_int32 * len(names))(*[int(fields[nm][1]) for nm in names])
    check(ctx.lib.gsx_rows_columns_f32_dev(ctx.handle, rows_ptr, int(first_byte), np.dtype(dtype).itemsize, int(n), offs, len(names), out_ptr),
          "gsx_rows_columns_f32_dev")


def rows_take_dev(ctx: "Context", rows_ptr: int, first_byte: int, stride_in: int, n_in: int, idx_ptr, n_out: int, zero_offsets, extra_ptr,
                  e: int, out_ptr: int):
    """gsx_rows_take_dev: the device twin of host_take_rows_shape on device addresses -- out row j = row idx[j] (idx_ptr None: row
    j) with the 4-byte fields at `zero_offsets` zeroed and `e` bytes of extra[idx[j]] appended"""
    zero_offsets = [int(o) for o in zero_offsets]
    offs = (C.c_int32 * max(len(zero_offsets), 1))(*zero_offsets)
    check(ctx.lib.gsx_rows_take_dev(ctx.handle, rows_ptr, int(first_byte), int(stride_in), int(n_in), idx_ptr, int(n_out), offs, len(zero_offsets),
                                    extra_ptr, int(e), out_ptr, int(stride_in) + int(e)), "gsx_rows_take_dev")


def remap_runs_array(runs):
    """merge.remap_runs' (source byte or -1, destination byte, byte count) triples as gsx_rows_remap_*'s int32 array -> (array, runs)"""
    flat = [int(v) for run in runs for v in run]
    if len(flat) % 3 or any(len(run) != 3 for run in runs):
        raise ValueError("remap runs: (source byte or -1, destination byte, byte count) triples")
    if any(not -2 ** 31 <= v < 2 ** 31 for v in flat):
        raise ValueError("remap runs: 32-bit values")
    return (C.c_int32 * max(len(flat), 1))(*flat), len(flat) // 3


def rows_remap_dev(ctx: "Context", src_ptr: int, src_first_byte: int, src_stride: int, n: int, runs, dst_ptr: int, dst_first_byte: int,
                   dst_stride: int, dst_row0: int, dst_rows: int):
    """gsx_rows_remap_dev: `n` resident rows re-laid by `runs` (merge.remap_runs) into rows [dst_row0, dst_row0 + n) of the
    `dst_rows` resident rows at `dst_ptr`; nothing outside those rows is written.  Asynchronous."""
    arr, n_runs = remap_runs_array(runs)
    check(ctx.lib.gsx_rows_remap_dev(ctx.handle, src_ptr, int(src_first_byte), int(src_stride), int(n), arr, n_runs, dst_ptr, int(dst_first_byte),
                                     int(dst_stride), int(dst_row0), int(dst_rows)), "gsx_rows_remap_dev")


def rows_remap_host(src: np.ndarray, runs, dst: np.ndarray, dst_row0: int = 0) -> np.ndarray:
    """gsx_rows_remap_host: the rows of the host table `src` re-laid by `runs` into rows [dst_row0, dst_row0 + len(src)) of the
    host table `dst` (both 1-D and C-contiguous, rows of up to 512 bytes) -> dst.  The path of a merge without resident rows, and
    the host tests' model of the kernel; no device is touched."""
    for name, a in (("source", src), ("destination", dst)):
        if not isinstance(a, np.ndarray) or a.ndim != 1 or not a.flags.c_contiguous:
            raise ValueError("rows_remap_host: the %s is a 1-D C-contiguous table" % name)
    if not dst.flags.writeable:
        raise ValueError("rows_remap_host: the destination is read-only")
    arr, n_runs = remap_runs_array(runs)
    s_at, d_at = src.ctypes.data, dst.ctypes.data          # (the C side takes a 16-byte aligned base and the first row's byte)
    check(load().gsx_rows_remap_host(s_at & ~15, s_at & 15, src.dtype.itemsize, len(src), arr, n_runs, d_at & ~15, d_at & 15, dst.dtype.itemsize,
                                     int(dst_row0), len(dst)), "gsx_rows_remap_host")
    return dst


def transform_layout(plan) -> TransformLayout:
    """gsx_transform_layout of a transform.TransformPlan"""
    lay = TransformLayout()
    lay.parts, lay.rest_m, lay.log_scale = int(plan.parts), int(plan.m), float(plan.log_scale)
    for name, offs in (("xyz_offset", plan.xyz), ("normal_offset", plan.normals), ("scale_offset", plan.scales), ("rot_offset", plan.rots)):
        getattr(lay, name)[:] = [int(o) for o in offs]
    lay.rest_offset[:] = [int(o) for o in plan.rest] + [-1] * (45 - len(plan.rest))
    for name, a in (("M", plan.M), ("R", plan.R), ("t", plan.t), ("q", plan.q), ("D1", plan.D[0]), ("D2", plan.D[1]), ("D3", plan.D[2])):
        getattr(lay, name)[:] = [float(v) for v in np.asarray(a, dtype=np.float64).reshape(-1)]
    return lay


def rows_transform_dev(ctx: "Context", rows_ptr: int, first_byte: int, stride: int, n: int, layout: TransformLayout, out_ptr: int):
    """gsx_rows_transform_dev: the scene transform of `n` resident rows -> rows at byte `first_byte` of `out_ptr` (which may be
    `rows_ptr`: in place).  Asynchronous."""
    check(ctx.lib.gsx_rows_transform_dev(ctx.handle, rows_ptr, int(first_byte), int(stride), int(n), C.byref(layout), out_ptr),
          "gsx_rows_transform_dev")


def rows_transform_host(table: np.ndarray, plan, out: "np.ndarray | None" = None) -> np.ndarray:
    """gsx_rows_transform_host: the kernel's per-row functions on a host table (1-D, C-contiguous, of plan.dtype) -> a new table,
    or `out` (which may be `table`: in place) -- the host tests' model of the device; no device is touched"""
    lib = load()
    if table.ndim != 1 or not table.flags.c_contiguous or table.dtype != np.dtype(plan.dtype):
        raise ValueError("rows_transform_host: a 1-D C-contiguous table of %s" % np.dtype(plan.dtype))
    if out is None:
        out = np.empty_like(table)
    elif out.shape != table.shape or out.dtype != table.dtype or not out.flags.c_contiguous:
        raise ValueError("rows_transform_host: an output of the table's shape")
    lay = transform_layout(plan)
    check(lib.gsx_rows_transform_host(table.ctypes.data, table.dtype.itemsize, len(table), C.byref(lay), out.ctypes.data), "gsx_rows_transform_host")
    return out


def rows_transform_table(data: np.ndarray, plan, stage_ms: "dict | None" = None, device: int = 0) -> np.ndarray:
    """The scene transform of a host table through the device: the rows uploaded once (ArenaSession.upload_rows), one
    gsx_rows_transform_dev in place there, and one download into a NEW, prefaulted table -- the caller's array is left alone.
    data: 1-D structured table of plan.dtype, rows of up to 512 bytes.  A plan without work, or no rows: a copy.
    One ArenaSession of the "transform" lease group; stage_ms: upload, transform, download."""
    data = np.ascontiguousarray(data)
    if data.ndim != 1 or data.dtype != np.dtype(plan.dtype) or not 1 <= data.dtype.itemsize <= RESIDENT_MAX_ROW_BYTES:
        raise ValueError("rows_transform_table: a 1-D table of %s, rows of up to %d bytes" % (np.dtype(plan.dtype), RESIDENT_MAX_ROW_BYTES))
    n = len(data)
    if plan.identity or n == 0:
        return data.copy()
    lib = require_hip()
    with ArenaSession("transform", device, stage_ms) as s:
        out = np.empty(n, data.dtype)
        join = prefault_parallel(out)
        d_rows = s.upload_rows(lib, data)
        rows_transform_dev(s.ctx, d_rows.ptr, 0, data.dtype.itemsize, n, transform_layout(plan), d_rows.ptr)
        s.mark("transform")
        s.download_rows(lib, out, d_rows, data.nbytes, join)
        s.mark("download")
    return out


def decimate_layout(plan, zero=()) -> DecimateLayout:
    """gsx_decimate_layout of a decimate.DecimatePlan; zero: further (name, offset) fields zeroed in every output row"""
    lay = DecimateLayout()
    lay.voxel_size = float(plan.voxel_size)
    lay.xyz_offset[:], lay.scale_offset[:], lay.rot_offset[:] = list(plan.xyz), list(plan.scales), list(plan.rots)
    lay.opacity_offset = int(plan.opacity)
    zero_offs = sorted({int(o) for _, o in tuple(plan.zero) + tuple(zero)})
    if len(plan.mean) > DECIMATE_MAX_MEAN or len(zero_offs) > DECIMATE_MAX_ZERO:
        raise ValueError("decimate: %d averaged and %d zeroed fields (at most %d and %d)" % (len(plan.mean), len(zero_offs), DECIMATE_MAX_MEAN,
                                                                                          DECIMATE_MAX_ZERO))
    lay.n_mean = len(plan.mean)
    for k, (_, o) in enumerate(plan.mean):
        lay.mean_offset[k] = int(o)
    lay.n_u8 = len(plan.u8)
    for k, (_, o) in enumerate(plan.u8):
        lay.u8_offset[k] = int(o)
    lay.n_zero = len(zero_offs)
    for k, o in enumerate(zero_offs):
        lay.zero_offset[k] = o
    return lay


def render_layout(plan) -> RenderLayout:
    """gsx_render_layout of a render.RenderPlan"""
    cam = plan.camera
    lay = RenderLayout()
    lay.xyz_offset[:], lay.scale_offset[:], lay.rot_offset[:] = list(plan.xyz), list(plan.scales), list(plan.rots)
    lay.opacity_offset = int(plan.opacity)
    lay.dc_offset[:], lay.rgb_offset[:] = list(plan.dc), list(plan.rgb)
    lay.degree, lay.rest_m = int(plan.degree), int(plan.m)
    for k in range(45):
        lay.rest_offset[k] = int(plan.rest[k]) if k < len(plan.rest) else -1
    lay.width, lay.height = int(cam.width), int(cam.height)
    lay.view[:] = [float(v) for v in np.asarray(cam.view, dtype=np.float64).reshape(12)]
    lay.eye[:] = [float(v) for v in cam.eye]
    lay.fx, lay.fy, lay.cx, lay.cy = cam.fx, cam.fy, cam.cx, cam.cy
    lay.tan_fovx, lay.tan_fovy, lay.near = cam.tan_fovx, cam.tan_fovy, cam.near
    lay.background[:] = [float(v) for v in plan.background]
    return lay


def render_table(data: np.ndarray, plan, stage_ms: "dict | None" = None, device: int = 0, info: "dict | None" = None) -> np.ndarray:
    """The image of a host table: the rows uploaded once (ResidentRows.from_host) and ResidentRows.render.  data: 1-D structured
    table of plan.dtype; the caller's array is left alone.  -> the (height, width, 3) uint8 image; `info` receives render_info.
    stage_ms: upload, the RENDER_STAGES clocks, download."""
    data = np.ascontiguousarray(data)
    if data.ndim != 1 or data.dtype != np.dtype(plan.dtype):
        raise ValueError("render_table: a 1-D table of %s" % np.dtype(plan.dtype))
    require_hip()
    with stage_clock(stage_ms, "upload"):
        rr = ResidentRows.from_host(data, device)
    try:
        image = rr.render(plan, stage_ms=stage_ms)
        if info is not None:
            info.update(rr.render_info)
        return image
    finally:
        rr.close()


def view_scores_table(data: np.ndarray, plans, stage_ms: "dict | None" = None, device: int = 0, info: "dict | None" = None):
    """The view scores of a host table: the rows uploaded once (ResidentRows.from_host) and ResidentRows.view_scores.  data: 1-D
    structured table of the plans' dtype; the caller's array is left alone.  -> (peak float32[n], total uint64[n]); `info`
    receives view_scores_info.  stage_ms: upload, the RENDER_STAGES clocks, download."""
    plans = list(plans)
    data = np.ascontiguousarray(data)
    if data.ndim != 1 or any(data.dtype != np.dtype(p.dtype) for p in plans):
        raise ValueError("view_scores_table: a 1-D table of the plans' dtype")
    require_hip()
    with stage_clock(stage_ms, "upload"):
        rr = ResidentRows.from_host(data, device)
    try:
        out = rr.view_scores(plans, stage_ms=stage_ms)
        if info is not None:
            info.update(rr.view_scores_info)
        return out
    finally:
        rr.close()


def view_keys_host(total: np.ndarray) -> np.ndarray:
    """gsx_view_keys_host: the ranking keys of summed contributions (uint64) -> uint32, smallest = most visible, 0 -> 0xffffffff
    (csrc/view_key.h, the function gsx_view_keys_dev runs).  No device is touched."""
    total = np.ascontiguousarray(total, dtype=np.uint64)
    keys = np.empty(total.shape, np.uint32)
    check(load().gsx_view_keys_host(total.ctypes.data, total.size, keys.ctypes.data), "gsx_view_keys_host")
    return keys


def image_compare_words(words) -> dict:
    """the nine words of gsx_image_compare_* -> dict(sse: three ints, windows, ssim: three ints -- the sums of the windows' 32.32
    fixed-point values), Python ints throughout"""
    w = [int(v) for v in words]
    return {"sse": tuple(w[0:3]), "windows": w[3], "ssim": tuple(w[4:7])}


def _image_pair(a, b, who: str):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != np.uint8 or b.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape != b.shape:
        raise ValueError("%s: two (height, width, 3) uint8 images of the same size" % who)
    h, w = a.shape[:2]
    if not (1 <= h <= FIDELITY_MAX_SIDE and 1 <= w <= FIDELITY_MAX_SIDE):
        raise ValueError("%s: an image of %d x %d (1 ... %d per side)" % (who, w, h, FIDELITY_MAX_SIDE))
    return a, b, w, h


def image_compare_dev(ctx: "Context", a_ptr: int, b_ptr: int, width: int, height: int, stage_ms: "dict | None" = None) -> dict:
    """gsx_image_compare_dev on two images that lie in HBM (height * width * 3 bytes each) -> image_compare_words.
    stage_ms["compare"]: the launch's stream clock, added."""
    words = (C.c_int64 * FIDELITY_WORDS)()
    clock = C.c_float(0.0) if stage_ms is not None else None
    check(ctx.lib.gsx_image_compare_dev(ctx.handle, a_ptr, b_ptr, int(width), int(height), words, C.byref(clock) if clock is not None else None),
          "gsx_image_compare_dev")
    if stage_ms is not None:
        stage_ms["compare"] = round(stage_ms.get("compare", 0.0) + float(clock.value), 3)
    return image_compare_words(words)


def image_compare(a: np.ndarray, b: np.ndarray, ctx: "Context | None" = None) -> dict:
    """The fidelity sums of two host images: both uploaded, one gsx_image_compare_dev on `ctx` (a context that
    lives for the call without one) -> dict(sse, windows, ssim).  For tests and small uses; fidelity.compare_rows compares
    images where the rasteriser left them."""
    a, b, w, h = _image_pair(a, b, "image_compare")
    require_hip()
    own = ctx is None
    ctx = Context() if own else ctx
    bufs = []
    try:
        for img in (a, b):
            bufs.append(ctx.alloc(img.nbytes))
            bufs[-1].upload(img)
        return image_compare_dev(ctx, bufs[0].ptr, bufs[1].ptr, w, h)
    finally:
        for buf in bufs:
            buf.free()
        if own:
            ctx.close()


def image_compare_host(a: np.ndarray, b: np.ndarray) -> dict:
    """gsx_image_compare_host: the same sums from the same per-window function on the host.  No device is touched."""
    a, b, w, h = _image_pair(a, b, "image_compare_host")
    words = (C.c_int64 * FIDELITY_WORDS)()
    check(load().gsx_image_compare_host(a.ctypes.data, b.ctypes.data, w, h, words), "gsx_image_compare_host")
    return image_compare_words(words)


def rows_decimate_table(data: np.ndarray, plan, zero_names=(), stage_ms: "dict | None" = None, device: int = 0):
    """The voxel decimation of a host table through the device: the rows uploaded once (ResidentRows.from_host), the device path
    of ResidentRows.decimate, and one download into a NEW table -- the caller's array is left alone.  data: 1-D structured table
    of plan.dtype.  -> (the table, decimate_info).  stage_ms: upload, the DECIMATE_STAGES clocks, download."""
    data = np.ascontiguousarray(data)
    if data.ndim != 1 or data.dtype != np.dtype(plan.dtype):
        raise ValueError("rows_decimate_table: a 1-D table of %s" % np.dtype(plan.dtype))
    if len(data) == 0:
        return data.copy(), {"groups": 0, "merged_groups": 0, "passed_through": 0}
    require_hip()
    with stage_clock(stage_ms, "upload"):
        rr = ResidentRows.from_host(data, device)
    out_rr = None
    try:
        out_rr = rr.decimate(plan, zero_names=zero_names, stage_ms=stage_ms)
        with stage_clock(stage_ms, "download"):
            out = out_rr.download()
        return out, out_rr.decimate_info
    finally:
        rr.close()
        if out_rr is not None:
            out_rr.close()


LIMIT_FIELDS = ("scale_0", "scale_1", "scale_2", "opacity")   # the fields of the splat budget's metric, in gsx_limit_keys_dev's order


def limit_count(max_count) -> int:
    """a splat budget as an int: ValueError for anything but an integer >= 1 (a bool and a float are no counts)"""
    if isinstance(max_count, (bool, np.bool_)) or not isinstance(max_count, (int, np.integer)) or int(max_count) < 1:
        raise ValueError(f"max_count must be an integer of at least 1. Got {max_count!r}.")
    return int(max_count)


def limit_info(info) -> dict:
    """gsx_limit_select_*'s three words -> dict(kept, threshold, ties_kept, threshold_key); threshold: the metric of the last
    row kept, float32(-sort_unkey(T)) (csrc/sog_math.h)"""
    key = int(info[0])
    bits = (key & 0x7fffffff) if key & 0x80000000 else (~key & 0xffffffff)
    return {"kept": int(info[2]), "threshold": -np.array([bits], np.uint32).view(np.float32)[0], "ties_kept": int(info[1]),
            "threshold_key": key}


def limit_columns_host(data: np.ndarray) -> np.ndarray:
    """(n, 4) float32: LIMIT_FIELDS of every row of a host table, one threaded pass (gsx_host_gather_f32) -- the array
    gsx_rows_columns_f32_dev writes for resident rows, gsx_limit_keys_dev's input"""
    return host_gather_xyz(data, LIMIT_FIELDS)


def limit_keys_dev(ctx: "Context", cols_ptr: int, n0: int, keys_ptr: int):
    """gsx_limit_keys_dev: (n0, 4) device columns -> n0 device keys.  Asynchronous."""
    check(ctx.lib.gsx_limit_keys_dev(ctx.handle, cols_ptr, int(n0), keys_ptr), "gsx_limit_keys_dev")


def limit_select_dev(ctx: "Context", keys_ptr: int, orig_ptr, n: int, max_count: int, mask_ptr: int) -> dict:
    """gsx_limit_select_dev: the mask of the `max_count` smallest keys among the chain's n rows at `mask_ptr` -> limit_info"""
    info = (C.c_uint32 * 3)()
    check(ctx.lib.gsx_limit_select_dev(ctx.handle, keys_ptr, orig_ptr, int(n), int(max_count), mask_ptr, info), "gsx_limit_select_dev")
    return limit_info(info)


def limit_select_host(keys: np.ndarray, max_count: int, orig: "np.ndarray | None" = None):
    """gsx_limit_select_host: the select's host twin (csrc/limit_select.h's digit walk and tie rule) on uint32 keys; orig: the
    ascending uint32 rows of `keys` the select runs over (None: all) -> (bool mask, one per selected row; limit_info).  No
    device is touched."""
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    if orig is not None:
        orig = np.ascontiguousarray(orig, dtype=np.uint32)
    n = len(keys) if orig is None else len(orig)
    mask = np.zeros(n, np.uint8)
    info = (C.c_uint32 * 3)()
    check(load().gsx_limit_select_host(keys.ctypes.data, orig.ctypes.data if orig is not None else None, n, int(max_count),
                                       mask.ctypes.data, info), "gsx_limit_select_host")
    return mask.view(np.bool_), limit_info(info)


def limit_mask(columns4: np.ndarray, max_count: int, device: int = 0) -> dict:
    """The splat budget on host columns, for the eager DataProcessor (sor_filter's place in remove_flyers): columns4, the (n, 4)
    float32 LIMIT_FIELDS of a table, uploaded once, gsx_limit_keys_dev and gsx_limit_select_dev there, and the n mask bytes
    back -> limit_info and mask (bool[n]) for host_compact_rows.  One ArenaSession of the "limit" lease group."""
    max_count = limit_count(max_count)
    cols = np.ascontiguousarray(columns4, dtype=np.float32)
    if cols.ndim != 2 or cols.shape[1] != 4:
        raise ValueError("limit_mask: an (n, 4) array of scale_0, scale_1, scale_2, opacity")
    n = len(cols)
    if n == 0:
        return dict(limit_info((0, 0, 0)), mask=np.zeros(0, np.bool_))
    require_hip()
    with ArenaSession("limit", device) as s:
        d_cols, d_keys, d_mask = s.buf("cols", 16 * n), s.buf("keys", 4 * n), s.buf("mask", n + 16)
        d_cols.upload(cols)
        limit_keys_dev(s.ctx, d_cols.ptr, n, d_keys.ptr)
        out = limit_select_dev(s.ctx, d_keys.ptr, None, n, max_count, d_mask.ptr)
        out["mask"] = d_mask.download(np.uint8, n).view(np.bool_)
    return out


def dev_patch_u8(ctx: "Context", dst_ptr: int, dst_len: int, idx: np.ndarray, val: np.ndarray):
    """gsx_dev_patch_u8: dst[idx[i]] = val[i] on the device, from host arrays"""
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    val = np.ascontiguousarray(val, dtype=np.uint8)
    assert idx.shape == val.shape and idx.ndim == 1
    check(ctx.lib.gsx_dev_patch_u8(ctx.handle, dst_ptr, int(dst_len), idx.ctypes.data, val.ctypes.data, len(idx)), "gsx_dev_patch_u8")


def resident_rgb_dev(ctx: "Context", rr: "ResidentRows", names3, d_fdc, d_rgb, d_list, d_cnt):
    """add_rgb_from_sh's colours (data_processor.py:316-343) of resident rows, left in HBM: the three f_dc fields through
    gsx_rows_columns_f32_dev into `d_fdc` (12 n bytes), gsx_rgb_from_sh_list_dev into `d_rgb` (3 n bytes), then numpy's own bytes
    for the listed, uncertain elements -- their f_dc words come back in one small download each -- through gsx_dev_patch_u8.
    d_list: 4 (3 n // 64 + 4096) bytes, d_cnt: 16.  -> the number of patched elements, or None when the list overflowed (NaNs by
    the million: the caller takes the host path for the colours)"""
    n3 = 3 * rr.n
    cap = n3 // 64 + 4096
    rows_columns_dev(ctx, rr.ptr, rr.first_byte, rr.dtype, rr.n, names3, d_fdc.ptr)
    check(ctx.lib.gsx_rgb_from_sh_list_dev(ctx.handle, d_fdc.ptr, n3, d_rgb.ptr, d_list.ptr, cap, d_cnt.ptr), "gsx_rgb_from_sh_list_dev")
    cnt = int(d_cnt.download(np.uint32, 1)[0])
    if cnt > cap:
        return None
    if cnt:
        idx = np.sort(d_list.download(np.uint32, cnt))
        # the listed words, gathered on the device into the list's own buffer (a (cnt, 1) column of 4-byte "rows")
        d_val = d_list.ptr + ((4 * cnt + 15) & ~15)
        if 4 * cnt + 16 + 4 * cnt <= d_list.nbytes:
            d_list.upload(idx)
            rows_take_dev(ctx, d_fdc.ptr, 0, 4, n3, d_list.ptr, cnt, (), None, 0, d_val)
            v = d_list.download_at(d_val - d_list.ptr, np.float32, cnt)
        else:
            v = d_fdc.download(np.float32, n3)[idx]
        with np.errstate(all="ignore"):
            lin = np.clip(0.5 + v * 0.28209479177387814, 0.0, 1.0)
            dev_patch_u8(ctx, d_rgb.ptr, n3, idx, (np.power(lin, 1.0 / 2.2) * 255).astype(np.uint8))
    return cnt


def pack_listed(s: "ArenaSession", n: int, run):
    """run(d_list, cap, d_cnt) launches a packer that lists the entries it leaves to numpy in d_list, `cap` of them at most, and
    counts all of them in d_cnt.  More listed entries than room: once more, with room for every one of them.
    -> (d_list, count); listed_rows() downloads them"""
    cap = n // 64 + 4096
    d_list, d_cnt = s.buf("list", 8 * cap), s.buf("count", 16)
    run(d_list, cap, d_cnt)
    cnt = int(d_cnt.download(np.uint32, 1)[0])
    if cnt > cap:
        d_list = s.buf("list", 8 * cnt)
        run(d_list, cnt, d_cnt)
        cnt = int(d_cnt.download(np.uint32, 1)[0])
    return d_list, cnt


def listed_rows(d_list, cnt: int) -> np.ndarray:
    """-> the (cnt, 2) uint32 entries a packer listed"""
    return d_list.download(np.uint32, 2 * cnt).reshape(cnt, 2) if cnt else np.zeros((0, 2), np.uint32)


def read_exact(f, view, path: str, where: str = "", unit: str = "bytes"):
    """fill the writable buffer `view` from the open binary file `f`, or ValueError about the file's early end"""
    view = memoryview(view)
    got = 0
    while got < len(view):
        r = f.readinto(view[got:])
        if not r:
            raise ValueError("%s: early end of file%s (%d of %d %s)" % (path, where, got, len(view), unit))
        got += r


def read_file(path: str, offset: int, view, where: str = "", unit: str = "bytes"):
    """read_exact() from byte `offset` of the file `path`"""
    with open(path, "rb") as f:
        f.seek(int(offset))
        read_exact(f, view, path, where, unit)


def cply_pack_table(data: np.ndarray, sh_names, order: "np.ndarray | None" = None, ctx: "Context | None" = None, stage_ms: "dict | None" = None):
    """The compressed-PLY writer's numeric core on a whole splat table (formats/compressed_ply.py:200-297).  Round 6: the raw rows
    are uploaded ONCE (gsx_dev_upload_staged) and the Morton sort, the chunk packers and the SH packer read their fields straight
    out of them (element stride = row_bytes / 4: gsx_cply_pack_strided_dev / gsx_cply_sh_strided_dev) -- round 5 gathered the 59
    columns on the host (one threaded pass, 472 MB of freshly faulted pages per 2M splats) and uploaded that.  The alpha byte comes
    from the opacity field on the device (float64 exp + the rounding certificate of the SOG textures; numpy's own sigmoid only for
    the ~1e-4 listed splats: gsx_cply_pack_opacity_dev); results come back through the staging lanes.  Tables the row path does not take (views that
    are not C-contiguous, rows that are not a multiple of 4 bytes, f_rest fields that are not consecutive) and calls with a caller's
    context gather their columns on the host as before.  A field the writer reads that is not float32 raises TypeError before the
    device is touched (the reference computes in the field's dtype); big-endian float32 fields are made little-endian first.
    -> (chunks (ceil(n/256), 18) f32, vertices (n, 4) u32, sh (n, m) u8 or None, order u32[n], recursion levels or None)"""
    reads = ["opacity" if c == "alpha" else c for c in CPLY_COLUMNS] + ["f_rest_%d" % i for i in range(45)]
    require_f4_fields(data, reads, "Compressed PLY writer")
    data = native_f4(data, reads)
    lib = require_hip()
    n = len(data)
    fields = data.dtype.fields or {}
    # sh_names: the list itself, or a function (highest f_rest index holding a non-zero | None) -> list: the writer's degree
    # detection (compressed_ply.py:139-171), which on resident rows takes the index from ONE device pass (gsx_fields_nonzero_dev)
    # instead of numpy's `np.any(data[f] != 0)` per strided column (~0.1 s each at 10M splats: more than this whole function)
    resolve = sh_names if callable(sh_names) else None
    present = [i for i in range(45) if "f_rest_%d" % i in fields]
    sh_names = ["f_rest_%d" % i for i in present] if resolve else list(sh_names)
    m = len(sh_names)
    base_names = ["opacity" if c == "alpha" else c for c in CPLY_COLUMNS]
    names = base_names + sh_names
    # (rows that are not a multiple of 4 bytes -- three u1 colour fields behind the floats: 251 -- are copied to 252-byte rows ON the
    #  device after the upload: gsx_rows_repack_dev, ~2 ms per 10M rows)
    resident = (ctx is None and n >= 1024 and data.ndim == 1 and data.flags.c_contiguous
                and all(nm in fields and fields[nm][0] == np.dtype("<f4") and fields[nm][1] % 4 == 0 for nm in names)
                and all(fields[sh_names[i]][1] == fields[sh_names[0]][1] + 4 * i for i in range(m)))
    if resolve and not resident:
        sh_names = list(resolve(None))          # the host's own scan
        m = len(sh_names)
        names = base_names + sh_names
    nchunks = (n + 255) // 256
    # only resident rows go to the arena (the "cply" lease, ArenaSession); a caller's context is used as it is
    with ArenaSession("cply", 0, stage_ms, ctx=ctx, shared=resident) as s:
        ctx = s.ctx
        verts = np.empty((n, 4), np.uint32)
        sh = np.empty((n, m), np.uint8) if m and not (resolve and resident) else None
        large = resident and n >= (1 << 18)
        joins = [prefault(large, verts, sh)]
        if resident:
            pitch = (data.dtype.itemsize + 3) & ~3
            rd = pitch // 4
            d_rows = s.upload_rows(lib, data, slack=16)
            if pitch != data.dtype.itemsize:
                d_raw, d_rows = d_rows, s.buf("rows_aligned", n * pitch)
                check(lib.gsx_rows_repack_dev(ctx.handle, d_raw.ptr, data.dtype.itemsize, n, d_rows.ptr, pitch), "gsx_rows_repack_dev")
                s.mark("repack")
            if resolve:
                word = C.c_uint64(0)
                if m:
                    check(lib.gsx_fields_nonzero_dev(ctx.handle, d_rows.ptr + int(fields[sh_names[0]][1]), rd, n, m, C.byref(word)),
                          "gsx_fields_nonzero_dev")
                active = [present[j] for j in range(m) if (word.value >> j) & 1]
                sh_names = list(resolve(max(active) if active else -1))
                m = len(sh_names)
                names = base_names + sh_names
                sh = np.empty((n, m), np.uint8) if m else None
                joins.append(prefault(large, sh))
                s.mark("sh_detect")
            # (round 6: the sigmoid's byte is decided on the device from the opacity field, with a rounding certificate; numpy only
            #  evaluates the listed ~1e-4 of the splats, below)
            col = lambda i: d_rows.ptr + int(fields[names[i]][1])
            strides = (_I64 * 14)(*([rd] * 14))
            xyz_stride, sh_ptr, sh_col_stride, sh_elem_stride = rd, (d_rows.ptr + int(fields[sh_names[0]][1])) if m else None, 1, rd
        else:
            mat = host_gather_columns(data, names)                     # (14 + m, n), row 9 = opacity
            with np.errstate(over="ignore"):
                mat[9] = 1.0 / (1.0 + np.exp(-mat[9]))                 # :200-203 (float32 in, float32 out, as in the reference)
            d_mat = s.buf("mat", max(mat.nbytes, 16))
            d_mat.upload(mat)
            col = lambda i: d_mat.ptr + 4 * n * i
            strides = (_I64 * 14)(*([1] * 14))
            xyz_stride, sh_ptr, sh_col_stride, sh_elem_stride = 1, col(14), n, 1
        levels = None
        d_order = s.buf("order", 4 * n)
        if order is None:
            lv = C.c_int()
            check(lib.gsx_morton_order_dev(ctx.handle, col(0), col(1), col(2), xyz_stride, n, d_order.ptr, C.byref(lv)), "gsx_morton_order_dev")
            levels = int(lv.value)
            s.mark("morton")
            order = d_order.download(np.uint32, n) if n else np.zeros(0, np.uint32)
        else:
            order = np.ascontiguousarray(order, dtype=np.uint32)
            d_order.upload(order)
        ptrs = (C.c_void_p * 14)(*[col(i) for i in range(14)])
        d_chunk, d_vert = s.buf("chunk", 72 * nchunks), s.buf("vert", 16 * n)
        unc_cap = n // 64 + 4096
        d_list, d_cnt = (s.buf("unc", 8 * unc_cap), s.buf("unc_count", 16)) if resident else (None, None)
        check(lib.gsx_cply_pack_opacity_dev(ctx.handle, ptrs, strides, d_order.ptr, n, d_chunk.ptr, d_vert.ptr, d_list.ptr if resident else None,
                                            unc_cap if resident else 0, d_cnt.ptr if resident else None), "gsx_cply_pack_opacity_dev")
        d_out = None
        if m:
            d_out = s.buf("sh", n * m)
            check(lib.gsx_cply_sh_strided_dev(ctx.handle, sh_ptr, m, sh_col_stride, sh_elem_stride, d_order.ptr, n, d_out.ptr), "gsx_cply_sh_strided_dev")
        s.mark("pack")
        chunks = d_chunk.download(np.float32, 18 * nchunks).reshape(nchunks, 18)
        for join in joins:
            join()
        dl = lib.gsx_dev_download_staged if resident else lib.gsx_dev_download
        if n:
            check(dl(ctx.handle, verts.ctypes.data, d_vert.ptr, verts.nbytes), "gsx_dev_download")
            if m:
                check(dl(ctx.handle, sh.ctypes.data, d_out.ptr, sh.nbytes), "gsx_dev_download")
        s.mark("download")
        if resident:
            m_unc = int(d_cnt.download(np.uint32, 1)[0])
            if m_unc > unc_cap:      # (thousands of opacities beyond +-80, or NaNs: numpy's expression for the whole column)
                pos = np.arange(n, dtype=np.int64)
                x = np.ascontiguousarray(data["opacity"])[order]
            else:
                lst = listed_rows(d_list, m_unc)
                pos, x = lst[:, 0].astype(np.int64), lst[:, 1].copy().view(np.float32)
            if len(pos):
                with np.errstate(all="ignore"):
                    a = 1.0 / (1.0 + np.exp(-x))                                               # :200-203
                    byte = np.clip(np.floor(a * 255 + 0.5), 0, 255).astype(np.uint32)       # :312
                verts[pos, 3] = (verts[pos, 3] & np.uint32(0xffffff00)) | byte
            s.mark("host_patch")
        return chunks, verts, sh, order, levels


def spz_pack_table(data: np.ndarray, sh_degree, scan_fields=(), stage_ms: "dict | None" = None, listed: "dict | None" = None,
                   device: int = 0):
    """The SPZ writer's body on a whole splat table (formats/spz.py:49-173, :298-343): the raw rows are uploaded ONCE through the
    staging lanes, the SH-degree scan and the packer read their fields straight out of them (any row size up to 512 bytes, fields
    at any byte offset), and the body comes back through the staging lanes into the buffer the file is written from.

    data: 1-D C-contiguous structured table whose fields named in SOG_FIELD_NAMES are little-endian float32 where present, with
    x y z, scale_0..2 and rot_0..3 among them (formats/spz_writer.py checks).  sh_degree: the degree, or a function (highest
    f_rest index of `scan_fields` holding a value != 0, -1 for none) -> degree, answered by one device pass over the resident rows.
    listed: a dict that receives the rows whose alpha byte ("alpha") or rotation word ("rotation") numpy evaluated.
    -> (out, degree): out = uint8[16 + (20 + 3 sh_dim) n], the body behind SPZ_HEADER_BYTES left for the caller's header.

    One ArenaSession of the "spz" lease group."""
    lib = require_hip()
    n = len(data)
    data = narrow_rows(data)
    with ArenaSession("spz", device, stage_ms) as s:
        ctx = s.ctx
        lay = spz_layout(data.dtype)
        d_rows = s.upload_rows(lib, data)
        degree = sh_degree
        if callable(sh_degree):
            word = rest_nonzero_word(lib, ctx, d_rows, lay, n, scan_fields)
            hit = [int(i) for i in scan_fields if (word >> int(i)) & 1]
            degree = int(sh_degree(max(hit) if hit else -1))
            s.mark("sh_detect")
        body_bytes = (20 + 3 * SPZ_SH_DIM[degree]) * n
        out = np.empty(SPZ_HEADER_BYTES + body_bytes, np.uint8)
        join = prefault(body_bytes >= (1 << 22), out)
        d_body = s.buf("body", body_bytes)

        def pack(d_list, cap, d_cnt):
            check(lib.gsx_spz_pack_dev(ctx.handle, d_rows.ptr, C.byref(lay), n, degree, d_body.ptr, d_list.ptr, cap, d_cnt.ptr),
                  "gsx_spz_pack_dev")
        d_list, cnt = pack_listed(s, n, pack)
        s.mark("pack")
        join()
        if body_bytes:
            check(lib.gsx_dev_download_staged(ctx.handle, out.ctypes.data + SPZ_HEADER_BYTES, d_body.ptr, body_bytes), "gsx_dev_download_staged")
        lst = listed_rows(d_list, cnt)
        s.mark("download")
        a_rows = lst[lst[:, 1] == 0, 0].astype(np.int64)
        r_rows = lst[lst[:, 1] == 1, 0].astype(np.int64)
        body = out[SPZ_HEADER_BYTES:]
        if len(a_rows):
            body[9 * n + a_rows] = spz_alpha_bytes(data["opacity"][a_rows])
        if len(r_rows):
            q = np.column_stack([data["rot_%d" % c][r_rows] for c in range(4)])
            spz_patch_rotations(body[16 * n:20 * n].view("<u4"), r_rows, q)
        if cnt:
            s.mark("host_patch")
        if listed is not None:
            listed["alpha"], listed["rotation"] = a_rows, r_rows
        return out, degree


KSPLAT_HEADER_BYTES = 4096 + 1024   # file header + the one section header (ksplat.py:370-413)
KSPLAT_SH_C0 = 0.28209479177387814  # ksplat.py:478


def ksplat_row_dtype(level: int, sh_count: int) -> np.dtype:
    """one interleaved .ksplat row (ksplat.py:502-515); level: 0, 1, 2, or 3 for every level >= 3"""
    if level == 0:
        fields = [("pos", "<f4", (3,)), ("scale", "<f4", (3,)), ("rot", "<f4", (4,)), ("color", "u1", (4,))]
        sh = "<f4"
    else:
        fields = [("pos", "<u2", (3,)), ("scale", "<f2", (3,)), ("rot", "<f2", (4,)), ("color", "u1", (4,))]
        sh = "<f2" if level == 1 else "u1"
    if sh_count:
        fields.append(("sh", sh, (sh_count,)))
    return np.dtype(fields)


def ksplat_exp_fields(data: np.ndarray, rows, level: int):
    """ksplat.py:464-468 and :482 with numpy's own exp, for `rows` -> (scales (m, 3) float32 / float16, alpha uint8[m])"""
    with np.errstate(all="ignore"):
        s = np.column_stack([np.exp(data["scale_%d" % a][rows]) for a in range(3)])
        a = np.clip((1 / (1 + np.exp(-data["opacity"][rows]))) * 255, 0, 255).astype(np.uint8)
        return (s if level == 0 else s.astype(np.float16)), a


def ksplat_rows_host(data: np.ndarray, rows, level: int, sh_count: int, centres: "np.ndarray | None", bucket_size: int,
                     sf_inv: float) -> np.ndarray:
    """ksplat.py:452-536 with numpy's own expressions for the rows the device lists -> their interleaved rows
    (ksplat_row_dtype).  centres: (n_buckets, 3) float32, final (levels >= 1); sf_inv: the Python float of :452."""
    rows = np.asarray(rows, dtype=np.int64)
    out = np.zeros(len(rows), ksplat_row_dtype(level, sh_count))
    with np.errstate(all="ignore"):
        xyz = np.column_stack([data[a][rows] for a in "xyz"])
        if level == 0:
            out["pos"] = xyz
        else:
            c = centres[rows // bucket_size]
            out["pos"] = np.clip(np.round((xyz - c) * sf_inv) + 32767, 0, 65535).astype(np.uint16)
        out["scale"], alpha = ksplat_exp_fields(data, rows, level)
        out["rot"] = np.column_stack([data["rot_%d" % a][rows] for a in range(4)]).astype(out.dtype["rot"].base)
        rgb = [np.clip((0.5 + KSPLAT_SH_C0 * data["f_dc_%d" % a][rows]) * 255, 0, 255).astype(np.uint8) for a in range(3)]
        out["color"] = np.column_stack(rgb + [alpha])
        if sh_count:
            sh = np.stack([data["f_rest_%d" % j][rows] for j in range(sh_count)], axis=1)
            if level == 2:
                out["sh"] = np.clip((sh - -2.0) / (2.0 - -2.0) * 255, 0, 255).astype(np.uint8)
            else:                          # levels >= 3 cast the values themselves (ksplat.py:527-533)
                out["sh"] = sh.astype(out.dtype["sh"].base)
    return out


def ksplat_centres_host(data: np.ndarray, bucket_size: int) -> np.ndarray:
    """ksplat.py:428-444 with numpy's own reductions (its order decides the sign of an all-zero bucket's centre) -> (nb, 3)"""
    idx = np.arange(0, len(data), bucket_size)
    cols = []
    with np.errstate(all="ignore"):
        for a in "xyz":
            v = data[a]
            cols.append((np.minimum.reduceat(v, idx) + np.maximum.reduceat(v, idx)) / 2.0)
    return np.column_stack(cols).astype(np.float32)


def grid_points_per_cell(k: int, n: int, tuned: bool) -> float:
    """csrc/grid_policy.h: grid_pts_per_cell (tuned) or grid_pts_per_cell_base; no GPU needed"""
    return float(load().gsx_sor_debug_points_per_cell(int(k), int(n), int(bool(tuned))))


def grid_group_bricks(bricks, nbx: int, nby: int, nbz: int):
    """csrc/grid_policy.h: group_deferred_bricks -> (the list rewritten group by group, the groups' sizes); no GPU needed"""
    b = np.array(bricks, dtype=np.uint32)
    sizes = np.zeros(8, np.uint32)
    ng = C.c_int32()
    check(load().gsx_sor_debug_group_bricks(b.ctypes.data, b.size, int(nbx), int(nby), int(nbz), sizes.ctypes.data, C.byref(ng)),
          "gsx_sor_debug_group_bricks")
    return b, [int(v) for v in sizes[:ng.value]]


def grid_refine_sizing(qb_lo, qb_hi, sub_queries: int, n_sub: int, pts_per_cell: float, parent_h: float, adaptive: int, hist,
                       bin_vol: float) -> RefineSizingOut:
    """csrc/grid_policy.h: refine_clip + refine_probe_edge for one group of deferred bricks; no GPU needed"""
    a = RefineSizingIn((C.c_float * 3)(*qb_lo), (C.c_float * 3)(*qb_hi), int(sub_queries), int(n_sub), float(pts_per_cell),
                       float(parent_h), int(adaptive), (C.c_uint32 * 32)(*[int(v) for v in hist]), float(bin_vol))
    out = RefineSizingOut()
    check(load().gsx_sor_debug_refine_sizing(C.byref(a), C.byref(out)), "gsx_sor_debug_refine_sizing")
    return out


def np_exp_host(x: np.ndarray) -> np.ndarray:
    """csrc/np_exp.h on the host (gsx_np_expf_host): the twin of the device's exp"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(x)
    check(load().gsx_np_expf_host(x.ctypes.data, out.ctypes.data, x.size), "gsx_np_expf_host")
    return out


def np_exp_probe_vector() -> np.ndarray:
    """~64K float32 inputs: the hard case 0xc2781e37, both ends of numpy's range (+inf above 0x1.62e430p+6, +0 below
    -0x1.9fe368p+6) and their neighbours, denormal results, |x| near 0, NaN / +-inf / +-0, uniform values and raw bit patterns"""
    rng = np.random.default_rng(0x6B73)
    f = np.float32
    edges = []
    for e in (f(88.72283935546875), f(-103.972084045410156), f(-87.33654), f(0.0)):
        v = e
        for _ in range(64):
            v = np.nextafter(v, f(-np.inf), dtype=np.float32)
        for _ in range(129):
            edges.append(v)
            v = np.nextafter(v, f(np.inf), dtype=np.float32)
    bits = np.array([0xC2781E37, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0, 0x00000001, 0x7F7FFFFF,
                     0xFF7FFFFF], np.uint32).view(np.float32)
    parts = [bits, np.array(edges, np.float32),
             rng.uniform(-103.98, -87.3, 12288).astype(np.float32),             # denormal and smallest normal results
             rng.uniform(-110.0, 90.0, 24576).astype(np.float32),
             rng.uniform(-1e-3, 1e-3, 4096).astype(np.float32),
             rng.integers(0, 1 << 32, 16384, dtype=np.uint64).astype(np.uint32).view(np.float32)]
    return np.concatenate(parts)


_np_exp_checked = None
NP_PROBE_FALLBACK = {"exp": "the .ksplat and .splat writers take every exp-derived value from numpy on the host",
                     "log": "the .splat reader takes the scales from numpy on the host"}


def np_probe(name: str) -> bool:
    """np_exp_probe and np_log_probe, `name` = "exp" / "log": numpy's float32 function against its host twin np_<name>_host on
    np_<name>_probe_vector(), once per process (the verdict: _np_<name>_checked).  On a mismatch, with the first differing
    input: a RuntimeWarning and False, or under GSX_STRICT_NUMPY=1 a GsxError and the verdict forgotten.  The twin, the vector
    and the verdict are looked up by name at the call: the tests replace them in this module."""
    g, slot = globals(), "_np_%s_checked" % name
    if g[slot] is not None:
        return g[slot]
    import warnings
    x = g["np_%s_probe_vector" % name]()
    with np.errstate(all="ignore"):
        want = getattr(np, name)(x).view(np.uint32)
    got = g["np_%s_host" % name](x).view(np.uint32)
    bad = np.nonzero(got != want)[0]
    if len(bad):
        i = int(bad[0])
        msg = ("numpy %s's float32 %s differs from the one libgsx_hip reproduces (numpy 2.x's AVX512F / AVX2 routine) on %d of %d "
               "probe inputs (first: x=0x%08x -> device 0x%08x, numpy 0x%08x): %s.  GSX_STRICT_NUMPY=1 turns this warning into an error."
               % (np.__version__, name, len(bad), len(x), int(x.view(np.uint32)[i]), int(got[i]), int(want[i]), NP_PROBE_FALLBACK[name]))
        if os.environ.get("GSX_STRICT_NUMPY") == "1":
            raise GsxError(msg)
        warnings.warn(msg, RuntimeWarning, stacklevel=3)
    g[slot] = not len(bad)
    return g[slot]


def np_exp_probe() -> bool:
    """The .ksplat and .splat writers store np.exp's float32 bits, so the device's exp (csrc/np_exp.h) must be THIS process's
    numpy's: np_probe("exp").  False: the writer takes every exp-derived result -- scales, alpha -- from numpy on the host, and
    stays exact."""
    return np_probe("exp")


def ksplat_pack_table(data: np.ndarray, degree, scan_fields, geometry, stage_ms: "dict | None" = None, listed: "dict | None" = None,
                      device: int = 0):
    """The .ksplat writer's payload on a whole splat table (formats/ksplat.py:319-544): the raw rows are uploaded ONCE, the SH-degree
    scan (gsx_spz_rest_nonzero_dev), the bucket centres and the row packer read their fields straight out of them, and the payload
    comes back into the buffer the file is written from.

    data: 1-D C-contiguous structured table, its fields in SOG_FIELD_NAMES little-endian float32 where present
    (formats/ksplat_writer.py checks).  degree: the SH degree, or a function (bits of the f_rest fields in scan_fields holding a
    value != 0) -> degree.  geometry(degree) -> (out, g): the whole file's buffer with both headers (and the first payload word)
    written, and a dict with level (0 / 1 / 2), sh_count, bucket_size, sf_inv, n_buckets, row_base, payload_bytes, head (the
    first payload word's bytes); it may raise (the reference's struct errors) before anything is packed.
    listed: a dict that receives the rows ("rows") and buckets ("buckets") numpy evaluated, and "exp_host" (True when the numpy
    probe failed and every scale and alpha came from numpy).  -> (out, degree)

    One ArenaSession of the "ksplat" lease group."""
    lib = require_hip()
    n = len(data)
    exp_ok = np_exp_probe()
    src = data                               # the caller's table: numpy's host patches run on it, as the reference's expressions do
    data = narrow_rows(data)
    with ArenaSession("ksplat", device, stage_ms) as s:
        ctx = s.ctx
        lay = spz_layout(data.dtype)
        d_rows = s.upload_rows(lib, data)
        if callable(degree):
            degree = int(degree(rest_nonzero_word(lib, ctx, d_rows, lay, n, scan_fields)))
            s.mark("sh_detect")
        out, g = geometry(degree)
        level, sh_count, bs, nb, row_base = g["level"], g["sh_count"], g["bucket_size"], g["n_buckets"], g["row_base"]
        pay = out[KSPLAT_HEADER_BYTES:]
        join = prefault(pay.nbytes >= (1 << 22), pay)
        d_pay = s.buf("payload", g["payload_bytes"] + 64)
        centres_ptr = d_pay.ptr + len(g["head"])

        def pack(d_list, cap, d_cnt):
            check(lib.gsx_dev_memset(ctx.handle, d_cnt.ptr, 0, 4), "gsx_dev_memset")
            if level >= 1 and n:
                check(lib.gsx_ksplat_centres_dev(ctx.handle, d_rows.ptr, C.byref(lay), n, bs, centres_ptr, d_list.ptr, cap, d_cnt.ptr),
                      "gsx_ksplat_centres_dev")
                s.mark("centres")
            check(lib.gsx_ksplat_pack_dev(ctx.handle, d_rows.ptr, C.byref(lay), n, level, sh_count, bs if level else 1, g["sf_inv"],
                                          centres_ptr if level else None, d_pay.ptr, row_base, d_list.ptr, cap, d_cnt.ptr),
                  "gsx_ksplat_pack_dev")
        d_list, cnt = pack_listed(s, n, pack)
        s.mark("pack")
        join()
        if g["payload_bytes"]:
            check(lib.gsx_dev_download_staged(ctx.handle, pay.ctypes.data, d_pay.ptr, g["payload_bytes"]), "gsx_dev_download_staged")
        pay[:len(g["head"])] = np.frombuffer(g["head"], np.uint8)
        lst = listed_rows(d_list, cnt)
        s.mark("download")
        rows = lst[lst[:, 1] == 0, 0].astype(np.int64)
        buckets = np.unique(lst[lst[:, 1] == 2, 0].astype(np.int64))
        body = pay[row_base:row_base + n * ksplat_row_dtype(level, sh_count).itemsize].view(ksplat_row_dtype(level, sh_count))
        cen = None
        if level >= 1 and (len(rows) or len(buckets)):
            cen = pay[len(g["head"]):row_base].view("<f4").reshape(nb, 3)
        if len(buckets):
            cen[buckets] = ksplat_centres_host(src, bs)[buckets]
            starts = buckets * bs
            rows = np.concatenate([rows] + [np.arange(a, min(a + bs, n)) for a in starts])
        if not exp_ok and n:               # the probe found another exp: every exp-derived result from numpy
            body["scale"], body["color"][:, 3] = ksplat_exp_fields(src, slice(None), level)
        if len(rows):
            rows = np.unique(rows)
            body[rows] = ksplat_rows_host(src, rows, level, sh_count, cen, bs, g["py_sf_inv"])
        if cnt or not exp_ok:
            s.mark("host_patch")
        if listed is not None:
            listed["rows"], listed["buckets"], listed["exp_host"] = rows, buckets, not exp_ok
        return out, degree


SPLAT_RECORD = np.dtype([("pos", "<f4", (3,)), ("scale", "<f4", (3,)), ("color", "u1", (4,)), ("rot", "u1", (4,))])   # splat.py:155-160


def splat_metric_host(data: np.ndarray) -> np.ndarray:
    """splat.py:92-94 with numpy's own exp: the float32 visibility metric of every row"""
    with np.errstate(all="ignore"):
        return np.exp((data["scale_0"] + data["scale_1"]) + data["scale_2"]) * (1 / (1 + np.exp(-data["opacity"])))


def splat_pack_table(data: np.ndarray, rgb: bool = False, stage_ms: "dict | None" = None, listed: "dict | None" = None,
                     variant: str = "pack", device: int = 0, resident: "ResidentRows | None" = None) -> np.ndarray:
    """The .splat writer's whole file on a splat table (formats/splat.py:82-166): the raw rows are uploaded ONCE; one device pass
    keys every row by -metric and packs its 32-byte record in input order (gsx_splat_pack_dev), a stable radix sort orders the
    keys (gsx_splat_order_dev) and the records are permuted into that order (gsx_splat_permute_dev) -> uint8[32 n], the file.

    data: 1-D structured table, x y z, scale_0..2, rot_0..3, opacity and (rgb False) f_dc_0..2 little-endian float32, or (rgb
    True) the u1 fields red, green, blue (formats/splat_writer.py checks).  variant "gather": the sort-first alternative (keys
    pass, sort, records gathered from the raw rows in sorted order), kept for the measurement of tools/probe_splat.py.
    listed: a dict that receives "exp_host" (True when the numpy probe failed: the metric, the scales and alpha then come from
    numpy, the sort and the rest from the device).  resident: the rows of `data` in HBM (ResidentRows, the caller's; the same
    count and dtype, rows of up to 512 bytes from byte 0 of their buffer): the kernels read them where they are, nothing is
    uploaded and stage_ms has no "upload".  Everything the host computes (the numpy-exp branch) still reads `data`.

    One ArenaSession of the "splat" lease group."""
    lib = require_hip()
    n = len(data)
    exp_ok = np_exp_probe()
    if not (resident_matches(resident, data) and resident.first_byte == 0 and resident.device == device):
        resident = None
    src = data
    data = narrow_rows(data, ("red", "green", "blue") if rgb else ())
    fields = data.dtype.fields
    colour = [int(fields[c][1]) for c in ("red", "green", "blue")] if rgb else [-1, -1, -1]
    with ArenaSession("splat", device, stage_ms) as s:
        ctx = s.ctx
        out = np.empty(32 * n, np.uint8)
        if n == 0:
            return out
        join = prefault(out.nbytes >= (1 << 22), out)
        lay = spz_layout(data.dtype)
        d_rows = s.upload_rows(lib, data, resident=resident)    # (resident rows: 16 readable bytes behind the last one)
        d_keys, d_order = s.buf("keys", 4 * n), s.buf("order", 4 * n)
        d_recs, d_out = s.buf("recs", 32 * n), s.buf("out", 32 * n)

        def pack(order, keys, recs):
            check(lib.gsx_splat_pack_dev(ctx.handle, d_rows.ptr, C.byref(lay), *colour, n, order, keys, recs), "gsx_splat_pack_dev")
        if variant == "gather":
            pack(None, d_keys.ptr, None)
            s.mark("keys")
        else:
            pack(None, d_keys.ptr, d_recs.ptr)
            s.mark("key_pack")
        if not exp_ok:                       # another exp than numpy's: numpy's metric, keyed and sorted on the device
            d_metric = s.buf("metric", 4 * n)
            d_metric.upload(np.ascontiguousarray(splat_metric_host(src), np.float32))
            check(lib.gsx_splat_keys_dev(ctx.handle, d_metric.ptr, n, d_keys.ptr), "gsx_splat_keys_dev")
            s.mark("host_metric")
        check(lib.gsx_splat_order_dev(ctx.handle, d_keys.ptr, n, d_order.ptr), "gsx_splat_order_dev")
        s.mark("sort")
        if variant == "gather":
            pack(d_order.ptr, None, d_out.ptr)
            s.mark("gather_pack")
        else:
            check(lib.gsx_splat_permute_dev(ctx.handle, d_recs.ptr, d_order.ptr, n, d_out.ptr), "gsx_splat_permute_dev")
            s.mark("permute")
        join()
        check(lib.gsx_dev_download_staged(ctx.handle, out.ctypes.data, d_out.ptr, out.nbytes), "gsx_dev_download_staged")
        s.mark("download")
        if not exp_ok:                       # the exp-derived bytes (scales, alpha) from numpy, in the device's order
            order = d_order.download(np.uint32, n).astype(np.int64)
            rec = out.view(SPLAT_RECORD)
            with np.errstate(all="ignore"):
                rec["scale"] = np.column_stack([np.exp(src["scale_%d" % a][order]) for a in range(3)])
                rec["color"][:, 3] = np.clip((1 / (1 + np.exp(-src["opacity"][order]))) * 255, 0, 255).astype(np.uint8)
            s.mark("host_patch")
        if listed is not None:
            listed["exp_host"] = not exp_ok
        return out


@functools.cache
def cply_read_tables() -> np.ndarray:
    """The compressed-PLY reader's quotient tables (GSX_CPLY_TAB_*), each entry numpy's own result for the reference's statement
    on that input -- so the device divides only in the colour's `/ SH_C0` and takes no log.  -> uint8[GSX_CPLY_TAB_BYTES]"""
    with np.errstate(all="ignore"):
        q2047 = np.arange(2048, dtype=np.uint32) / 2047                                     # compressed_ply.py:346
        q1023 = np.arange(1024, dtype=np.uint32) / 1023
        q255 = np.arange(256, dtype=np.uint32) / 255.0                                      # :359
        dq = (np.arange(1024, dtype=np.uint32) / 1023.0 - 0.5) / 0.7071067811865476        # :370-371
        a = np.clip(np.arange(256, dtype=np.uint32) / 255.0, 1e-6, 1.0 - 1e-6)             # :361, :118-119
        opa = np.log(a / (1.0 - a)).astype(np.float32)
        sh = ((np.arange(256, dtype=np.uint8) / 256.0 - 0.5) * 8.0).astype(np.float32)     # :126
    tables = np.concatenate([np.concatenate([q2047, q1023, q255, dq]).view(np.uint8), opa.view(np.uint8), sh.view(np.uint8)])
    assert tables.nbytes == 8 * 4352 + 4 * 512
    return tables


def cply_unpack_table(path: str, segments: dict, layout: CplyReadLayout, n_chunks: int, n_vertices: int, dtype: np.dtype,
                      stage_ms: "dict | None" = None, device: int = 0, profile: "dict | None" = None, keep: "dict | None" = None) -> np.ndarray:
    """The compressed-PLY reader's rows (formats/compressed_ply.py:14-124) from a binary little-endian file: the elements' bodies
    are read from `path` (segments: "chunk", "vertex", "sh" -> (file offset, bytes) or None) straight into page-locked staging,
    uploaded once, decoded by gsx_cply_unpack_dev and downloaded into a prefaulted array of `dtype` (68 + 4 n_sh bytes of
    float32 per row; formats/compressed_ply_reader.py builds it).  Rows past 256 n_chunks stay zero, as in the reference.

    One ArenaSession of the "cplyread" lease group."""
    lib = require_hip()
    n = int(n_vertices)
    n_dec = min(n, 256 * int(n_chunks))
    out = np.empty(n, dtype)
    if n_dec == 0:
        out.view(np.uint8)[:] = 0
        return out
    place, total = {}, 0
    for k in ("chunk", "vertex", "sh"):      # each body at a 16-byte boundary of one staging buffer, 16 spare bytes after it
        if segments.get(k) is not None:
            place[k] = total
            total += (int(segments[k][1]) + 16 + 15) & ~15
    rb = dtype.itemsize

    def fill(host):
        with open(path, "rb") as f:
            for k, at in place.items():
                f.seek(int(segments[k][0]))
                read_exact(f, host[at:at + int(segments[k][1])], path, " in element %r" % k)
    with ArenaSession("cplyread", device, stage_ms) as s:
        host, join = stage_in(s, out, total, fill, "file_read")
        d_in, d_tab = s.upload_in(lib, host, total, cply_read_tables())
        s.mark("upload")
        d_out = session_out(s, keep, n_dec, n, dtype, profile)
        ptr = {k: d_in.ptr + place[k] for k in place}
        check(lib.gsx_cply_unpack_dev(s.ctx.handle, ptr["chunk"], int(n_chunks), ptr["vertex"], n, ptr.get("sh"), C.byref(layout), d_tab.ptr,
                                      d_out.ptr), "gsx_cply_unpack_dev")
        s.mark("kernel")
        session_profile(s, profile, d_out, n_dec, n, dtype)
        s.download_rows(lib, out, d_out, n_dec * rb, join)
        out.view(np.uint8)[n_dec * rb:] = 0        # rows past 256 n_chunks
        s.mark("download")
        session_keep(s, keep, out)
        return out


@functools.cache
def ksplat_read_tables() -> np.ndarray:
    """The .ksplat reader's colour tables, numpy's own results for the reference's statements on every byte: float32
    (b / 255.0 - 0.5) / SH_C0 [256] (formats/ksplat.py:230-233) | log(a / (1 - a)), a = clip(b / 255.0, 1e-7, 1 - 1e-7) [256]
    (:24-27) -- so the device takes no log.  -> float32[512]"""
    with np.errstate(all="ignore"):
        b = np.arange(256, dtype=np.uint8)
        rgba_f = b.astype(np.float32) / 255.0
        f_dc = (rgba_f - 0.5) / 0.28209479177387814
        alpha = np.clip(b.astype(np.float32) / 255.0, 1e-7, 1.0 - 1e-7)
        opa = np.log(alpha / (1.0 - alpha))
    assert f_dc.dtype == np.float32 and opa.dtype == np.float32
    return np.concatenate([f_dc, opa])


def ksplat_unpack_table(path: str, body_offset: int, body_bytes: int, level: int, sections, prefix: np.ndarray, n_coeffs: int,
                        n_rows: int, dtype: np.dtype, stage_ms: "dict | None" = None, device: int = 0,
                        profile: "dict | None" = None, keep: "dict | None" = None) -> np.ndarray:
    """The .ksplat reader's rows (formats/ksplat.py:104-317) from a file whose headers the caller has parsed and checked
    (formats/ksplat_reader.py): `body_bytes` bytes from file offset `body_offset` are read straight into page-locked staging,
    uploaded once, decoded by gsx_ksplat_unpack_dev (sections: KsplatReadSection records with offsets inside that body; prefix:
    uint32 prefix sums of the partially filled buckets' lengths) and downloaded into a prefaulted array of `dtype`
    (68 + 4 n_coeffs bytes of float32 per row).

    One ArenaSession of the "ksread" lease group."""
    lib = require_hip()
    n = int(n_rows)
    out = np.empty(n, dtype)
    rb = dtype.itemsize
    if rb != 68 + 4 * int(n_coeffs):
        raise ValueError("ksplat_unpack_table: rows of %d bytes for %d f_rest fields" % (rb, n_coeffs))
    if n == 0:
        return out
    total = int(body_bytes)
    secs = (KsplatReadSection * max(len(sections), 1))(*sections)
    prefix = np.ascontiguousarray(prefix, dtype=np.uint32)
    with ArenaSession("ksread", device, stage_ms) as s:
        host, join = stage_in(s, out, total, lambda view: read_file(path, body_offset, view, unit="payload bytes"), "file_read")
        d_in, d_tab = s.upload_in(lib, host, total + 32, ksplat_read_tables())   # 16-byte loads reach up to 15 bytes past the last row
        d_prefix = s.buf("prefix", max(prefix.nbytes, 16))
        if prefix.size:
            d_prefix.upload(prefix)
        s.mark("upload")
        d_out = session_out(s, keep, n, n, dtype, profile)
        check(lib.gsx_ksplat_unpack_dev(s.ctx.handle, d_in.ptr, total, int(level), secs, len(sections), d_prefix.ptr, int(prefix.size),
                                        d_tab.ptr, int(n_coeffs), d_out.ptr, n), "gsx_ksplat_unpack_dev")
        s.mark("kernel")
        session_profile(s, profile, d_out, n, n, dtype)
        s.download_rows(lib, out, d_out, n * rb, join)
        s.mark("download")
        session_keep(s, keep, out)
        return out


SPZ_READ_TABLES = ("opacity", "f_dc", "rgb", "scale", "sh", "rot_legacy", "rot_v3")   # GSX_SPZ_TAB_* order (include/gsx_hip.h)
SPZ_READ_POS_BYTES = {1: 6, 2: 9, 3: 9}   # spz.py:184, :190
SPZ_READ_ROT_BYTES = {1: 3, 2: 3, 3: 4}   # :232, :228


@functools.cache
def spz_read_tables() -> dict:
    """The SPZ reader's tables, numpy's own results for the reference's statements on every input (formats/spz.py), each with
    the reference's expression and operand dtypes -- so the device takes no log and divides only in the positions:
    "opacity" f4[256] :345-348 | "f_dc" f4[256] :207 | "rgb" u1[256] :214, the byte derived from that f_dc | "scale" f4[256]
    :222 (float64 there, rounded once on assignment) | "sh" f4[256] :243 | "rot_legacy" f4[256] :256 | "rot_v3" f4[1024]
    :274-277 (float64 there -- uint32 times a Python float -- holding a float32 value with its sign)"""
    with np.errstate(all="ignore"):
        b = np.arange(256, dtype=np.uint8)
        v = np.clip(b.astype(np.float32) / 255.0, 1e-7, 1.0 - 1e-7)
        opa = np.log(v / (1.0 - v))
        f_dc = (b.astype(np.float32) / 255.0 - 0.5) / 0.15
        rgb = np.clip((0.5 + 0.28209479177387814 * f_dc) * 255.0, 0, 255).astype(np.uint8)
        scale = (b / 16.0 - 10.0).astype(np.float32)
        sh = (b.astype(np.float32) - 128.0) / 128.0
        rot_legacy = b.astype(np.float32) / 127.5 - 1.0
        c = np.arange(1024, dtype=np.uint32)
        mag, neg = c & 0x1FF, (c >> 9) & 0x1
        rot_v3 = ((mag.astype(np.float32) / 511.0) * 0.707106781186547524401 * (1.0 - 2.0 * neg)).astype(np.float32)
    for t in (opa, f_dc, sh, rot_legacy):
        assert t.dtype == np.float32
    return dict(zip(SPZ_READ_TABLES, (opa, f_dc, rgb, scale, sh, rot_legacy, rot_v3)))


def spz_read_table_words() -> np.ndarray:
    """spz_read_tables() as the device takes them: uint32[GSX_SPZ_TAB_WORDS], the float32 bits, the colour bytes widened"""
    t = spz_read_tables()
    words = np.concatenate([t[k].astype(np.uint32) if t[k].dtype == np.uint8 else t[k].view(np.uint32) for k in SPZ_READ_TABLES])
    assert words.size == 2560
    return words


def spz_body_bytes(version: int, degree: int, n: int) -> int:
    """the six sections of n rows (spz.py:182-241)"""
    return n * (SPZ_READ_POS_BYTES[version] + 1 + 3 + 3 + SPZ_READ_ROT_BYTES[version] + 3 * SPZ_SH_DIM[degree])


def spz_unpack_table(fill, body_bytes: int, version: int, degree: int, fractional_bits: int, n_rows: int, dtype: np.dtype,
                     stage_ms: "dict | None" = None, device: int = 0, fill_stage: str = "file_read", profile: "dict | None" = None, keep: "dict | None" = None) -> np.ndarray:
    """The SPZ reader's rows (formats/spz.py:175-251) from a file whose header the caller has parsed and checked
    (formats/spz_reader.py): ``fill(view)`` puts the `body_bytes` bytes behind the header straight into page-locked staging
    (it raises what the reference raises on a damaged or short file: nothing has been uploaded then), one upload, decoded by
    gsx_spz_unpack_dev and downloaded into a prefaulted array of `dtype` (packed rows of 71 + 12 sh_dim bytes).

    One ArenaSession of the "spzread" lease group."""
    lib = require_hip()
    n, total = int(n_rows), int(body_bytes)
    rb = dtype.itemsize
    if rb != 71 + 12 * SPZ_SH_DIM[degree] or total != spz_body_bytes(version, degree, n):
        raise ValueError("spz_unpack_table: rows of %d bytes, a body of %d for version %d degree %d" % (rb, total, version, degree))
    out = np.empty(n, dtype)
    if n == 0:
        return out
    host_tab = spz_read_table_words()
    with ArenaSession("spzread", device, stage_ms) as s:
        host, join = stage_in(s, out, total, fill, fill_stage)
        d_in, d_tab = s.upload_in(lib, host, total + 32, host_tab)   # 16-byte loads reach up to 15 bytes past the last section
        s.mark("upload")
        d_out = session_out(s, keep, n, n, dtype, profile)
        check(lib.gsx_spz_unpack_dev(s.ctx.handle, d_in.ptr, total, int(version), int(degree), int(fractional_bits), d_tab.ptr, d_out.ptr, n),
              "gsx_spz_unpack_dev")
        s.mark("kernel")
        session_profile(s, profile, d_out, n, n, dtype)
        s.download_rows(lib, out, d_out, n * rb, join)
        s.mark("download")
        session_keep(s, keep, out)
        return out


SOG_READ_TABLES = ("scale_cb", "sh0_cb", "shn_cb", "opacity", "quat", "pos")       # GSX_SOG_TAB_* order (include/gsx_hip.h)
SOG_READ_TEXTURES = ("means_l", "means_u", "scales", "quats", "sh0", "shN_labels", "shN_centroids")   # gsx_sog_unpack_dev's order
SOG_COEFFS_PER_BAND = (0, 9, 24, 45)      # sog.py:170


@functools.cache
def sog_read_fixed_tables():
    """sog_read_tables' "opacity" and "quat": the two that depend on no file"""
    with np.errstate(all="ignore"):
        b = np.arange(256, dtype=np.uint8)
        alpha = np.clip(b.astype(np.float32) / 255.0, 1.0 / 255.0, 0.9999)
        opa = -np.log((1.0 / alpha) - 1.0)
        quat = (b.astype(np.float32) / 255.0 - 0.5) * 2.0
    assert opa.dtype == np.float32 and quat.dtype == np.float32
    return opa, quat


def sog_read_tables(mins, maxs, scale_codebook, sh0_codebook, shn_codebook=None) -> dict:
    """The SOG reader's tables, numpy's own results for the reference's statements on every input (formats/sog.py), each with
    the reference's expression and operand dtypes -- so the device takes no exp and no log:
    "scale_cb", "sh0_cb", "shn_cb" f4[len] :94, :149, :205, np.array(codebook, dtype=np.float32) as long as the file's (shn_cb
    empty without one) | "opacity" f4[256] :156-158 | "quat" f4[256] :108 | "pos" f4[3][65536] :78-86: the u16 code divided by
    65535.0 is float64 and so is all that follows, mins and maxs being the JSON's Python numbers; rounded once to float32, as
    the assignment into the float32 field does"""
    with np.errstate(all="ignore"):
        qv = np.arange(65536, dtype=np.uint32).astype(np.uint16)
        pos = np.empty((3, 65536), np.float32)
        for idx in range(3):
            norm = qv / 65535.0
            log_val = norm * (maxs[idx] - mins[idx]) + mins[idx]
            pos[idx] = np.sign(log_val) * (np.exp(np.abs(log_val)) - 1.0)
        assert norm.dtype == np.float64
    cbs = [np.array(cb if cb is not None else [], dtype=np.float32) for cb in (scale_codebook, sh0_codebook, shn_codebook)]
    return dict(zip(SOG_READ_TABLES, (*cbs, *sog_read_fixed_tables(), pos)))


def sog_read_table_words(tables: dict) -> np.ndarray:
    """sog_read_tables() as the device takes them: uint32[GSX_SOG_TAB_WORDS], the float32 bits; each codebook's first 256 entries
    (bytes index it), a shorter one padded with zeros (the caller has checked the indices against it)"""
    words = np.zeros(1280 + 3 * 65536, np.uint32)
    for k, name in enumerate(SOG_READ_TABLES[:5]):
        t = np.ascontiguousarray(tables[name], np.float32).reshape(-1)[:256]
        words[256 * k:256 * k + len(t)] = t.view(np.uint32)
    words[1280:] = np.ascontiguousarray(tables["pos"], np.float32).reshape(-1).view(np.uint32)
    return words


def sog_texel_layout(n: int, bands: int, palette: int):
    """-> ({texture: (byte offset, bytes)}, total): where each texture's texels lie in the staging buffer, SOG_READ_TEXTURES'
    order, each at a 16-byte boundary -- the first n RGBA texels of a per-row texture; of the centroid image the first 64 C
    pixels of each of its ceil(palette / 64) rows of 64 * 3 C (the only ones sog.py:190-202 reads), C coefficients per channel"""
    place, total = {}, 0
    for name in SOG_READ_TEXTURES[:6 if bands else 5]:
        place[name] = (total, 4 * n)
        total += (4 * n + 15) & ~15
    if bands:
        c = SOG_COEFFS_PER_BAND[bands] // 3
        nb = 4 * 64 * c * ((palette + 63) // 64)
        place["shN_centroids"] = (total, nb)
        total += (nb + 15) & ~15
    return place, total


def sog_unpack_table(fill, n_rows: int, bands: int, palette: int, tables: dict, dtype: np.dtype, on_flag=None,
                     stage_ms: "dict | None" = None, device: int = 0, profile: "dict | None" = None, keep: "dict | None" = None) -> np.ndarray:
    """The SOG reader's rows (formats/sog.py:60-247) from a bundle whose meta.json the caller has parsed and checked
    (formats/sog_reader.py): ``fill(view, place)`` decodes the textures' texels straight into page-locked staging
    (sog_texel_layout; it raises what the reference raises on a missing or short texture: nothing has been uploaded then), one
    upload of the staging and one of `tables` (sog_read_tables), decoded by gsx_sog_unpack_dev and downloaded into a prefaulted
    array of `dtype` (packed rows of 68 + 4 * 9 / 24 / 45 bytes).  A label at or above `palette` makes the kernel set a flag:
    ``on_flag(view, place)`` then raises numpy's own error from the host texels and no rows are returned.

    One ArenaSession of the "sogread" lease group."""
    lib = require_hip()
    n, bands, palette = int(n_rows), int(bands), int(palette)
    rb = dtype.itemsize
    if bands not in (0, 1, 2, 3) or rb != 68 + 4 * SOG_COEFFS_PER_BAND[bands] or n < 1 or (bands and not 1 <= palette <= 65536):
        raise ValueError("sog_unpack_table: %d rows of %d bytes, %d bands, a palette of %d" % (n, rb, bands, palette))
    place, total = sog_texel_layout(n, bands, palette)
    host_tab = sog_read_table_words(tables)
    out = np.empty(n, dtype)
    with ArenaSession("sogread", device, stage_ms) as s:
        host, join = stage_in(s, out, total, lambda view: fill(view, place), "decode")
        d_in, d_tab = s.upload_in(lib, host, total + 32, host_tab)   # spare bytes behind the last texel: no load reaches past the allocation
        d_flag = s.buf("flag", 16)
        check(lib.gsx_dev_memset(s.ctx.handle, d_flag.ptr, 0, 16), "gsx_dev_memset")
        s.mark("upload")
        d_out = session_out(s, keep, n, n, dtype, profile)
        offsets = (_I64 * 7)(*[place[t][0] if t in place else -1 for t in SOG_READ_TEXTURES])
        check(lib.gsx_sog_unpack_dev(s.ctx.handle, d_in.ptr, total, offsets, bands, palette, d_tab.ptr, d_out.ptr, n, d_flag.ptr),
              "gsx_sog_unpack_dev")
        s.mark("kernel")
        if bands and int(d_flag.download(np.uint32, 1)[0]):
            join()
            if on_flag is not None:
                on_flag(host, place)
            raise IndexError("sog_unpack_table: a label at or above the palette's %d entries" % palette)
        session_profile(s, profile, d_out, n, n, dtype)
        s.download_rows(lib, out, d_out, n * rb, join)
        s.mark("download")
        session_keep(s, keep, out)
        return out


def np_log_host(x: np.ndarray) -> np.ndarray:
    """csrc/np_log.h on the host (gsx_np_logf_host): the twin of the device's log"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(x)
    check(load().gsx_np_logf_host(x.ctypes.data, out.ctypes.data, x.size), "gsx_np_logf_host")
    return out


def np_log_probe_vector() -> np.ndarray:
    """~64K float32 inputs: the neighbours of 1e-6f (the reader's clamp) and of every power of two, the mantissas nearest
    sqrt(1/2) on both sides at every exponent (where the routine doubles m), denormals, +-0, +-inf, NaNs of both signs,
    exp(uniform(-14, 6)) (the scales of real scenes) and raw bit patterns"""
    rng = np.random.default_rng(0x6C6F67)
    u = np.uint32
    near = np.arange(-4, 5, dtype=np.int64)
    clamp = int(np.float32(1e-6).view(u)) + np.arange(-64, 65, dtype=np.int64)
    powers = ((np.arange(1, 255, dtype=np.int64) << 23)[:, None] + near).ravel()                   # 2^-126 ... 2^127
    denormal_powers = np.unique(np.clip((1 << np.arange(23, dtype=np.int64))[:, None] + near, 0, None).ravel())
    half_root = ((np.arange(0, 255, dtype=np.int64) << 23)[:, None] + 0x3504F3 + near).ravel()     # 0x3f3504f3 = float32(sqrt(1/2))
    special = np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF,
                        0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x80000001, 0xBF800000, 0x3F800000], np.int64)
    bits = np.concatenate([clamp, powers, denormal_powers, half_root, special]).astype(u).view(np.float32)
    parts = [bits,
             rng.integers(1, 1 << 23, 8192, dtype=np.uint64).astype(u).view(np.float32),          # denormals
             np.exp(rng.uniform(-14.0, 6.0, 28672)).astype(np.float32),
             rng.integers(0, 1 << 32, 20480, dtype=np.uint64).astype(u).view(np.float32)]
    return np.concatenate(parts)


_np_log_checked = None


def np_log_probe() -> bool:
    """The .splat reader stores np.log's float32 bits, so the device's log (csrc/np_log.h) must be THIS process's numpy's.  Probed
    once per process: the host twin against np.log on np_log_probe_vector().  On a mismatch: a RuntimeWarning and False (the
    reader then takes the three scale columns from numpy on the host, and stays exact), or under GSX_STRICT_NUMPY=1 a GsxError."""
    return np_probe("log")


SPLAT_READ_TABLES = ("f_dc", "opacity")   # GSX_SPLAT_TAB_* order (include/gsx_hip.h)
SPLAT_READ_RECORD = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("scale_0", "<f4"), ("scale_1", "<f4"), ("scale_2", "<f4"),
                              ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("opacity", "u1"),
                              ("rot_0", "u1"), ("rot_1", "u1"), ("rot_2", "u1"), ("rot_3", "u1")])   # splat.py:24-29


@functools.cache
def splat_read_tables() -> dict:
    """The .splat reader's tables, numpy's own results for the reference's statements on every byte, each with the reference's
    expression and operand dtypes -- so the device takes no log of them: "f_dc" f4[256] splat.py:75-77 | "opacity" f4[256]
    :67-69 (the clip's bounds are Python floats: the chain stays float32)"""
    with np.errstate(all="ignore"):
        b = np.arange(256, dtype=np.uint8)
        f_dc = (b.astype(np.float32) / 255.0 - 0.5) / 0.28209479177387814
        linear_alpha = b.astype(np.float32) / 255.0
        linear_alpha = np.clip(linear_alpha, 1.0 / 255.0, 0.9999)
        opa = -np.log((1.0 / linear_alpha) - 1.0)
    assert f_dc.dtype == np.float32 and opa.dtype == np.float32
    return dict(zip(SPLAT_READ_TABLES, (f_dc, opa)))


def splat_unpack_table(path: str, n_rows: int, dtype: np.dtype, stage_ms: "dict | None" = None, device: int = 0,
                       profile: "dict | None" = None, keep: "dict | None" = None) -> np.ndarray:
    """The .splat reader's rows (formats/splat.py:9-80): the first 32 `n_rows` bytes of `path` are read straight into page-locked
    staging, uploaded once, decoded by gsx_splat_unpack_dev and downloaded into a prefaulted array of `dtype` (packed rows of 71
    bytes; formats/splat_reader.py builds it).  When np_log_probe() fails, the three scale columns are numpy's, computed on the
    host from the staged records.

    One ArenaSession of the "splatread" lease group."""
    lib = require_hip()
    n = int(n_rows)
    rb = dtype.itemsize
    if rb != 71 or n < 1:
        raise ValueError("splat_unpack_table: %d rows of %d bytes" % (n, rb))
    log_ok = np_log_probe()
    if not log_ok:
        keep = None                      # (the scales are patched on the host below: the device rows are not the table's)
    total = n * SPLAT_READ_RECORD.itemsize
    tabs = splat_read_tables()
    host_tab = np.concatenate([tabs[k] for k in SPLAT_READ_TABLES])
    out = np.empty(n, dtype)
    with ArenaSession("splatread", device, stage_ms) as s:
        host, join = stage_in(s, out, total, lambda view: read_file(path, 0, view, unit="record bytes"), "file_read")
        d_in, d_tab = s.upload_in(lib, host, total, host_tab)
        s.mark("upload")
        d_out = session_out(s, keep, n, n, dtype, profile)
        check(lib.gsx_splat_unpack_dev(s.ctx.handle, d_in.ptr, n, d_tab.ptr, d_out.ptr), "gsx_splat_unpack_dev")
        s.mark("kernel")
        session_profile(s, profile, d_out, n, n, dtype)
        s.download_rows(lib, out, d_out, n * rb, join)
        if not log_ok:
            recs = host.view(SPLAT_READ_RECORD)
            with np.errstate(all="ignore"):
                for f in ("scale_0", "scale_1", "scale_2"):
                    out[f] = np.log(np.maximum(recs[f], 1e-6))                    # splat.py:43-48
        s.mark("download")
        session_keep(s, keep, out)
        return out


def ply_unpack_table(path: str, body_offset: int, n_rows: int, layout: PlyReadLayout, dtype: np.dtype, stage_ms: "dict | None" = None,
                     device: int = 0, profile: "dict | None" = None, keep: "dict | None" = None) -> np.ndarray:
    """The 3DGS / CloudCompare PLY readers' rows (formats/ply_3dgs.py:45-58, formats/ply_cc.py:45-60): the vertex element's body
    (`n_rows` rows of layout.in_stride bytes at byte `body_offset` of `path`) is read straight into page-locked staging, from
    the 16-byte boundary at or below it (so row 0 sits at byte 0 ... 15 of the buffer), uploaded once, transcoded by
    gsx_ply_unpack_dev and downloaded into a prefaulted array of `dtype` (layout.out_stride bytes per row;
    formats/ply_reader.py builds both).  A body that ends early raises read_exact's ValueError.

    One ArenaSession of the "plyread" lease group."""
    lib = require_hip()
    n, rb = int(n_rows), dtype.itemsize
    if n < 1 or rb != layout.out_stride:
        raise ValueError("ply_unpack_table: %d rows of %d bytes for a layout of %d" % (n, rb, layout.out_stride))
    start = int(body_offset) & ~15
    first = int(body_offset) - start
    used = first + n * layout.in_stride
    total = (used + 16 + 15) & ~15             # the kernel's 16-byte loads read up to 15 bytes past the last row
    out = np.empty(n, dtype)
    with ArenaSession("plyread", device, stage_ms) as s:
        host, join = stage_in(s, out, total, lambda view: read_file(path, start, view[:used], " in element 'vertex'"), "file_read")
        d_in, _ = s.upload_in(lib, host, total)
        s.mark("upload")
        d_out = session_out(s, keep, n, n, dtype, profile)
        check(lib.gsx_ply_unpack_dev(s.ctx.handle, d_in.ptr, first, n, C.byref(layout), d_out.ptr), "gsx_ply_unpack_dev")
        s.mark("kernel")
        session_profile(s, profile, d_out, n, n, dtype)
        s.download_rows(lib, out, d_out, n * rb, join)
        s.mark("download")
        session_keep(s, keep, out)
        return out


def ply_unpack_host(body: np.ndarray, n_rows: int, layout: PlyReadLayout, dtype: np.dtype) -> np.ndarray:
    """gsx_ply_unpack_host: the kernel's transcode on the host (`body`: uint8, the vertex rows from their first byte) -- the host
    tests' model of the device and the check of a descriptor table without one"""
    lib = load()
    n = int(n_rows)
    src = np.zeros(n * layout.in_stride + 4, np.uint8)
    src[:n * layout.in_stride] = body[:n * layout.in_stride]
    out = np.empty(n, dtype)
    check(lib.gsx_ply_unpack_host(src.ctypes.data, n, C.byref(layout), out.ctypes.data), "gsx_ply_unpack_host")
    return out


class PlyTextError(ValueError):
    """the body of an ASCII PLY element breaks the rules of DESIGN.md "ASCII PLY bodies"; str(): the reason, which names the
    element and the 1-based line"""


PLY_TEXT_BLANKS = b" \t\x0b\x0c\r"                 # what separates the tokens of a line (\n ends the line)
PLY_TEXT_CHUNK_BYTES = 64 << 20                    # text per upload: about 100 000 rows of a degree-3 scene
PLY_TEXT_MAX_CHUNK_BYTES = 1 << 29                 # (a chunk's rows are patched through 32-bit byte indices)
_PLY_TEXT_FLOAT = re.compile(rb"[+-]?(?:(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE][+-]?[0-9]+)?|[nN][aA][nN]|[iI][nN][fF](?:[iI][nN][iI][tT][yY])?)\Z")
_PLY_TEXT_INT = re.compile(rb"[+-]?[0-9]+\Z")


def ply_text_value(token: bytes, typ: str) -> bytes:
    """one token of an ASCII PLY body -> the little-endian bytes of its value as a property of numpy type `typ` ("f4", "u1" ...),
    the rule the device's number code is held against: a float token of the grammar is Python's float(token), and for "f4" that
    double cast to float32; an integer token is [+-]?D+ and must fit the type.  ValueError with the reason otherwise."""
    if typ in ("f4", "f8"):
        if not _PLY_TEXT_FLOAT.match(token):
            raise ValueError("%r is no decimal number" % token.decode("latin-1"))
        v = np.float64(float(token))
        with np.errstate(over="ignore", under="ignore"):
            return (v.astype("<f4") if typ == "f4" else v.astype("<f8")).tobytes()
    if not _PLY_TEXT_INT.match(token):
        raise ValueError("%r is no integer" % token.decode("latin-1"))
    v, info = int(token), np.iinfo(typ)
    if not info.min <= v <= info.max:
        raise ValueError("%d does not fit a property of type %s" % (v, np.dtype(typ).name))
    return np.array(v, "<" + typ).tobytes()


def ply_text_layout(props) -> PlyTextLayout:
    """[(name, numpy type str)] of an element -> gsx_ply_text_layout: the packed binary row of those properties"""
    if not 1 <= len(props) <= PLY_TEXT_MAX_PROPS:
        raise ValueError("ply_text_layout: %d properties (1 ... %d are supported)" % (len(props), PLY_TEXT_MAX_PROPS))
    tl, off = PlyTextLayout(), 0
    for i, (_, t) in enumerate(props):
        tl.offset[i], tl.type[i] = off, PLY_TYPE_CODES[t]
        off += np.dtype(t).itemsize
    tl.n_props, tl.in_stride = len(props), off
    return tl


def ply_text_chunk_host(text: np.ndarray, length: int, rows_left: int, tl: PlyTextLayout, rows: np.ndarray, list_cap: "int | None" = None):
    """gsx_ply_text_host on the first `length` bytes of `text` (uint8) into `rows` (uint8, rows_left rows of room)
    -> (result words, the (k, 4) uint32 entries of the listed tokens or None when more were listed than list_cap)"""
    lib = load()
    res = (C.c_int64 * PLY_TEXT_RESULT_WORDS)()
    cap = int(list_cap) if list_cap is not None else length // 2 + 1
    lst = np.zeros((max(cap, 1), 4), np.uint32)
    check(lib.gsx_ply_text_host(text.ctypes.data, int(length), int(rows_left), C.byref(tl), rows.ctypes.data, lst.ctypes.data, cap, res), "gsx_ply_text_host")
    return list(res), (lst[:res[4]] if res[4] <= cap else None)


def _ply_text_chunks(path: str, body_offset: int, n_rows: int, tl: PlyTextLayout, props, element: str, chunk_bytes: int, stats: "dict | None",
                     staging, run_chunk, patch, mark):
    """The ASCII reader's host loop, shared by the device path and its host model: windows of `chunk_bytes` of the file from
    `body_offset` on, each cut behind its last newline (the file's last line gets the newline it may lack), handed to
    ``run_chunk(host, length, rows_done, rows_left) -> (result words, listed tokens)``; the listed tokens are settled by
    ply_text_value and handed to ``patch(rows_done, byte indices, bytes)``.  Whatever breaks the rules raises PlyTextError.
    -> the byte offset of the file just past the element's last line"""
    lib = load()
    chunk_bytes = int(min(max(int(chunk_bytes), 1), PLY_TEXT_MAX_CHUNK_BYTES))
    host = staging(int(lib.gsx_ply_text_padded_bytes(chunk_bytes + 1)))
    P, stride = tl.n_props, tl.in_stride
    pos, done = int(body_offset), 0
    tokens = host_tokens = chunks = 0
    with open(path, "rb") as f:
        while done < n_rows:
            f.seek(pos)
            view, got = memoryview(host)[:chunk_bytes], 0
            while got < chunk_bytes:
                r = f.readinto(view[got:])
                if not r:
                    break
                got += r
            at_end = got < chunk_bytes
            window = host[:got]
            cut = _ply_text_last_newline(window) + 1
            if at_end and got > cut:                   # the file's last line has no newline of its own
                host[got] = 10
                cut = got + 1
            if cut == 0:
                if at_end:
                    raise PlyTextError("element %r ends after %d of %d lines (line %d is missing)" % (element, done, n_rows, done + 1))
                raise PlyTextError("element %r, line %d: longer than %d bytes" % (element, done + 1, chunk_bytes))
            host[cut:int(lib.gsx_ply_text_padded_bytes(cut))] = 10
            mark("file_read")
            res, listed = run_chunk(host, cut, done, n_rows - done)
            rows, bad = int(res[2]), int(res[3])
            listed = listed[np.argsort(listed[:, 0], kind="stable")]
            if bad >= 0:                               # (the lines before it are whole: their tokens' rows and columns hold)
                listed = listed[listed[:, 0] < bad * P]
            if len(listed):
                idx, val = [], []
                for t, off, _, _ in listed.tolist():
                    end = off
                    while host[end] != 10 and host[end] not in PLY_TEXT_BLANKS:
                        end += 1
                    row, col = divmod(t, P)
                    try:
                        b = ply_text_value(bytes(host[off:end]), props[col][1])
                    except ValueError as e:
                        raise PlyTextError("element %r, line %d, property %r: %s" % (element, done + row + 1, props[col][0], e)) from None
                    at = row * stride + tl.offset[col]
                    idx += range(at, at + len(b))
                    val += b
                if bad < 0:
                    patch(done, np.array(idx, np.uint32), np.array(val, np.uint8), rows * stride)
                    mark("patch")
            if bad >= 0:
                words = bytes(_ply_text_line(host, cut, bad)).split()
                why = ("is blank" if not words else "begins with '#'" if words[0].startswith(b"#") else
                       "holds %d values for %d properties" % (len(words), P))
                raise PlyTextError("element %r, line %d: %s" % (element, done + bad + 1, why))
            tokens, host_tokens, chunks = tokens + rows * P, host_tokens + len(listed), chunks + 1
            done += rows
            pos += int(res[5])
            if done < n_rows and at_end:
                raise PlyTextError("element %r ends after %d of %d lines (line %d is missing)" % (element, done, n_rows, done + 1))
    if stats is not None:
        stats.update(tokens=tokens, host_tokens=host_tokens, chunks=chunks, end_offset=pos)
    return pos


def _ply_text_last_newline(window: np.ndarray) -> int:
    """index of the last \\n of the uint8 array, or -1 (searched from the end in blocks: the whole window is not touched)"""
    hi = len(window)
    while hi > 0:
        lo = max(hi - 65536, 0)
        hit = np.flatnonzero(window[lo:hi] == 10)
        if len(hit):
            return lo + int(hit[-1])
        hi = lo
    return -1


def _ply_text_line(host: np.ndarray, length: int, k: int) -> np.ndarray:
    """line k (0-based, without its newline) of the chunk"""
    ends = np.flatnonzero(host[:length] == 10)
    return host[(ends[k - 1] + 1 if k else 0):ends[k]]


def ply_text_table(path: str, body_offset: int, n_rows: int, props, layout: PlyReadLayout, dtype: np.dtype, stage_ms: "dict | None" = None,
                   device: int = 0, profile: "dict | None" = None, keep: "dict | None" = None, stats: "dict | None" = None,
                   chunk_bytes: "int | None" = None, element: str = "vertex") -> np.ndarray:
    """The 3DGS / CloudCompare PLY readers' rows from an ASCII body (formats/ply_3dgs.py:10,45-58, formats/ply_cc.py:10,45-60): the
    text of the element's `n_rows` lines, from byte `body_offset` of `path`, is read into page-locked staging in chunks of
    `chunk_bytes` (default PLY_TEXT_CHUNK_BYTES; each cut behind its last newline), uploaded, scanned (gsx_ply_text_scan_dev) and
    parsed (gsx_ply_text_parse_dev) into ONE device buffer of n_rows x layout.in_stride bytes: the element as plyfile would hand
    it on, in the declared types `props` ([(name, numpy type str)]).  The tokens the device lists are settled on the host
    (ply_text_value) and patched into the rows (gsx_dev_patch_u8); a chunk that lists more than there is room for is converted
    by the host twin.  Then gsx_ply_unpack_dev, the profile pass, the download and `keep` as in ply_unpack_table.
    A body that breaks the rules raises PlyTextError.  stats receives tokens, host_tokens, chunks and end_offset (the byte just
    past the element's last line).  Stage clocks: file_read, upload, scan, kernel, patch, unpack, download.

    One ArenaSession of the "plytext" lease group."""
    lib = require_hip()
    n, rb = int(n_rows), dtype.itemsize
    tl = ply_text_layout(props)
    if n < 1 or rb != layout.out_stride or tl.in_stride != layout.in_stride:
        raise ValueError("ply_text_table: %d rows of %d bytes for a layout of %d, properties of %d for %d" % (n, rb, layout.out_stride, tl.in_stride, layout.in_stride))
    cb = int(chunk_bytes or PLY_TEXT_CHUNK_BYTES)
    cb = max(min(cb, os.path.getsize(path) - int(body_offset) + 1), 1)        # (no more staging than the file has text)
    out = np.empty(n, dtype)
    with ArenaSession("plytext", device, stage_ms) as s:
        join = prefault(out.nbytes >= (1 << 22), out)
        h = s.ctx.handle
        d_body = s.buf("body", n * tl.in_stride + 32)            # (the unpack kernel's 16-byte loads read past the last row)
        cap = int(min(max(cb, 1), PLY_TEXT_MAX_CHUNK_BYTES)) + 1
        d_text = s.buf("in", int(lib.gsx_ply_text_padded_bytes(cap)))
        work_bytes = int(lib.gsx_ply_text_work_bytes(cap))
        d_work = s.buf("work", work_bytes)
        list_cap = cap // 1024 + 4096
        d_list = s.buf("list", 16 * list_cap)
        res = (C.c_int64 * PLY_TEXT_RESULT_WORDS)()

        def run_chunk(host, length, done, left):
            s.upload_staging(lib, d_text.ptr, host[:int(lib.gsx_ply_text_padded_bytes(length))])
            s.mark("upload")
            check(lib.gsx_ply_text_scan_dev(h, d_text.ptr, length, d_work.ptr, work_bytes), "gsx_ply_text_scan_dev")
            s.mark("scan")
            rows_ptr = d_body.ptr + done * tl.in_stride
            check(lib.gsx_ply_text_parse_dev(h, d_text.ptr, length, left, C.byref(tl), rows_ptr, d_work.ptr, work_bytes, d_list.ptr, list_cap, res),
                  "gsx_ply_text_parse_dev")
            s.mark("kernel")
            r = list(res)
            if r[4] == 0:
                return r, np.zeros((0, 4), np.uint32)
            if r[4] <= list_cap:
                return r, d_list.download(np.uint32, 4 * r[4]).reshape(-1, 4)
            rows = np.zeros(r[2] * tl.in_stride, np.uint8)       # more listed tokens than room: the host twin takes the chunk
            r, listed = ply_text_chunk_host(host, length, left, tl, rows)
            check(lib.gsx_dev_upload(h, rows_ptr, rows.ctypes.data, rows.nbytes), "gsx_dev_upload")
            s.mark("patch")
            return r, listed

        def patch(done, idx, val, nbytes):
            dev_patch_u8(s.ctx, d_body.ptr + done * tl.in_stride, nbytes, idx, val)

        _ply_text_chunks(path, body_offset, n, tl, props, element, cb, stats, lambda nb: s.staging("in", nb), run_chunk, patch, s.mark)
        d_out = session_out(s, keep, n, n, dtype, profile)
        check(lib.gsx_ply_unpack_dev(h, d_body.ptr, 0, n, C.byref(layout), d_out.ptr), "gsx_ply_unpack_dev")
        s.mark("unpack")
        session_profile(s, profile, d_out, n, n, dtype)
        s.download_rows(lib, out, d_out, n * rb, join)
        s.mark("download")
        session_keep(s, keep, out)
        return out


def ply_text_host(path: str, body_offset: int, n_rows: int, props, layout: "PlyReadLayout | None" = None, dtype: "np.dtype | None" = None,
                  stats: "dict | None" = None, chunk_bytes: "int | None" = None, element: str = "vertex") -> np.ndarray:
    """ply_text_table without a device: the same chunk loop, gsx_ply_text_host for the kernels and gsx_ply_unpack_host for the
    transcode -- the host tests' model of the device, and the readers' parse of the non-vertex elements (layout None: the
    element's own rows, a structured array of `props`)"""
    n = int(n_rows)
    tl = ply_text_layout(props)
    own = np.dtype([(nm, "<" + t if np.dtype(t).itemsize > 1 else t) for nm, t in props])
    body = np.zeros(n * tl.in_stride + 4, np.uint8)

    def run_chunk(host, length, done, left):
        return ply_text_chunk_host(host, length, left, tl, body[done * tl.in_stride:])

    def patch(done, idx, val, nbytes):
        body[done * tl.in_stride + idx.astype(np.int64)] = val

    if n:
        _ply_text_chunks(path, body_offset, n, tl, props, element, int(chunk_bytes or PLY_TEXT_CHUNK_BYTES), stats,
                         lambda nb: np.empty(nb, np.uint8), run_chunk, patch, lambda name: None)
    elif stats is not None:
        stats.update(tokens=0, host_tokens=0, chunks=0, end_offset=int(body_offset))
    if layout is None:
        return body[:n * tl.in_stride].view(own).copy()
    return ply_unpack_host(body, n, layout, dtype)


def ply_pack_table(data: np.ndarray, plan_of, scan=None, stage_ms: "dict | None" = None, device: int = 0):
    """The 3DGS / CloudCompare PLY writers' vertex rows from a whole table (formats/ply_3dgs.py:70-109, formats/ply_cc.py:70-116):
    the raw rows are uploaded ONCE through the staging lanes, the crop scan reads its fields straight out of them, the plan is
    made from its answer, gsx_ply_pack_dev moves whole rows, and the file's rows come back through the staging lanes into the
    buffer the file is written from.

    data: 1-D C-contiguous structured table of n >= 1 rows of up to 512 bytes.  scan: None, or (offsets, present_mask) of the
    little-endian float32 f_rest_* fields for gsx_ply_rest_nonzero_dev; plan_of(last_idx) -- the highest scanned index holding a
    value != 0, -1 for none, None without a scan -- -> the plan (formats/ply_writer.py: WritePlan).
    -> (plan, rows): rows = uint8[n * plan.out_stride], or None when the plan is refused or its rows are the table's already
    (nothing is packed or downloaded then).

    One ArenaSession of the "plyw" lease group."""
    lib = require_hip()
    n = len(data)
    if n < 1 or not data.flags.c_contiguous or data.dtype.itemsize > PLY_WRITE_MAX_STRIDE:
        raise ValueError("ply_pack_table: %d rows of %d bytes (C-contiguous rows of up to %d)" % (n, data.dtype.itemsize, PLY_WRITE_MAX_STRIDE))
    with ArenaSession("plyw", device, stage_ms) as s:
        ctx = s.ctx
        d_rows = s.upload_rows(lib, data)
        last_idx = None
        if scan is not None:
            offsets, present = scan
            word = C.c_uint64(0)
            check(lib.gsx_ply_rest_nonzero_dev(ctx.handle, d_rows.ptr, data.dtype.itemsize, n, (C.c_int32 * 45)(*[int(o) for o in offsets]),
                                               int(present), C.byref(word)), "gsx_ply_rest_nonzero_dev")
            last_idx = word.value.bit_length() - 1
            s.mark("sh_detect")
        plan = plan_of(last_idx)
        s.mark("plan")
        if plan.refusal is not None or plan.identity:
            return plan, None
        lay = plan.layout()
        if lay.in_stride != data.dtype.itemsize:
            raise ValueError("ply_pack_table: a layout for rows of %d bytes, a table of %d" % (lay.in_stride, data.dtype.itemsize))
        nbytes = n * lay.out_stride
        out = np.empty(nbytes, np.uint8)
        join = prefault(nbytes >= (1 << 22), out)
        d_out = s.buf("out", nbytes)
        check(lib.gsx_ply_pack_dev(ctx.handle, d_rows.ptr, n, C.byref(lay), d_out.ptr), "gsx_ply_pack_dev")
        s.mark("pack")
        s.download_rows(lib, out, d_out, nbytes, join)
        s.mark("download")
        return plan, out


def ply_pack_host(data: np.ndarray, layout: PlyWriteLayout) -> np.ndarray:
    """gsx_ply_pack_host: the kernel's run code on the host (`data`: a 1-D C-contiguous table of layout.in_stride bytes a row) ->
    uint8[n * layout.out_stride] -- the host tests' model of the device and the check of a run table without one"""
    lib = load()
    n = len(data)
    if not data.flags.c_contiguous or data.dtype.itemsize != layout.in_stride:
        raise ValueError("ply_pack_host: C-contiguous rows of %d bytes" % layout.in_stride)
    out = np.empty(n * layout.out_stride, np.uint8)
    check(lib.gsx_ply_pack_host(data.ctypes.data, n, C.byref(layout), out.ctypes.data), "gsx_ply_pack_host")
    return out


def parquet_chunk_bits(validity, bit_offset: int, length: int) -> np.ndarray:
    """bits [bit_offset, bit_offset + length) of an Arrow validity bitmap (LSB first; None: every row is valid) -> bool[length]"""
    if validity is None:
        return np.ones(length, bool)
    v = np.frombuffer(validity, np.uint8)
    if (bit_offset + length + 7) >> 3 > len(v):
        raise ValueError("parquet: a validity bitmap of %d bytes for bits %d ... %d" % (len(v), bit_offset, bit_offset + length))
    bits = np.unpackbits(v[bit_offset >> 3:(bit_offset + length + 7) >> 3], bitorder="little")
    return bits[bit_offset & 7:(bit_offset & 7) + length].astype(bool)


def parquet_rows_plan(columns, n_rows: int, fields, out_stride: int):
    """Where the Parquet reader's columns lie in the one buffer its kernel reads.

    columns: per column a list of chunks (values, validity bytes or None, bit offset, length) -- `values` a 1-D array of the
    column's type whose first `length` elements are the chunk's (the caller has applied the chunk's offset to it), `validity`
    the chunk's Arrow bitmap as it lies in memory, its bit `bit offset` the chunk's first row; any bit offset, any length, the
    lengths of a column adding up to n_rows.  fields: per output field (column index or None, type code, destination offset,
    destination bytes).  A column's chunks are laid end to end from a 64-byte boundary; a column any of whose chunks has a
    bitmap gets ONE bitmap of (n + 63) / 64 * 8 bytes with bit r = row r, re-packed here.
    -> (ParquetRowsLayout, buffer bytes, [(byte offset, uint8 array)]: what to copy where)"""
    n = int(n_rows)
    if len(fields) < 1 or len(fields) > PARQUET_MAX_FIELDS:
        raise ValueError("parquet_rows_plan: %d fields (1 ... %d)" % (len(fields), PARQUET_MAX_FIELDS))
    lay = ParquetRowsLayout()
    lay.out_stride, lay.n_fields = int(out_stride), len(fields)
    placed, parts, total = {}, [], 0
    for k, (ci, code, dof, nb) in enumerate(fields):
        lay.src_type[k], lay.dst_offset[k], lay.dst_bytes[k] = int(code), int(dof), int(nb)
        lay.col_offset[k] = lay.valid_offset[k] = -1
        if ci is None:
            continue
        size = int(nb) if code == PLY_T_RAW else PARQUET_TYPE_BYTES[int(code)]
        if ci not in placed:
            chunks = columns[ci]
            if sum(int(c[3]) for c in chunks) != n:
                raise ValueError("parquet_rows_plan: column %d has %d rows in its chunks, the table %d" % (ci, sum(int(c[3]) for c in chunks), n))
            off, pos = total, 0
            total = (total + n * size + 63) & ~63
            for values, _, _, length in chunks:
                values = np.asarray(values)
                if values.dtype.itemsize != size or values.ndim != 1 or len(values) < length:
                    raise ValueError("parquet_rows_plan: column %d holds %s[%d], field %d reads %d values of %d bytes" % (ci, values.dtype, len(values), k, length, size))
                if length:
                    parts.append((off + pos * size, np.ascontiguousarray(values[:length]).view(np.uint8)))
                pos += int(length)
            voff = -1
            if n and any(c[1] is not None for c in chunks):
                bits = np.concatenate([parquet_chunk_bits(v, int(bo), int(ln)) for _, v, bo, ln in chunks])
                bitmap = np.zeros((n + 63) // 64 * 8, np.uint8)
                packed = np.packbits(bits, bitorder="little")
                bitmap[:len(packed)] = packed
                voff = total
                total = (total + len(bitmap) + 63) & ~63
                parts.append((voff, bitmap))
            placed[ci] = (off, voff, size)
        off, voff, have = placed[ci]
        if have != size:
            raise ValueError("parquet_rows_plan: column %d is read with %d and %d bytes a value" % (ci, have, size))
        lay.col_offset[k] = off
        lay.valid_offset[k] = -1 if code == PLY_T_RAW else voff
        if code == PLY_T_RAW and voff >= 0:
            raise ValueError("parquet_rows_plan: field %d is a byte copy of a column with a validity bitmap" % k)
    return lay, total + 64, parts


def _parquet_fill(parts):
    def fill(host):
        for off, a in parts:
            host[off:off + a.nbytes] = a
    return fill


def parquet_rows_table(columns, n_rows: int, fields, dtype: np.dtype, stage_ms: "dict | None" = None, device: int = 0,
                       profile: "dict | None" = None, keep: "dict | None" = None) -> np.ndarray:
    """The Parquet reader's rows (formats/parquet.py:51-55): Arrow's column chunks are laid end to end in page-locked staging
    (parquet_rows_plan: the one host copy a pageable upload makes anyway), uploaded once, transposed and cast by
    gsx_parquet_rows_dev and downloaded into a prefaulted array of `dtype`.  n_rows = 0 -> the empty array, no launch.

    One ArenaSession of the "pqread" lease group.  Stage clocks: gather, upload, kernel, download."""
    lib = require_hip()
    dtype = np.dtype(dtype)
    n, rb = int(n_rows), dtype.itemsize
    lay, total, parts = parquet_rows_plan(columns, n, fields, rb)
    if n == 0:
        return np.zeros(0, dtype)
    out = np.empty(n, dtype)
    with ArenaSession("pqread", device, stage_ms) as s:
        host, join = stage_in(s, out, total, _parquet_fill(parts), "gather")
        d_in, _ = s.upload_in(lib, host, total)
        s.mark("upload")
        d_out = session_out(s, keep, n, n, dtype, profile)
        check(lib.gsx_parquet_rows_dev(s.ctx.handle, d_in.ptr, total, n, C.byref(lay), d_out.ptr), "gsx_parquet_rows_dev")
        s.mark("kernel")
        session_profile(s, profile, d_out, n, n, dtype)
        s.download_rows(lib, out, d_out, n * rb, join)
        s.mark("download")
        session_keep(s, keep, out)
        return out


def parquet_rows_host(columns, n_rows: int, fields, dtype: np.dtype) -> np.ndarray:
    """gsx_parquet_rows_host: the kernel's casts on the host, from the same buffer -- the host tests' model of the device"""
    lib = load()
    dtype = np.dtype(dtype)
    n = int(n_rows)
    lay, total, parts = parquet_rows_plan(columns, n, fields, dtype.itemsize)
    buf = np.zeros(total, np.uint8)
    _parquet_fill(parts)(buf)
    out = np.zeros(n, dtype)
    check(lib.gsx_parquet_rows_host(buf.ctypes.data, total, n, C.byref(lay), out.ctypes.data), "gsx_parquet_rows_host")
    return out


def parquet_columns_plan(in_stride: int, n_rows: int, fields):
    """fields: per output column (source byte offset, bytes, kind) -- kind 0: a bit copy alone, 1: float32, 2: float64 (a validity
    bitmap and a null count with it).  -> (ParquetColumnsLayout, buffer bytes, [(column offset, bitmap offset or -1)])"""
    n = int(n_rows)
    if len(fields) < 1 or len(fields) > PARQUET_MAX_FIELDS:
        raise ValueError("parquet_columns_plan: %d fields (1 ... %d)" % (len(fields), PARQUET_MAX_FIELDS))
    lay = ParquetColumnsLayout()
    lay.in_stride, lay.n_fields = int(in_stride), len(fields)
    total, places = 0, []
    for k, (so, nb, kind) in enumerate(fields):
        lay.src_offset[k], lay.bytes[k], lay.kind[k] = int(so), int(nb), int(kind)
        lay.col_offset[k] = total
        total = (total + n * int(nb) + 63) & ~63
        lay.valid_offset[k] = -1
        if kind:
            lay.valid_offset[k] = total
            total = (total + (n + 63) // 64 * 8 + 63) & ~63
        places.append((lay.col_offset[k], lay.valid_offset[k]))
    return lay, total + 64, places


def _parquet_column_views(host, n, fields, places, counts):
    cols, bitmaps, nulls = [], [], []
    for (so, nb, kind), (co, vo) in zip(fields, places):
        cols.append(host[co:co + n * nb])
        bitmaps.append(host[vo:vo + (n + 7) // 8] if kind else None)
        nulls.append(int(counts[len(nulls)]) if kind else 0)
    return cols, bitmaps, nulls


def parquet_columns_table(data: np.ndarray, fields, stage_ms: "dict | None" = None, device: int = 0, consume=None):
    """The Parquet writer's columns from a whole table (formats/parquet.py:94-108 and pa.Table.from_pandas behind :111): the raw
    rows are uploaded ONCE, gsx_parquet_columns_dev writes every field as a contiguous column, with the Arrow validity bitmap
    and the null count of every float column, and all of it comes back into page-locked staging in one copy.

    data: 1-D C-contiguous structured table of n >= 1 rows of up to 512 bytes.  fields: parquet_columns_plan's.
    -> (columns, bitmaps, null counts): per field uint8[n * bytes], uint8[(n + 7) // 8] or None (kind 0), int.  They are views
    of the session's staging, good while the session lasts: `consume(columns, bitmaps, null_counts)` runs inside it and its
    result is returned; without one they are copied.

    One ArenaSession of the "pqw" lease group.  Stage clocks: upload, kernel, download (and what `consume` marks itself)."""
    lib = require_hip()
    n = len(data)
    if n < 1 or not data.flags.c_contiguous or data.dtype.itemsize > PARQUET_MAX_STRIDE:
        raise ValueError("parquet_columns_table: %d rows of %d bytes (C-contiguous rows of up to %d)" % (n, data.dtype.itemsize, PARQUET_MAX_STRIDE))
    fields = [(int(so), int(nb), int(kind)) for so, nb, kind in fields]
    lay, total, places = parquet_columns_plan(data.dtype.itemsize, n, fields)
    with ArenaSession("pqw", device, stage_ms) as s:
        ctx = s.ctx
        d_rows = s.upload_rows(lib, data)
        d_out, d_cnt = s.buf("out", total), s.buf("count", 8 * PARQUET_MAX_FIELDS)
        check(lib.gsx_parquet_columns_dev(ctx.handle, d_rows.ptr, n, C.byref(lay), d_out.ptr, total, d_cnt.ptr), "gsx_parquet_columns_dev")
        s.mark("kernel")
        host = s.staging("out", total)
        if s.leased:                                    # page-locked: the runtime's plain copy runs at link rate
            check(lib.gsx_dev_download(ctx.handle, host.ctypes.data, d_out.ptr, total), "gsx_dev_download")
        else:
            check(lib.gsx_dev_download_staged(ctx.handle, host.ctypes.data, d_out.ptr, total), "gsx_dev_download_staged")
        counts = d_cnt.download(np.uint64, PARQUET_MAX_FIELDS)
        s.mark("download")
        cols, bitmaps, nulls = _parquet_column_views(host, n, fields, places, counts)
        if consume is not None:
            return consume(cols, bitmaps, nulls)
        return [c.copy() for c in cols], [None if b is None else b.copy() for b in bitmaps], nulls


def parquet_columns_host(data: np.ndarray, fields):
    """gsx_parquet_columns_host: the kernel's split on the host -> (columns, bitmaps, null counts) as parquet_columns_table"""
    lib = load()
    n = len(data)
    data = np.ascontiguousarray(data)
    fields = [(int(so), int(nb), int(kind)) for so, nb, kind in fields]
    lay, total, places = parquet_columns_plan(data.dtype.itemsize, n, fields)
    host = np.zeros(total, np.uint8)
    counts = np.zeros(PARQUET_MAX_FIELDS, np.uint64)
    check(lib.gsx_parquet_columns_host(data.ctypes.data, n, C.byref(lay), host.ctypes.data, total, counts.ctypes.data), "gsx_parquet_columns_host")
    return _parquet_column_views(host, n, fields, places, counts)


class DeviceArray:
    """A raw HBM allocation owned by a Context (only used where no other allocator is around)."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(ctx.lib.gsx_dev_malloc(ctx.handle, self.nbytes, C.byref(p)), "gsx_dev_malloc")
        self.ptr = p.value

    def upload(self, arr: np.ndarray):
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes
        check(self.ctx.lib.gsx_dev_upload(self.ctx.handle, self.ptr, a.ctypes.data, a.nbytes), "gsx_dev_upload")
        return self

    def download(self, dtype, count: int) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        assert out.nbytes <= self.nbytes
        check(self.ctx.lib.gsx_dev_download(self.ctx.handle, out.ctypes.data, self.ptr, out.nbytes), "gsx_dev_download")
        return out

    def download_at(self, byte_offset: int, dtype, count: int) -> np.ndarray:
        """`count` elements starting `byte_offset` bytes into the buffer"""
        out = np.empty(count, dtype=dtype)
        assert 0 <= byte_offset and byte_offset + out.nbytes <= self.nbytes
        check(self.ctx.lib.gsx_dev_download(self.ctx.handle, out.ctypes.data, self.ptr + byte_offset, out.nbytes), "gsx_dev_download")
        return out

    def free(self):
        if self.ptr:
            self.ctx.lib.gsx_dev_free(self.ctx.handle, self.ptr)
            self.ptr = None


class Context:
    """gsx_ctx wrapper: device-resident entry points (pointers are plain ints)."""

    def __init__(self, device: int = 0, stream: int | None = None, own_stream: bool = False):
        self.lib = require_hip()
        h = C.c_void_p()
        check(self.lib.gsx_ctx_create(int(device), C.byref(h)), "gsx_ctx_create")
        self.handle = h
        if stream is not None:
            self.set_stream(stream)
        elif own_stream:   # a non-blocking stream of its own: contexts created like this run concurrently on one GPU
            check(self.lib.gsx_ctx_own_stream(self.handle), "gsx_ctx_own_stream")

    def close(self):
        if self.handle:
            self.lib.gsx_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream: int):
        check(self.lib.gsx_ctx_set_stream(self.handle, C.c_void_p(int(stream))), "gsx_ctx_set_stream")

    def synchronize(self):
        check(self.lib.gsx_ctx_synchronize(self.handle), "gsx_ctx_synchronize")

    def check(self):
        """synchronise + raise GsxError if a _dev call met non-finite coordinates since the last check"""
        check(self.lib.gsx_ctx_check(self.handle), "gsx_ctx_check")

    def last_knn_algo(self) -> int:
        """KNN_* of the path this context's last KNN call took (adaptive mode picks GRID or TREE)"""
        return int(self.lib.gsx_ctx_last_knn_algo(self.handle))

    def set_param(self, name: str, value: float):
        check(self.lib.gsx_ctx_set_param(self.handle, name.encode(), float(value)), "gsx_ctx_set_param")

    def set_timing(self, on: bool):
        check(self.lib.gsx_ctx_set_timing(self.handle, 1 if on else 0), "gsx_ctx_set_timing")

    def reset_timing(self):
        check(self.lib.gsx_ctx_reset_timing(self.handle), "gsx_ctx_reset_timing")

    def timing(self, slot: int):
        n = C.c_uint64()
        ms = C.c_double()
        check(self.lib.gsx_ctx_get_timing(self.handle, int(slot), C.byref(n), C.byref(ms)), "gsx_ctx_get_timing")
        return int(n.value), float(ms.value)

    def density_stage_clocks(self):
        """stage clocks (ms) of this context's last density_filter_large / voxel_clusters call while timing was on"""
        ms = (C.c_double * len(DENSITY_STAGES))()
        check(self.lib.gsx_density_stage_clocks(self.handle, ms), "gsx_density_stage_clocks")
        return dict(zip(DENSITY_STAGES, (float(v) for v in ms)))

    def alloc(self, nbytes: int) -> DeviceArray:
        return DeviceArray(self, nbytes)

    def sor_knn(self, x: int, y: int, z: int, stride: int, n_ref: int, q_begin: int, q_count: int, k: int,
                mean_out: int, algo: int = KNN_AUTO, want_info: bool = False):
        info = SorInfo() if want_info else None
        check(self.lib.gsx_sor_knn_dev(self.handle, x, y, z, stride, n_ref, q_begin, q_count, int(k), int(algo),
                                       mean_out, C.byref(info) if want_info else None), "gsx_sor_knn_dev")
        return info.as_dict() if want_info else None

    def sor_knn_share(self, x: int, y: int, z: int, stride: int, n: int, k: int, share: int, nshares: int,
                      mean_out: int, algo: int = KNN_AUTO, want_info: bool = False):
        info = SorInfo() if want_info else None
        check(self.lib.gsx_sor_knn_share_dev(self.handle, x, y, z, stride, n, int(k), int(algo), int(share),
                                             int(nshares), mean_out, C.byref(info) if want_info else None),
              "gsx_sor_knn_share_dev")
        return info.as_dict() if want_info else None

    def debug_brick_plan(self, cap: int = 1 << 22):
        """brick plan of this context's last grid KNN call: dict(nx, ny, nz, plan, bricks, origin (ox, oy, oz, inv_h) as
        float32, runs = (bricks, 3) int array of (bundle, first quarter, last quarter) when the planned bricks ran)"""
        import numpy as np
        grid = (C.c_int32 * 8)()
        origin = (C.c_float * 4)()
        buf = np.zeros((cap, 2), np.uint32)
        check(self.lib.gsx_sor_debug_brick_plan(self.handle, grid, origin, buf.ctypes.data_as(C.c_void_p), cap),
              "gsx_sor_debug_brick_plan")
        m = min(int(grid[4]), cap) if grid[3] else 0
        runs = np.stack([buf[:m, 0], buf[:m, 1] & 0xffff, buf[:m, 1] >> 16], axis=1).astype(np.int64)
        return {"nx": int(grid[0]), "ny": int(grid[1]), "nz": int(grid[2]), "plan": int(grid[3]), "bricks": int(grid[4]),
                "origin": np.array(list(origin), np.float32), "runs": runs}

    def debug_work_queue(self):
        """work queues of this context's last grid KNN call: dict(name -> dict(ctr = final tail counters of the eight groups,
        items, blocks = workgroups of the launch, four waves each)) for knn_brick, knn_brick_extra, knn_ring, knn_ring_fast"""
        import numpy as np
        ctr = np.zeros((4, 8), np.uint32)
        items = np.zeros(4, np.int64)
        blocks = np.zeros(4, np.int32)
        check(self.lib.gsx_sor_debug_work_queue(self.handle, ctr.ctypes.data_as(C.c_void_p), items.ctypes.data_as(C.c_void_p),
                                                blocks.ctypes.data_as(C.c_void_p)), "gsx_sor_debug_work_queue")
        names = ("knn_brick", "knn_brick_extra", "knn_ring", "knn_ring_fast")
        return {nm: {"ctr": ctr[i].astype(np.int64), "items": int(items[i]), "blocks": int(blocks[i])} for i, nm in enumerate(names)}

    def debug_tree(self, want_leaves: bool = False, cap: int | None = None):
        """which stage of the Morton-tree path answered in this context's last tree run: dict(n, nleaves, fail_count = queries
        knn_leaf handed to knn_tree_near, fail2_count = queries knn_tree_near handed to knn_tree_query, max_leaf (adaptive
        mode's guard sets it), leaf_cap, defer_why = int array of 8: knn_tree_near's reasons); want_leaves: also keys = the n
        sorted Morton keys (uint64) and leafstart = the nleaves + 1 leaf starts, through buffers of `cap` entries (None: as
        many as the run needs)"""
        import numpy as np
        ctr = np.zeros(16, np.uint32)
        n, nl = _I64(), _I64()
        check(self.lib.gsx_sor_debug_tree(self.handle, ctr.ctypes.data_as(C.c_void_p), None, None, 0, C.byref(n), C.byref(nl)),
              "gsx_sor_debug_tree")
        res = {"n": int(ctr[0]), "nleaves": int(ctr[1]), "fail_count": int(ctr[2]), "fail2_count": int(ctr[3]), "max_leaf": int(ctr[4]),
               "leaf_cap": int(ctr[5]), "defer_why": ctr[8:16].astype(np.int64)}
        if want_leaves:
            cap = max(int(n.value), int(nl.value) + 1) if cap is None else int(cap)
            keys = np.zeros(max(cap, 1), np.uint64)
            starts = np.zeros(max(cap, 1), np.uint32)
            check(self.lib.gsx_sor_debug_tree(self.handle, ctr.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p),
                                              starts.ctypes.data_as(C.c_void_p), cap, C.byref(n), C.byref(nl)), "gsx_sor_debug_tree")
            res["keys"] = keys[:int(n.value)]
            res["leafstart"] = starts[:int(nl.value) + 1].astype(np.int64)
        return res

    def debug_wave_stamps(self, kernel: int):
        """diagnostic builds (-DGSX_WAVE_STAMPS) only: (waves, 16) uint64 records of knn_brick (kernel 0) or knn_ring_fast
        (kernel 1) of this context's last grid KNN call, the waves that wrote none left out (tools/wave_stamps.py)"""
        import numpy as np
        cap = 1 << 14
        buf = np.zeros((cap, 16), np.uint64)
        count = C.c_int64()
        check(self.lib.gsx_sor_debug_wave_stamps(self.handle, int(kernel), buf.ctypes.data_as(C.c_void_p), cap, C.byref(count)),
              "gsx_sor_debug_wave_stamps")
        rec = buf[:min(cap, int(count.value))]
        return rec[rec[:, 14] == 1]

    def knn_probe_root(self, values: int, n: int, mode: int, out: int):
        """debug / tests: out[i] = float64 root of values[i] (device pointers); mode 0 sqrt_rn_dist2, 1 __dsqrt_rn"""
        check(self.lib.gsx_knn_probe_root_dev(self.handle, values, int(n), int(mode), out), "gsx_knn_probe_root_dev")

    def knn_probe_root_short(self, values: int, n: int, mode: int, out: int):
        """debug / tests: out[i] = sqrt_short_dist2(values[i]) (PROBE_SHORT_ROOT, the certified epilogue's root) or the
        v_rsq_f64 seed it starts from (PROBE_SHORT_SEED); device pointers"""
        check(self.lib.gsx_knn_probe_root_short_dev(self.handle, values, int(n), int(mode), out), "gsx_knn_probe_root_short_dev")

    def knn_probe_mean(self, d2: int, m: int, stride: int, k: int, form: int, cap: int, out: int):
        """debug / tests: float32 row means of m rows of ascending float64 squared distances (device pointers) through one
        form of the KNN epilogue: PROBE_MEAN_NET / LIST (cap = list length / capacity), LE128, NP (include/gsx_hip.h)"""
        check(self.lib.gsx_knn_probe_mean_dev(self.handle, d2, int(m), int(stride), int(k), int(form), int(cap), out),
              "gsx_knn_probe_mean_dev")

    def sor_stats(self, mean_dists: int, n: int, threshold_factor: float, stats_out: int):
        check(self.lib.gsx_sor_stats_dev(self.handle, mean_dists, n, float(threshold_factor), stats_out),
              "gsx_sor_stats_dev")

    def sor_mask(self, mean_dists: int, n: int, threshold_ptr: int, mask_out: int):
        check(self.lib.gsx_sor_mask_dev(self.handle, mean_dists, n, threshold_ptr, mask_out), "gsx_sor_mask_dev")


class DeviceArena:
    """A long-lived context + named GROW-ONLY device buffers, one per device and process (``arena(device)``).

    hipMalloc / hipFree are not cheap at the writers' sizes: a call that allocates its ~6 GB of work buffers afresh spends
    anything from 3 to 300 ms in the allocator (measured on MI355X, 20 allocations of a 10M-splat SOG encode: 3 ms when the
    runtime still holds the address ranges of the previous call's frees, 308 ms when it does not), and the first DMA into a
    freshly mapped range runs at half the link rate.  A writer that is called again (a converter working through a directory
    of scenes, bench.py's repetitions) finds its buffers here; ``release_arenas()`` gives the memory back.

    Every named buffer belongs to a LEASE GROUP, the part of its name before the first "_" ("sog_rows" -> "sog", "rgb_in" ->
    "rgb"), and every group runs on a context of its own (``context(group)``: its stream and the library's per-context work
    buffers).  ``buf()``, ``pinned()`` and ``context()`` serve a group only while it is leased (``lease`` / ``leased``): one user
    of a group at a time, so a buffer never grows -- and frees its old allocation -- under another thread that still reads it.
    A caller that does not win its lease (another thread holds it) takes private allocations instead.
    A user whose lease lasts one call takes it through ``ArenaSession``, which does all of this for it."""

    def __init__(self, device: int = 0):
        self.device = int(device)
        self.closed = False
        self._ctxs = {}                 # lease group -> Context
        self._sides = {}                # lease group -> second Context with a stream of its own
        self._bufs = {}
        self._pinned = {}
        self._leases = set()

    @staticmethod
    def group(name: str) -> str:
        return name.split("_", 1)[0]

    def _require(self, group: str, what: str):
        if group not in self._leases:   # (one set lookup: a user that skips the lease fails at once instead of racing)
            raise RuntimeError("DeviceArena: %s used without holding the %r lease" % (what, group))

    def context(self, group: str) -> "Context":
        """the context of lease group `group` (created on first use, kept until release())"""
        self._require(group, "context(%r)" % group)
        c = self._ctxs.get(group)
        if c is None:
            c = self._ctxs[group] = Context(self.device)
        return c

    def side(self, group: str) -> "Context":
        """a second context of lease group `group` with a stream of its own (copies that overlap the first one's kernels)"""
        self._require(group, "side(%r)" % group)
        c = self._sides.get(group)
        if c is None:
            c = self._sides[group] = Context(self.device, own_stream=True)
        return c

    def buf(self, name: str, nbytes: int) -> DeviceArray:
        group = self.group(name)
        self._require(group, "buf(%r)" % name)
        nbytes = max(int(nbytes), 16)
        cur = self._bufs.get(name)
        if cur is None or cur.nbytes < nbytes:
            if cur is not None:
                cur.free()
            cur = self.context(group).alloc(nbytes + 256)
            self._bufs[name] = cur
        return cur

    def pinned(self, name: str, nbytes: int) -> np.ndarray:
        """a named grow-only PAGE-LOCKED host buffer as a uint8 array (hipHostMalloc: the DMA engines read it at link rate)"""
        group = self.group(name)
        self._require(group, "pinned(%r)" % name)
        nbytes = max(int(nbytes), 16)
        ctx = self.context(group)
        cur = self._pinned.get(name)
        if cur is None or cur[1] < nbytes:
            if cur is not None:
                ctx.lib.gsx_host_pinned_free(ctx.handle, C.c_void_p(cur[0]))
                del self._pinned[name]
            p = C.c_void_p()
            check(ctx.lib.gsx_host_pinned_alloc(ctx.handle, nbytes, C.byref(p)), "gsx_host_pinned_alloc")
            cur = self._pinned[name] = (p.value, nbytes)
        return np.ctypeslib.as_array((C.c_uint8 * cur[1]).from_address(cur[0]))

    def lease(self, who: str) -> bool:
        """one user of lease group `who` at a time -> True when this caller got it (False: another user holds it, or the arena
        has been released; the caller then takes allocations of its own)"""
        with _arena_lock:               # (two threads asking at once: exactly one of them gets it; release_arenas() takes it too)
            if self.closed or who in self._leases:
                return False
            self._leases.add(who)
            return True

    def unlease(self, who: str):
        with _arena_lock:
            self._leases.discard(who)

    @contextlib.contextmanager
    def leased(self, who: str):
        """``with ar.leased("sog") as won:`` -- the lease of `who` for the block when `won`, given back on every exit path"""
        won = self.lease(who)
        try:
            yield won
        finally:
            if won:
                self.unlease(who)

    def held_bytes(self) -> int:
        return sum(b.nbytes for b in self._bufs.values())

    def held_pinned_bytes(self) -> int:
        return sum(nb for _, nb in self._pinned.values())

    def release(self):
        self.closed = True
        for b in self._bufs.values():
            b.free()
        self._bufs.clear()
        for name, (ptr, _) in self._pinned.items():
            c = self._ctxs.get(self.group(name))
            if c is not None and c.handle:
                c.lib.gsx_host_pinned_free(c.handle, C.c_void_p(ptr))
        self._pinned.clear()
        for c in (*self._sides.values(), *self._ctxs.values()):
            c.close()
        self._sides.clear()
        self._ctxs.clear()


_arenas = {}
_arena_lock = threading.RLock()


def arena(device: int = 0) -> DeviceArena:
    with _arena_lock:
        a = _arenas.get(int(device))
        if a is None or a.closed:
            a = _arenas[int(device)] = DeviceArena(device)
        return a


def release_arenas():
    """free every cached work buffer and context of the writers' arenas (they are re-created on the next call)"""
    with _arena_lock:
        for dev, a in list(_arenas.items()):
            if a._leases:            # some user holds a lease (a writer mid-call, a lazy DataProcessor with pending filters): it keeps it
                continue
            if not a.closed:
                a.release()
            del _arenas[dev]


class ArenaSession:
    """One call's use of a lease group: ``with ArenaSession("spz", device, stage_ms) as s:`` around the whole device part.

    The call runs on the process's arena -- ``s.ctx`` is the group's context, ``s.buf("rows", n)`` the grow-only buffer
    "spz_rows", no allocation on a repeated call -- while it holds the group's lease; a second call at the same moment (another
    thread) takes a context and buffers of its own, freed and closed when the block ends.  ``shared=False`` never asks the arena,
    and a caller's `ctx` is used as it is: no lease, and not closed here.

    A GsxError in the block gives the lease back and THEN releases the arenas (a failed HIP call: no context in an unknown state
    is handed on; with the lease still held release_arenas() would spare this arena); every other exit keeps the arena's
    buffers.  Private buffers are freed before their context closes.  ``s.mark(name)`` is the stage clock (a synchronisation per
    stage) when the caller asks for one with a `stage_ms` dict; it starts when the session is made.

    The six table readers share one sequence: stage_in() -- staging, the caller's fill, the fill stage's mark, all on the host --
    then ``s.upload_in``, the caller's own uploads and mark("upload"), its launch and mark("kernel"), ``s.download_rows`` and
    mark("download").  A reader that is handed a ``profile`` dict runs session_profile() between the launch and the download:
    one more pass over the decoded rows (gsx_table_profile_dev) and a mark("profile").  The six table writers open with
    ``s.upload_rows``: the table into the buffer "rows" and mark("upload"), or a caller's resident rows where they are."""

    def __init__(self, group: str, device: int = 0, stage_ms: "dict | None" = None, ctx: "Context | None" = None, shared: bool = True):
        self.group, self.device, self.stage_ms, self.ctx = group, device, stage_ms, ctx
        self._ar = arena(device) if shared and ctx is None else None
        self.leased = self._ar is not None and self._ar.lease(group)
        self._own = ctx is None and not self.leased
        self._bufs = []
        self.kept = None                # session_out's ResidentRows until session_keep hands it to the caller's dict
        self._t = time.perf_counter()

    def __enter__(self):
        try:
            if self.ctx is None:
                self.ctx = self._ar.context(self.group) if self.leased else Context(self.device)
        except BaseException as e:      # (the lease is held already: the block's own exit paths)
            self.__exit__(type(e), e, None)
            raise
        return self

    def __exit__(self, etype, exc, tb):
        if self.kept is not None:       # (the block ended before session_keep: nobody else knows these rows)
            kept, self.kept = self.kept, None
            kept.close()
        if self.leased and etype is not None and issubclass(etype, GsxError):
            self._ar.unlease(self.group)
            self.leased = False
            release_arenas()
        for b in self._bufs:
            b.free()
        if self.leased:
            self._ar.unlease(self.group)
        if self._own and self.ctx is not None:
            self.ctx.close()

    def mark(self, name: str):
        if self.stage_ms is not None:
            self.ctx.synchronize()
            now = time.perf_counter()
            self.stage_ms[name] = round(self.stage_ms.get(name, 0.0) + (now - self._t) * 1e3, 3)
            self._t = now

    def buf(self, name: str, nbytes: int) -> DeviceArray:
        if self.leased:
            return self._ar.buf(self.group + "_" + name, nbytes)
        b = self.ctx.alloc(max(int(nbytes), 16))
        self._bufs.append(b)
        return b

    def staging(self, name: str, nbytes: int) -> np.ndarray:
        """`nbytes` of host memory to read a file into: the arena's page-locked buffer under the lease, a pageable array without"""
        return self._ar.pinned(self.group + "_" + name, nbytes)[:nbytes] if self.leased else np.empty(nbytes, np.uint8)

    def upload_staging(self, lib, dev_ptr: int, host: np.ndarray):
        """staging() memory to the device: page-locked, the runtime's plain copy runs at link rate; pageable goes through the lanes"""
        if self.leased:
            check(lib.gsx_dev_upload(self.ctx.handle, dev_ptr, host.ctypes.data, host.nbytes), "gsx_dev_upload")
        else:
            check(lib.gsx_dev_upload_staged(self.ctx.handle, dev_ptr, host.ctypes.data, host.nbytes), "gsx_dev_upload_staged")

    def upload_in(self, lib, host: np.ndarray, dev_bytes: int, tables: "np.ndarray | None" = None):
        """a reader's uploads after stage_in(): the staging `host` into the buffer "in" of `dev_bytes` (the caller's size: what its
        kernel's 16-byte loads may reach behind the last row), `tables` into the buffer "tables".  No mark: the caller adds its
        own uploads and marks "upload".  -> (d_in, d_tables or None)"""
        d_in = self.buf("in", dev_bytes)
        d_tab = self.buf("tables", tables.nbytes) if tables is not None else None
        self.upload_staging(lib, d_in.ptr, host)
        if d_tab is not None:
            d_tab.upload(tables)
        return d_in, d_tab

    def upload_rows(self, lib, data: np.ndarray, slack: int = 64, resident: "ResidentRows | None" = None):
        """a table writer's first step, upload_in's mirror: the table `data` into the buffer "rows" of data.nbytes + `slack` (the
        kernels' 16-byte loads read up to 15 bytes past the last row), one upload_table when the table has bytes, and
        mark("upload") either way.  With the caller's `resident` rows of the table: those, where they are -- no buffer, no upload
        and no "upload" mark.  -> an object with .ptr"""
        if resident is not None:
            return resident
        d_rows = self.buf("rows", data.nbytes + slack)
        if data.nbytes:
            upload_table(lib, self.ctx, d_rows.ptr, data)
        self.mark("upload")
        return d_rows

    def download_rows(self, lib, out: np.ndarray, d_out: DeviceArray, nbytes: int, join):
        """the last step of a reader and of the PLY writer: the prefault joined, then the first `nbytes` of `d_out` through the
        staging lanes into the first `nbytes` of `out`"""
        join()
        check(lib.gsx_dev_download_staged(self.ctx.handle, out.view(np.uint8).ctypes.data, d_out.ptr, nbytes), "gsx_dev_download_staged")


class DeviceChain:
    """Coordinates resident in HBM across consecutive filters (device half).

    The reference ends every filter with ``self.data = vertices[mask]`` on the host table (data_processor.py:114,149)
    and re-gathers ``coords`` at the start of the next one (:38,139).  Here the (n,3) rows are uploaded once, every
    filter leaves its mask in HBM, ``gsx_compact_rows_dev`` compacts the rows there, and the composed survivor list comes
    back once -- the 248-byte host rows are compacted once, after the last filter.

    Over resident rows (``resident=``) the chain also owns every buffer that work on them needs, by name and size, and gives
    each back: ``resident_column`` for ge_keep, ``resident_rgb`` / ``rgb_to_host`` for add_rgb_from_sh's colours, and ``take``,
    which picks the survivor list and has the rows write the survivors into new resident rows.  DataProcessor calls these and
    holds no device buffer itself."""

    def __init__(self, xyz_rows: "np.ndarray | None" = None, device: int = 0, keep_pristine: bool = False, table: "np.ndarray | None" = None,
                 resident: "ResidentRows | None" = None):
        """xyz_rows: (n, 3) coordinates, or table: the structured splat table itself -- its x, y, z are then gathered (threaded, C ABI
        gsx_host_gather_f32) straight into a page-locked staging buffer of the arena: no 12n-byte temporary whose pages are faulted
        in, copied from at pageable rate and unmapped again (9 + 5 + 9 ms of configs.dropin_e2e_10m's 37) --, or resident: the
        table's rows in HBM (ResidentRows, the caller's: not closed here) -- its '<f4' x, y, z are then gathered device to device
        (gsx_rows_columns_f32_dev): no host gather, no pinned staging, no upload"""
        self.resident = resident
        a = None
        if resident is not None:
            device = resident.device
        elif table is None:
            a = np.ascontiguousarray(xyz_rows, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != 3:
                raise ValueError("Requires 3D data")
        # round 6: the process-wide arena's context and named buffers when no other chain holds them -- a chain per filter run used
        # to create a context, hipMalloc its ~37 bytes per row and, inside the context, the whole KNN workspace, and free it all
        # again at close(): 10-12 of the 37 ms of configs.dropin_e2e_10m.  release_arenas() gives the memory back.
        require_hip()
        ar = arena(device)
        # the lease is taken BEFORE chain_xyz is touched: a chain that does not win it never writes the buffer another chain is
        # still uploading from
        self._ar = ar if ar.lease("chain") else None
        self.ctx = None
        self.rows = self.spare = self.orig = self.mask = self.pristine = self._md = self._st = None
        self._pool = []
        try:
            if resident is None and table is not None:
                n_t = len(table)
                # (exact=False: a row filter may start the chain on any table; DataProcessor checks f32_inexact_field before SOR, the
                #  density filter or the box take the float32 copy for the table's values)
                if n_t >= 4096 and self._ar is not None:
                    a = host_gather_xyz(table, out=ar.pinned("chain_xyz", 12 * n_t)[:12 * n_t].view(np.float32).reshape(n_t, 3), exact=False)
                else:
                    a = host_gather_xyz(table, exact=False)
            self._setup(a, device, keep_pristine, table is not None or resident is not None)
        except BaseException:
            self.close()                    # (gives the lease back; a private context and its buffers are freed)
            raise

    def _setup(self, a, device, keep_pristine, pinned_source):
        self.ctx = self._ar.context("chain") if self._ar is not None else Context(device)
        self._names = iter(range(1 << 30))
        self.ctx.set_param("adaptive", 1)   # every step below synchronises anyway
        rr = self.resident
        self.n0 = self.n = rr.n if rr is not None else int(a.shape[0])
        nbytes = 12 * self.n0
        self.rows = self._alloc(max(nbytes, 16), "rows")
        if rr is not None:
            rows_columns_dev(self.ctx, rr.ptr, rr.first_byte, rr.dtype, rr.n, ("x", "y", "z"), self.rows.ptr)
        elif nbytes >= (32 << 20) and not pinned_source:      # through the pinned staging lanes: a caller's array is pageable memory
            check(self.ctx.lib.gsx_dev_upload_staged(self.ctx.handle, self.rows.ptr, a.ctypes.data, nbytes), "gsx_dev_upload_staged")
        else:
            self.rows.upload(a)
        self.spare = self._alloc(max(nbytes, 16), "spare")
        # bench.py only: a second device copy of the uploaded rows, so that restart() can run the chain again without PCIe
        self.pristine = self._alloc(max(nbytes, 16), "pristine") if keep_pristine else None
        if self.pristine is not None:
            check(self.ctx.lib.gsx_dev_copy(self.ctx.handle, self.pristine.ptr, self.rows.ptr, nbytes), "gsx_dev_copy")
        self.orig = None                    # None = identity
        self._pool = []                     # survivor-list buffers not in use (4 n0 bytes each; at most two ever exist)
        self.empty = False                  # keep_none(): no survivor, whatever self.orig says
        self.mask = self._alloc(self.n0 + 16, "mask")
        self._md = self._st = None          # SOR work buffers (mean distances, statistics), allocated on first use
        self._pristine_box = None           # box of the uploaded rows, when it was measured before any filter ran (restart() keeps it)
        self._box = None                    # box of the rows at the first density_filter() (a superset of every LATER state of the
                                            # chain; restart() drops it).  gsx_density_filter_dev re-derives the frame itself when
                                            # a row falls outside the box it was given (status word `oob` of the device result)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _alloc(self, nbytes: int, name: str):
        """a named grow-only buffer of the arena while this chain holds its lease, an allocation of its own otherwise"""
        if self._ar is not None:
            return self._ar.buf("chain_" + name, nbytes)
        return self.ctx.alloc(nbytes)

    def _free(self, b):
        if b is not None and self._ar is None:
            b.free()

    def restart(self):
        """back to the state right after the upload (needs keep_pristine): device-to-device copy, identity survivor list"""
        if self.pristine is None:
            raise ValueError("DeviceChain(keep_pristine=True) is needed for restart()")
        check(self.ctx.lib.gsx_dev_copy(self.ctx.handle, self.rows.ptr, self.pristine.ptr, 12 * self.n0), "gsx_dev_copy")
        if self.orig is not None:
            self._pool.append(self.orig)
        self.orig = None
        self.n, self.empty = self.n0, False
        # the cached box is the box of the rows that were current at the first density_filter() -- after a restart the
        # pristine rows may reach beyond it: back to the box of the PRISTINE rows if that is what was
        # measured (no filter had run yet), else to "not measured"
        self._box = self._pristine_box

    def _xyz(self):
        p = self.rows.ptr
        return p, p + 4, p + 8, 3

    def bbox(self):
        """per-axis (min, max) of the surviving rows -> ([3], [3]) float32: by value what np.min / np.max give on each column (the
        sign of a zero extreme is not defined).  gsx_slab_bbox_dev (the multi-GPU path's box kernel) drops NaNs: when its flag
        reports a non-finite coordinate, the rows come back and numpy reduces them -- an axis that holds a NaN is nan"""
        lo, hi = self._bbox_dev()
        if self.bbox_nonfinite:
            rows = self.rows.download(np.float32, 3 * self.n).reshape(-1, 3)
            lo, hi = list(np.min(rows, axis=0)), list(np.max(rows, axis=0))
        return lo, hi

    def _bbox_dev(self):
        """the box kernel's answer as it is: per-axis (min, max) of the surviving rows without their NaNs, and bbox_nonfinite"""
        out = self._alloc(32, "bbox")
        try:
            x, y, z, st = self._xyz()
            check(self.ctx.lib.gsx_slab_bbox_dev(self.ctx.handle, x, y, z, st, self.n, out.ptr), "gsx_slab_bbox_dev")
            b = out.download(np.float32, 7)
        finally:
            self._free(out)
        self.bbox_nonfinite = bool(b[6] != 0)      # a NaN or an infinity among the coordinates (numpy's min / max would propagate a NaN)
        return [-b[0], -b[1], -b[2]], [b[3], b[4], b[5]]

    def density_voxels(self, voxel_size: float, min_points: int):
        n = self.n
        dense_cap = int(min(n, n // max(int(min_points), 1) + 1))
        keys = np.empty((max(dense_cap, 1), 3), dtype=np.int64)
        counts = np.empty(max(dense_cap, 1), dtype=np.int64)
        nu, nd = C.c_int64(), C.c_int64()
        x, y, z, st = self._xyz()
        check(self.ctx.lib.gsx_density_voxels_dev(self.ctx.handle, x, y, z, st, n, float(voxel_size), int(min_points), dense_cap,
                                                  C.byref(nu), C.byref(nd), keys.ctypes.data, counts.ctypes.data), "gsx_density_voxels_dev")
        m = int(nd.value)
        return {"n_unique": int(nu.value), "dense_keys": keys[:m].copy(), "dense_counts": counts[:m].copy()}

    def density_filter(self, voxel_size: float, min_points: int, keep_multicluster: bool):
        """the whole density filter on the device (gsx_density_filter_dev) -> dict(status, n_unique, kept_clusters, largest,
        left: rows after the compaction) ; status DENSITY_HOST (more than 1024 dense voxels, or a tie for the largest cluster):
        nothing was applied, take density_filter_large"""
        return self._density_filter("gsx_density_filter_dev", voxel_size, min_points, keep_multicluster)

    def density_filter_large(self, voxel_size: float, min_points: int, keep_multicluster: bool):
        """density_filter for any number of dense voxels (gsx_density_filter_large_dev: union-find over the voxel table), the same
        dict; status DENSITY_HOST only for a tie for the largest cluster without keep_multicluster: nothing was applied, take the
        host path"""
        return self._density_filter("gsx_density_filter_large_dev", voxel_size, min_points, keep_multicluster)

    def _density_filter(self, entry: str, voxel_size: float, min_points: int, keep_multicluster: bool):
        if self._box is None:     # box of the rows as they are now: a superset of whatever survives later filters
            lo, hi = self._bbox_dev()
            self._box = np.array(list(lo) + list(hi), dtype=np.float32)
            if self.orig is None and not self.empty:     # nothing has been removed yet: this IS the box of the uploaded rows
                self._pristine_box = self._box
        info = DensityInfo()
        x, y, z, st = self._xyz()
        check(getattr(self.ctx.lib, entry)(self.ctx.handle, x, y, z, st, self.n, float(voxel_size), int(min_points),
                                           1 if keep_multicluster else 0, self._box.ctypes.data, self.mask.ptr, C.byref(info)), entry)
        out = {"status": int(info.status), "n_unique": int(info.n_unique), "kept_clusters": int(info.kept_clusters),
               "largest": int(info.largest), "left": None}
        if info.status == DENSITY_OK:
            out["left"] = self._compact()
        return out

    def _compact(self) -> int:
        out = self._pool.pop() if self._pool else self._alloc(4 * self.n0 + 16, "list%d" % next(self._names))
        n_out = C.c_int64()
        check(self.ctx.lib.gsx_compact_rows_dev(self.ctx.handle, self.rows.ptr, self.orig.ptr if self.orig is not None else None,
                                                self.mask.ptr, self.n, self.spare.ptr, out.ptr, C.byref(n_out)),
              "gsx_compact_rows_dev")
        self.rows, self.spare = self.spare, self.rows
        if self.orig is not None:
            self._pool.append(self.orig)    # the previous survivor list is free again
        self.orig = out
        self.n = int(n_out.value)
        return self.n

    def density_keep(self, voxel_size: float, kept_keys: np.ndarray) -> int:
        kk = np.ascontiguousarray(kept_keys, dtype=np.int64).reshape(-1, 3)
        x, y, z, st = self._xyz()
        check(self.ctx.lib.gsx_density_mask_dev(self.ctx.handle, x, y, z, st, self.n, float(voxel_size), kk.ctypes.data, len(kk),
                                                self.mask.ptr), "gsx_density_mask_dev")
        return self._compact()

    def keep_none(self):
        """a filter removed every row (reference: ``self.data = self.data[:0]``, data_processor.py:54-57,91-93).
        ``orig`` may still be None (= identity) when this is the first filter of the chain, so emptiness is its own flag."""
        self.n = 0
        self.empty = True

    def bbox_keep(self, bounds6) -> int:
        """crop_by_bbox (data_processor.py:215-224): bounds as numpy would see them -- Python floats are weak scalars
        (rounded to float32 before the comparison), numpy float64 scalars promote the comparison to f64"""
        b = np.array([float(np.float32(v)) if type(v) in (float, int) else float(v) for v in bounds6], dtype=np.float64)
        check(self.ctx.lib.gsx_mask_bbox_dev(self.ctx.handle, self.rows.ptr, self.n, b.ctypes.data, self.mask.ptr), "gsx_mask_bbox_dev")
        return self._compact()

    def resident_column(self, name: str):
        """the '<f4' field `name` of the resident rows the chain started from as a device column for ge_keep (the chain's buffer
        "column": the next ge_keep or resident_column overwrites it; a private one is freed by ge_keep)"""
        rr = self.resident
        dev = self._alloc(max(4 * self.n0, 16), "column")
        rows_columns_dev(self.ctx, rr.ptr, rr.first_byte, rr.dtype, rr.n, (name,), dev.ptr)
        return dev

    def resident_rgb(self, names3) -> "DeviceArray | None":
        """add_rgb_from_sh's colours of EVERY resident row the chain started from, out of its '<f4' fields `names3`, left in HBM
        (resident_rgb_dev, in the sizes it asks for) -> the (n0, 3) uint8 device array for take() or rgb_to_host(), which
        release it; None when more uncertain elements were listed than the list holds: the caller computes them on the host"""
        n = self.n0
        d_fdc, d_rgb = self._alloc(12 * n + 16, "fdc"), self._alloc(3 * n + 16, "rgb")
        d_list, d_cnt = self._alloc(4 * (3 * n // 64 + 4096), "rgblist"), self._alloc(16, "rgbcnt")
        done = None
        try:
            done = resident_rgb_dev(self.ctx, self.resident, names3, d_fdc, d_rgb, d_list, d_cnt)
        finally:
            for b in (d_fdc, d_list, d_cnt) + ((d_rgb,) if done is None else ()):
                self._free(b)
        return d_rgb if done is not None else None

    def rgb_to_host(self, d_rgb: DeviceArray) -> np.ndarray:
        """resident_rgb()'s colours as a host (n0, 3) uint8 array; the device array is released"""
        try:
            return d_rgb.download(np.uint8, 3 * self.n0).reshape(self.n0, 3)
        finally:
            self._free(d_rgb)

    def take(self, zero_names=(), rgb=None, stage_ms: "dict | None" = None) -> "ResidentRows | None":
        """The chain's survivors out of the resident rows it started from, as NEW resident rows (ResidentRows.take on the chain's
        context; the caller's to close): the composed survivor list when a filter removed rows, every row when none did, no row
        after keep_none().  rgb: None, resident_rgb()'s device colours, or a host (n0, 3) uint8 array (uploaded into the chain's
        "rgbhost") -- one row per ORIGINAL row, appended to the survivors as red, green, blue.  The colour buffers are released on
        every way out; the source rows and the chain stay open.  None when the widened rows cannot be written."""
        compact = self.n != self.n0 or self.empty
        n_out = 0 if (self.empty or self.n == 0) else self.n
        device_rgb = rgb if isinstance(rgb, DeviceArray) else None
        uploaded = None
        try:
            if rgb is not None and device_rgb is None and n_out:
                uploaded = self._alloc(3 * self.n0 + 16, "rgbhost").upload(np.ascontiguousarray(rgb, np.uint8))
            extra = device_rgb if device_rgb is not None else uploaded
            return self.resident.take(self.orig.ptr if (self.orig is not None and compact) else None, n_out, zero_names,
                                      extra.ptr if extra is not None else None, ("red", "green", "blue") if rgb is not None else (),
                                      ctx=self.ctx, stage_ms=stage_ms)
        finally:
            self._free(uploaded)
            self._free(device_rgb)

    def decimate(self, plan, zero_names=(), stage_ms: "dict | None" = None) -> "ResidentRows":
        """The voxel decimation `plan` of the chain's survivors out of the resident rows it started from, as NEW resident rows
        (ResidentRows.decimate on the chain's context; the caller's to close): the key kernel reads the rows through the composed
        survivor list, so the table before the decimation is neither taken nor downloaded.  The source rows and the chain stay
        open."""
        compact = self.n != self.n0 or self.empty
        n = 0 if (self.empty or self.n == 0) else self.n
        idx = self.orig.ptr if (self.orig is not None and compact and n) else None
        return self.resident.decimate(plan, idx, n, zero_names, ctx=self.ctx, stage_ms=stage_ms)

    def ge_keep(self, column, threshold: float) -> int:
        """rows whose value in ``column`` (float32, one per row of the table the chain started from) is >= threshold; column: a
        host array, or resident_column()'s device column"""
        if isinstance(column, DeviceArray):
            dev = column
        else:
            col = np.ascontiguousarray(column, dtype=np.float32)
            if col.shape != (self.n0,):
                raise ValueError("column must have one value per original row")
            dev = self._alloc(max(col.nbytes, 16), "column").upload(col)
        try:
            check(self.ctx.lib.gsx_mask_ge_dev(self.ctx.handle, dev.ptr, self.orig.ptr if self.orig is not None else None, self.n,
                                               float(threshold), self.mask.ptr), "gsx_mask_ge_dev")
            return self._compact()
        finally:
            self._free(dev)

    def view_prune(self, plans, rows: "ResidentRows | None" = None, min_contribution: "float | None" = None,
                   max_count: "int | None" = None, stage_ms: "dict | None" = None) -> dict:
        """One scoring pass and what is asked of it, on a chain no filter has removed a row from: the view scores
        of `rows` -- the resident rows the chain started from, or other rows in HBM that are the chain's table row for row --
        over `plans` into the chain's "view_peak" and "view_total" (ResidentRows.view_scores_into on the chain's context); then
        with `min_contribution` the rows whose peak is >= float32(min_contribution) are kept (ge_keep with the peaks as the
        column), and with `max_count` the budget ranks what is left by that pass's totals (gsx_view_keys_dev into "limit_keys",
        limit_keep(keys=)).  The scoring comes first and is all that can refuse (render.RenderRefused): the chain is then as it
        was.  -> the scoring's info and never_seen (rows whose peak is 0), after_filter (rows the threshold left, None without
        one), limit (limit_keep's dict, None without a budget)."""
        rows = rows if rows is not None else self.resident
        n0 = self.n0
        if self.n != n0 or self.orig is not None or self.empty or rows is None or rows.n != n0:
            raise ValueError("DeviceChain.view_prune: a chain that has removed no row, and rows that are its table's")
        d_peak, d_total = self._alloc(max(4 * n0, 16), "view_peak"), self._alloc(max(8 * n0, 16), "view_total")
        d_keys = None
        try:
            check(self.ctx.lib.gsx_dev_memset(self.ctx.handle, d_peak.ptr, 0, max(4 * n0, 16)), "gsx_dev_memset")
            check(self.ctx.lib.gsx_dev_memset(self.ctx.handle, d_total.ptr, 0, max(8 * n0, 16)), "gsx_dev_memset")
            out = rows.view_scores_into(plans, d_peak.ptr, d_total.ptr, stage_ms=stage_ms, ctx=self.ctx)
            out["never_seen"] = int(np.count_nonzero(d_peak.download(np.uint32, n0) == 0))
            out["after_filter"] = out["limit"] = None
            if min_contribution is not None:
                peaks, d_peak = d_peak, None        # (ge_keep releases its column)
                out["after_filter"] = self.ge_keep(peaks, float(np.float32(min_contribution)))
            if max_count is not None:
                if limit_count(max_count) < self.n:
                    d_keys = self._alloc(max(4 * n0, 16), "limit_keys")
                    check(self.ctx.lib.gsx_view_keys_dev(self.ctx.handle, d_total.ptr, n0, d_keys.ptr), "gsx_view_keys_dev")
                out["limit"] = self.limit_keep(max_count, keys=d_keys)
            return out
        finally:
            for b in (d_peak, d_total, d_keys):
                self._free(b)

    def limit_keep(self, max_count: int, columns: "np.ndarray | None" = None, keys: "DeviceArray | None" = None) -> dict:
        """the splat budget (csrc/limit.hip): of the rows the chain has, the `max_count` with the smallest .splat sort keys, equal
        keys by row index, in input order.  The keys are those of EVERY row the chain started from: their (n0, 4) LIMIT_FIELDS
        gathered out of the resident rows on the device, or `columns` (limit_columns_host of the host table) uploaded once, into
        the chain's "limit_cols"; the keys go to "limit_keys" and the select reads them through the survivor list.  Both buffers
        are released like "column".  keys: a device array of one uint32 per ORIGINAL row (the caller's: not released here), used
        instead of the metric's keys -- gsx_view_keys_dev's for the ranking by views.  -> dict(kept, threshold, ties_kept,
        threshold_key)"""
        max_count = limit_count(max_count)
        n0 = self.n0
        if max_count >= self.n:             # nothing to remove: no device work
            return {"kept": self.n, "threshold": None, "ties_kept": 0, "threshold_key": None}
        if keys is not None:
            out = limit_select_dev(self.ctx, keys.ptr, self.orig.ptr if self.orig is not None else None, self.n, max_count, self.mask.ptr)
            out["kept"] = self._compact()
            return out
        d_cols, d_keys = self._alloc(max(16 * n0, 16), "limit_cols"), self._alloc(max(4 * n0, 16), "limit_keys")
        try:
            rr = self.resident
            if rr is not None:
                rows_columns_dev(self.ctx, rr.ptr, rr.first_byte, rr.dtype, rr.n, LIMIT_FIELDS, d_cols.ptr)
            else:
                cols = np.ascontiguousarray(columns, dtype=np.float32)
                if cols.shape != (n0, 4):
                    raise ValueError("columns must hold scale_0, scale_1, scale_2, opacity of every original row")
                d_cols.upload(cols)
            limit_keys_dev(self.ctx, d_cols.ptr, n0, d_keys.ptr)
            out = limit_select_dev(self.ctx, d_keys.ptr, self.orig.ptr if self.orig is not None else None, self.n, max_count, self.mask.ptr)
            out["kept"] = self._compact()
            return out
        finally:
            self._free(d_cols)
            self._free(d_keys)

    def sor_keep(self, k: int, threshold_factor: float):
        numpy_reduction_selfcheck(self.ctx)
        n = self.n
        if self._md is None:                # sized for the whole table once: no allocation in later calls
            self._md, self._st = self._alloc(4 * self.n0 + 16, "md"), self._alloc(16, "st")
        md, st = self._md, self._st
        x, y, z, stride = self._xyz()
        self.ctx.sor_knn(x, y, z, stride, n, 0, n, int(k), md.ptr)
        self.ctx.sor_stats(md.ptr, n, float(threshold_factor), st.ptr)
        self.ctx.sor_mask(md.ptr, n, st.ptr + 8, self.mask.ptr)
        self.ctx.check()
        stats = st.download(np.float32, 3)
        kept = self._compact()
        return {"mean": stats[0], "std": stats[1], "threshold": stats[2], "kept": kept}

    def survivors(self) -> np.ndarray:
        """indices (ascending) of the surviving rows in the table the chain started from"""
        if self.empty or self.n == 0:
            return np.zeros(0, np.uint32)
        if self.orig is None:
            return np.arange(self.n0, dtype=np.uint32)
        return self.orig.download(np.uint32, self.n) if self.n else np.zeros(0, np.uint32)

    def close(self):
        if self._ar is not None:             # the arena keeps the buffers and the context (and its KNN workspace) for the next chain
            ar, self._ar = self._ar, None
            healthy = self.ctx is None      # (nothing ran on the context yet: a failed gather)
            if self.ctx is not None and self.ctx.handle:
                try:
                    self.ctx.set_param("adaptive", 0)
                    self.ctx.synchronize()
                    healthy = True
                except GsxError:
                    pass
            ar.unlease("chain")
            self.ctx = None
            if not healthy:                  # a failed HIP call somewhere in this chain: do not hand the context on
                release_arenas()
            return
        if self.ctx is None:
            return
        for b in (self.rows, self.spare, self.orig, self.mask, self.pristine, self._md, self._st, *self._pool):
            if b is not None:
                b.free()
        self.ctx.close()
        self.ctx = None
