"""``DataProcessor`` -- same name, signatures, messages and error behaviour as the reference's
gsconverter/processing/data_processor.py, with the two heavy filters running on the MI355X:

  * ``remove_flyers``        (reference :119-182)  -> gsx_sor_filter        (exact KNN, HIP)
  * ``apply_density_filter`` (reference :11-117)   -> gsx_density_voxels / gsx_density_mask

Differences from the reference, all deliberate:
  * ``remove_flyers`` APPLIES the survivor mask.  The reference's CPU branch computes the
    mask at :180 and returns the data unfiltered (:181-182); its GPU branch
    applies it (:149).  This class follows the GPU branch.
  * the KNN is exact (cKDTree semantics), not the Taichi kernel's 27-cell approximation
    (SURVEY.md F4/F5); any k up to 2047 (k <= 64 on the fast kernels).
  * there is NO CPU fallback: if the HIP library or the GPU is missing the call raises
    ``GsxError`` (a RuntimeError).
  * coordinates the device cannot take without changing the answer raise ``TypeError`` (before any device work): SOR
    takes x/y/z that float32 holds exactly, the density filter x/y/z that numpy promotes to float32 ("Field
    dtypes").  The row filters run the reference's numpy expressions on columns that are not float32.
Every method of the reference class is implemented here (round 3: ``cap_sh_degree``, ``add_rgb_from_sh``,
``apply_auto_bbox`` too -- SURVEY.md 8(f) rank 4); ``__getattr__`` only forwards names a FUTURE reference version
might add.

This class holds the reference's semantics -- messages, order of checks, return values -- and decides what ``.data`` still owes
the table; the device work behind it belongs to the objects that own the memory (``_lib.DeviceChain``, ``_lib.ResidentRows``).
"""
from __future__ import annotations

import contextlib

import numpy as np

from .. import _lib
from .. import decimate as _decimate
from .. import fidelity as _fidelity
from .. import render as _render
from .. import transform as _transform
from .. import views as _views
from ..utils import debug_print, status_print
from . import clusters as _clusters


XYZ = ("x", "y", "z")
RGB = ("red", "green", "blue")
DEVICE_CLUSTERS_ABOVE = 1024  # eager density filter: more dense voxels than this are clustered by gsx_voxel_clusters, fewer by clusters.py
MAX_SOR_K = 2047  # include/gsx_hip.h: 1 <= k <= 64 on the fast kernels, 65..2047 through the exact list-free kernel (slow)


def sor_params_from_intensity(intensity):
    """reference :125-134 (intensity 5 -> (27, 12.44), not the (25, 10.5) of its comment)."""
    k = int(10 + (intensity - 1) * (40 / 9))
    threshold_factor = 20.0 - (intensity - 1) * (17.0 / 9)
    return k, threshold_factor


def density_params_from_sensitivity(sensitivity):
    """reference :24-28."""
    voxel_size = max(0.1, 2.0 - (sensitivity * 1.8))
    threshold_percentage = 0.1 + (sensitivity * 0.9)
    return voxel_size, threshold_percentage


_REFERENCE_CLASS = None  # set by install() before it rebinds gsconverter's name to this class


def _reference_class():
    global _REFERENCE_CLASS
    if _REFERENCE_CLASS is None:
        from gsconverter.processing.data_processor import DataProcessor as ref  # type: ignore
        if ref.__module__.startswith("gsconverter"):
            _REFERENCE_CLASS = ref
        else:
            raise ImportError("gsconverter.processing.DataProcessor is already the HIP drop-in")
    return _REFERENCE_CLASS


@contextlib.contextmanager
def _xyz_rows(vertices, names=("x", "y", "z"), buf_name="eager_xyz"):
    """reference :38/:139 `coords` -- ``with _xyz_rows(vertices) as xyz:`` (N,3) float32, gathered from the AoS table by the threaded C
    routine.  Large tables: into a page-locked staging buffer the arena keeps (round 6: a fresh 12n-byte array costs as much to fault
    in, copy from at pageable rate and unmap again as the filter itself), under the lease of the buffer's group for the whole block --
    another thread's filter at the same moment gathers into a fresh array instead of over (or, growing the buffer, freeing) this one"""
    n = len(vertices)
    ar = _lib.arena(0) if n >= 65536 and isinstance(vertices, np.ndarray) else None
    with ar.leased(ar.group(buf_name)) if ar is not None else contextlib.nullcontext(False) as won:
        out = None
        if won:
            try:
                out = ar.pinned(buf_name, 12 * n)[:12 * n].view(np.float32).reshape(n, 3)
            except _lib.GsxError:
                out = None              # no device: the callers' device entry points say so themselves
        yield _lib.host_gather_xyz(vertices, names, out=out)


def _require_sor_k(k):
    """the reference's cKDTree path takes any k and its Taichi kernel silently caps K at 50 (gpu_ops.py:244); here k <= 64 runs on
    the register-resident kernels, 65..2047 on the exact list-free kernel"""
    if not 1 <= int(k) <= MAX_SOR_K:
        raise ValueError(f"SOR: k={k} is outside the supported range 1..{MAX_SOR_K} of the MI355X path "
                         f"(--sor_intensity maps to k = 10..50, the CLI default is 25)")


def _host_clusters(dense_keys, keep_multicluster):
    """the density filter's clustering on the host (clusters.py: the reference's set-iteration order decides a tie for the largest)
    -> (keys of the kept voxels (m, 3) int64 in np.unique's row order, clusters kept, voxels of the largest), or None when no
    cluster is kept"""
    comps = _clusters.connected_clusters(map(tuple, dense_keys.tolist()))
    kept, kept_clusters, max_len = _clusters.select_clusters(comps, keep_multicluster)
    if not kept:
        return None
    return np.array(sorted(kept), dtype=np.int64).reshape(-1, 3), kept_clusters, max_len


class DataProcessor:
    """Drop-in for the reference's class (module docstring).  ``lazy=True`` (what ``install()`` gives the reference's orchestrator, which ignores the filters' return values,
    converter.py:196-236): consecutive density / SOR filters keep the coordinates in HBM (``_lib.DeviceChain``) and the
    host table is compacted ONCE, when ``.data`` is read -- SURVEY.md 8(f) rank 1.  The filter methods then return
    ``None``.  Default (eager): every method updates and returns ``self.data`` like the reference."""

    lazy_default = False

    def __init__(self, data, lazy=None, resident=None):
        """resident: the rows of `data` in HBM as a reader kept them (_lib.ResidentRows; this object owns them from here on and
        ``close()`` frees them).  A lazy processor then gathers the chain's coordinates, the alpha filter's column and the colours'
        f_dc from those rows on the device, and ``.data`` is ONE gsx_rows_take_dev -- survivors, zeroed fields, colours -- and
        one download; ``.resident`` is the rows of ``.data`` in HBM.  Rows that are not `data`'s (_lib.resident_eligible), or an
        eager processor: closed here, and everything runs as without them."""
        self._rr = None             # the rows of self._data in HBM (owned), or None: the host path
        self.resident_ms = {}       # clocks of the resident path: gather, take, download
        if resident is not None:
            lazy_now = DataProcessor.lazy_default if lazy is None else bool(lazy)
            if (lazy_now and isinstance(data, np.ndarray) and data.ndim == 1 and not resident.closed
                    and _lib.resident_eligible(resident.dtype, resident.n, data.dtype, len(data))):
                self._rr = resident
            else:
                resident.close()
        self._data = data
        self._chain = None          # _lib.DeviceChain over the rows of self._data, or None
        self._pending_zero = []     # lazy cap_sh_degree: columns to zero once the host table has been compacted
        self._pending_rgb = None    # lazy add_rgb_from_sh: (n0, 3) u8 colours of the UNcompacted table (a host array, or the chain's
        #                             device array), appended by the compaction pass
        self._host_stale = False    # lazy apply_transform moved the rows in HBM: the host table still holds the old frame, and
        #                             .data owes a download even when no filter removes a row
        self.lazy = DataProcessor.lazy_default if lazy is None else bool(lazy)

    @property
    def data(self):
        self._materialize()
        return self._data

    @data.setter
    def data(self, value):
        # a deferred cap_sh_degree belongs to the table it was called on: the reference zeroes that table at once
        # (data_processor.py:313), so it is applied to the OLD table before the new one replaces it
        # -- unless a filter's compaction is still pending in the chain: the reference had by then replaced self.data
        # with the filtered COPY and zeroed that, leaving the caller's array alone; the copy would be discarded here, so
        # the pending fills are simply dropped
        if self._pending_zero and isinstance(self._data, np.ndarray) and not self._compaction_pending():
            names, self._pending_zero = self._pending_zero, []
            _lib.host_zero_columns(self._data, names)
        self._pending_zero = []
        self._pending_rgb = None
        self._host_stale = False
        self._drop_chain()
        self._drop_resident()       # (the rows in HBM were the old table's)
        self._data = value

    @property
    def resident(self):
        """the rows of ``.data`` in HBM (_lib.ResidentRows, this object's: ``close()`` frees them), or None whenever the host path
        produced ``.data``"""
        self._materialize()
        return self._rr

    def close(self):
        """give the device chain and the resident rows back (idempotent; ``.data`` stays: a transform the rows in HBM took and
        the host table has not seen yet is materialised first)"""
        if self._host_stale and self._rr is not None:
            self._materialize()
        self._drop_chain()
        self._drop_resident()

    def _drop_chain(self):
        if self._chain is not None:
            self._chain.close()
            self._chain = None

    def _drop_resident(self):
        if self._rr is not None:
            rr, self._rr = self._rr, None
            rr.close()

    def _timed(self, name, ctx=None):
        """``with self._timed("gather", ctx):`` -- the block's milliseconds, after a synchronisation of `ctx` when one is given,
        added to resident_ms[name]"""
        return _lib.stage_clock(self.resident_ms, name, ctx)

    def _compaction_pending(self):
        """has a filter of the device chain removed rows that the table still holds?  A chain is only ever built over a table
        that has rows, so this holds after keep_none() (n = 0) too"""
        return self._chain is not None and self._chain.n != self._chain.n0

    def _materialize(self):
        """``.data``'s pending work, decided once for both executors: the chain's survivor list when a filter removed rows, the
        fields cap_sh_degree deferred and the colours add_rgb_from_sh deferred.  On the rows in HBM (_take_resident) when this
        object has them and they can take it, else on the host table (_take_host).  The chain is closed either way; a take's
        new rows replace the source rows, which are closed, after that."""
        compact, ch, zero, rgb = self._compaction_pending(), self._chain, self._pending_zero, self._pending_rgb
        stale = self._host_stale and self._rr is not None
        self._chain, self._pending_zero, self._pending_rgb, self._host_stale = None, [], None, False
        taken = None
        try:
            if self._rr is not None:
                if not (compact or zero or rgb is not None):
                    if stale:
                        self._data = self._download_resident()  # (the transformed rows: a new table, the caller's stays)
                    self.resident_ms.setdefault("take", 0.0)    # (the resident path ran, and had nothing to take)
                    return                                      # .data is the table, .resident its rows
                new_dtype = _lib.resident_take_dtype(self._rr.dtype, RGB if rgb is not None else ())
                if new_dtype is not None and (rgb is None or ch is not None):   # (only a chain can hand colours to the take)
                    taken = self._take_resident(ch, zero, rgb, new_dtype)
                else:
                    # this table is not taken (the widened row does not end in the three bytes, or is too long): device colours
                    # come to the host, the resident rows are dropped and the host path runs
                    if isinstance(rgb, _lib.DeviceArray):
                        rgb = ch.rgb_to_host(rgb)
                    if stale:
                        self._data = self._download_resident()
                    self._drop_resident()
            if taken is None:
                self._take_host(ch if compact else None, zero, rgb)
        finally:
            if ch is not None:
                ch.close()
        if taken is not None:
            self._drop_resident()
            self._data, self._rr = taken

    def _download_resident(self):
        """the rows in HBM as a new, prefaulted host table (one download, clock "download"); when it raises the rows are closed"""
        try:
            out = np.empty(self._rr.n, self._rr.dtype)
            join = _lib.prefault_parallel(out)
            with self._timed("download"):
                join()
                self._rr.download_into(out)
        except BaseException:
            self._drop_resident()
            raise
        return out

    def _take_resident(self, ch, zero, rgb, new_dtype):
        """the pending work on the rows in HBM: one take -- the chain's when there is one, the rows' own otherwise -- into new
        resident rows and one download into a prefaulted table of `new_dtype` -> (the table, its rows in HBM).  When anything
        raises the new rows and the source rows are closed"""
        n_out = ch.n if ch is not None else self._rr.n
        out_rr = None
        try:
            out = np.empty(n_out, new_dtype)
            join = _lib.prefault_parallel(out)
            out_rr = (ch.take(zero, rgb, stage_ms=self.resident_ms) if ch is not None
                      else self._rr.take(None, n_out, zero, stage_ms=self.resident_ms))
            if n_out:
                with self._timed("download"):
                    join()
                    out_rr.download_into(out)
            else:
                self.resident_ms.setdefault("take", 0.0)        # (no survivor: nothing to take)
        except BaseException:
            if out_rr is not None:
                out_rr.close()
            self._drop_resident()
            raise
        return out, out_rr

    def _take_host(self, ch, zero, rgb):
        """the pending work on the host table: the survivor list of `ch` (None: no compaction is pending) applied in one threaded
        pass, then the deferred column fills of cap_sh_degree on the rows that are left"""
        if ch is not None:
            # the chain's survivor list (ascending row indices) applied to the host table directly -- round 5: the
            # boolean mask numpy would index with (`mask[survivors] = True` on 8M indices) cost more than the compaction
            if rgb is not None or zero:
                # round 6: ... and add_rgb_from_sh's widened copy (:262-274; the reference's converter calls it after the filters
                # for every target that needs colours, converter.py:243-252) and cap_sh_degree's deferred column fill (:310-313)
                # in the same pass: one read of the survivors, one write of the new table
                self._data = _lib.host_take_rows_shape(self._data, ch.survivors(), RGB if rgb is not None else (), rgb, zero)
                rgb, zero = None, []
            else:
                self._data = _lib.host_take_rows(self._data, ch.survivors())
        if rgb is not None:
            self._data = _lib.host_append_u8_columns(self._data, RGB, rgb)
        if zero and isinstance(self._data, np.ndarray):
            _lib.host_zero_columns(self._data, zero)    # in place, like the reference (:313): the caller's array when
            #                                             no filter has compacted the table, the compacted copy otherwise

    def _chain_for(self, vertices):
        if self._chain is None:
            if self._rr is not None:                            # (coords gathered out of the rows in HBM)
                with self._timed("gather"):
                    self._chain = _lib.DeviceChain(resident=self._rr)
                    self._chain.ctx.synchronize()
            else:
                self._chain = _lib.DeviceChain(table=vertices)  # (coords gathered straight into a page-locked staging buffer)
        return self._chain

    def _columns(self, names):
        """the named columns of the (materialised) table as contiguous arrays: one threaded pass (gsx_host_gather_columns_f32) for
        float32 fields of a plain table, numpy's own copies otherwise.  Same values, so numpy's elementwise expressions on them give
        what they give on the strided views the reference uses.  Reductions only by value: np.min / np.max over zeros of both signs
        may return a different zero for a contiguous array than for a strided view of the same values (numpy 2.2.6), so a zero
        extreme is taken from the strided view (apply_auto_bbox)"""
        d = self.data
        fields = d.dtype.fields or {}
        if isinstance(d, np.ndarray) and d.ndim == 1 and len(d) >= 4096 and all(nm in fields and fields[nm][0] == np.dtype("<f4") for nm in names):
            return list(_lib.host_gather_columns(d, list(names)))
        return [d[nm] for nm in names]

    def _column(self, name):
        return self._columns((name,))[0]

    def _require_sor_dtypes(self):
        """remove_flyers' refusal ("Field dtypes"): the reference's cKDTree measures in float64 whatever the table holds
        (:139,156), so the device's float32 coordinates give its mask exactly when float32 holds every coordinate -- float32 fields
        of either byte order, float16, float64 fields whose values all come back from float32 (one host pass).  Anything else
        raises TypeError here, before the device or the table or the chain is touched"""
        bad = _lib.f32_inexact_field(self._data, XYZ)
        if bad is not None:
            raise TypeError(f"remove_flyers: field {bad[0]!r} is {bad[1].str} and holds values float32 does not; the reference's "
                            f"KD-tree measures them in float64, the MI355X path in float32 -- cast the table to float32 first "
                            f"if that is what is wanted")

    def _require_density_dtypes(self):
        """apply_density_filter's refusal: the reference divides np.column_stack((x, y, z)) -- numpy's promotion of the three
        dtypes -- by the voxel size (:38-39).  The device divides in float32, so only tables whose coordinates promote to float32
        (float32 of either byte order, float16 next to float32) are taken; anything else raises TypeError before any device work"""
        fields = self._data.dtype.fields or {}
        dts = [fields[f][0] for f in XYZ if f in fields]
        if len(dts) < 3 or _lib.is_f4(np.result_type(*dts)):
            return                      # (a missing field: numpy's own error, where the reference meets it)
        promoted = np.result_type(*dts)
        nm = next(f for f in XYZ if not _lib.is_f4(fields[f][0]))
        raise TypeError(f"apply_density_filter: field {nm!r} is {fields[nm][0].str}; the reference divides the coordinates in "
                        f"{promoted} (np.column_stack of x, y, z), the MI355X path in float32 -- a float64 division mode is not "
                        f"implemented")

    def _xyz_is_f32(self):
        names = self._data.dtype.names or ()
        return all(f in names and self._data.dtype[f] == np.float32 for f in ("x", "y", "z"))

    def _flush_rgb(self):
        """a deferred add_rgb_from_sh changes the table's dtype: any further method sees the table the reference would have by then"""
        if self._pending_rgb is not None:
            self._materialize()

    def __len__(self):   # rows currently surviving, without materialising
        if self._chain is not None:
            return self._chain.n
        if self._host_stale and self._rr is not None:   # (a decimation in HBM: the host table still has the rows before it)
            return self._rr.n
        return len(self._data)

    # ------------------------------------------------------------------ SOR
    def remove_flyers(self, k=25, threshold_factor=10.5, chunk_size=50000, intensity=None):
        debug_print("[DEBUG] Executing 'remove_flyers' function...")
        self._flush_rgb()
        if not isinstance(self._data, np.ndarray):
            raise TypeError("self.data must be a numpy structured array.")
        self._require_sor_dtypes()
        if intensity is not None:
            k, threshold_factor = sor_params_from_intensity(intensity)
        debug_print(f"SOR Filter (Remove Flyers) Params: K={k}, Sigma={threshold_factor:.2f}")

        if self.lazy and isinstance(self._data, np.ndarray) and len(self) > 0:
            _require_sor_k(k)
            ch = self._chain_for(self._data)
            num_points = ch.n
            status_print("[SOR] Determining outliers on GPU (HIP gfx950, exact KNN, device-resident chain)...")
            res = ch.sor_keep(int(k), float(threshold_factor))
            self.last_sor = {"mean": res["mean"], "std": res["std"], "threshold": res["threshold"]}
            status_print(f"After removing flyers (GPU), retained {res['kept']} out of {num_points} vertices.")
            return None
        vertices = self.data
        num_points = len(vertices)
        if num_points == 0:
            # the reference's GPU branch slices the empty table with an empty mask and reports it (:146-150)
            status_print("[SOR] Determining outliers on GPU (HIP gfx950, exact KNN)...")
            status_print("After removing flyers (GPU), retained 0 out of 0 vertices.")
            return self.data
        _require_sor_k(k)
        status_print("[SOR] Determining outliers on GPU (HIP gfx950, exact KNN)...")
        with _xyz_rows(vertices) as xyz:
            res = _lib.sor_filter(xyz, int(k), float(threshold_factor), want_mean=False)
        self.last_sor = {"mean": res["mean"], "std": res["std"], "threshold": res["threshold"]}
        self.data = _lib.host_compact_rows(vertices, res["mask"])  # reference :149
        status_print(f"After removing flyers (GPU), retained {len(self.data)} out of {num_points} vertices.")
        return self.data

    # ------------------------------------------------------------------ density
    def apply_density_filter(self, voxel_size=1.0, threshold_percentage=0.32, sensitivity=None,
                             keep_multicluster=False):
        debug_print("[DEBUG] Executing 'apply_density_filter' function...")
        self._flush_rgb()
        if not isinstance(self._data, np.ndarray):
            raise TypeError("self.data must be a numpy structured array.")
        self._require_density_dtypes()
        if sensitivity is not None:
            voxel_size, threshold_percentage = density_params_from_sensitivity(sensitivity)
        debug_print(f"Density Filter Params: Voxel={voxel_size:.4f}, Thresh={threshold_percentage:.4f}%, "
                    f"MultiCluster={keep_multicluster}")

        if self.lazy and len(self) > 0:
            return self._density_lazy(voxel_size, threshold_percentage, keep_multicluster)
        vertices = self.data
        n = len(vertices)
        min_points = int(n * (threshold_percentage / 100.0))  # reference :48
        if n == 0:
            return self._density_keeps_nothing()
        with _xyz_rows(vertices) as cols:        # (the staging buffer is held across both device calls)
            occ = _lib.density_voxels(cols, float(voxel_size), min_points)
            debug_print(f"[DEBUG] Found {occ['n_unique']} unique voxels.")
            if len(occ["dense_keys"]) == 0:
                return self._density_keeps_nothing()
            # more dense voxels than the reference's own thresholds can give (--density_threshold near 0: every occupied voxel
            # is dense): their clusters on the device too; only a tie for the largest comes back for the host steps
            res = (_lib.voxel_clusters(occ["dense_keys"], bool(keep_multicluster))
                   if len(occ["dense_keys"]) > DEVICE_CLUSTERS_ABOVE else None)
            if res is not None and res["status"] == _lib.DENSITY_OK:
                kept_keys = occ["dense_keys"][res["keep"]]      # (np.unique's row order already)
                kept_clusters, max_len = res["kept_clusters"], res["largest"]
            else:
                found = _host_clusters(occ["dense_keys"], keep_multicluster)
                if found is None:
                    return self._density_keeps_nothing(warn=False)
                kept_keys, kept_clusters, max_len = found
            mask = _lib.density_mask(cols, float(voxel_size), kept_keys)
        self.data = _lib.host_compact_rows(vertices, mask)  # reference :114
        status_print(f"Density Filter: Kept {kept_clusters} clusters (largest: {max_len} voxels).")
        status_print(f"After density filter, retained {len(self.data)} out of {len(vertices)} vertices.")
        return self.data

    def _density_keeps_nothing(self, ch=None, warn=True):
        """the density filter's exit when no row survives (reference :54-57, :91-93; without the warning when the dense voxels
        gave no cluster to keep): `ch`, the lazy filter's chain, keeps none; the eager filter sets and returns the empty table"""
        if warn:
            status_print("Warning: Density filter removed all points.")
        if ch is not None:
            ch.keep_none()
            return None
        self.data = self.data[:0]
        return self.data

    def _density_lazy(self, voxel_size, threshold_percentage, keep_multicluster):
        """the same steps on the device-resident rows; the host table is untouched until ``.data`` is read"""
        ch = self._chain_for(self._data)
        n = ch.n
        min_points = int(n * (threshold_percentage / 100.0))  # reference :48
        # the whole filter in one device call (occupancy, clusters of the dense voxels, keep rule, mask, compaction); > 1024
        # dense voxels come back undecided and take the call without a cap; only a tie for the largest cluster -- the
        # reference's set-iteration order decides it -- comes back from that one too and takes the steps below
        res = ch.density_filter(float(voxel_size), min_points, bool(keep_multicluster))
        if res["status"] == _lib.DENSITY_HOST:
            res = ch.density_filter_large(float(voxel_size), min_points, bool(keep_multicluster))
        if res["status"] != _lib.DENSITY_HOST:
            debug_print(f"[DEBUG] Found {res['n_unique']} unique voxels.")
            if res["status"] == _lib.DENSITY_EMPTY:
                return self._density_keeps_nothing(ch)
            kept_clusters, max_len, left = res["kept_clusters"], res["largest"], res["left"]
        else:
            occ = ch.density_voxels(float(voxel_size), min_points)
            debug_print(f"[DEBUG] Found {occ['n_unique']} unique voxels.")
            if len(occ["dense_keys"]) == 0:
                return self._density_keeps_nothing(ch)
            found = _host_clusters(occ["dense_keys"], keep_multicluster)
            if found is None:
                return self._density_keeps_nothing(ch, warn=False)
            kept_keys, kept_clusters, max_len = found
            left = ch.density_keep(float(voxel_size), kept_keys)
        status_print(f"Density Filter: Kept {kept_clusters} clusters (largest: {max_len} voxels).")
        status_print(f"After density filter, retained {left} out of {n} vertices.")
        return None

    # ------------------------------------------------------------------ O(N) row filters
    # Lazy mode (the orchestrator's): masks over the device-resident rows (chain.hip), composed with density / SOR into the
    # one host compaction at the end.  Eager mode: the reference's numpy expressions; only `self.data[mask]` -- 1.2 s per
    # call at 10M splats in numpy -- goes through the threaded C compaction.
    def apply_alpha_filter(self, min_opacity_u8):
        """reference :184-213"""
        self._flush_rgb()
        debug_print(f"[DEBUG] Executing 'apply_alpha_filter' with min={min_opacity_u8}")
        if 'opacity' not in self._data.dtype.names:
            status_print("Warning: No opacity channel found. Alpha filter skipped.")
            return
        limit = min_opacity_u8
        if limit <= 0:
            return
        if limit >= 255:
            self.data = self.data[:0]
            return
        alpha_thresh = np.clip(limit / 255.0, 1e-6, 1.0 - 1e-6)
        logit_thresh = np.log(alpha_thresh / (1.0 - alpha_thresh))
        if self.lazy and len(self) > 0 and self._data['opacity'].dtype == np.float32:
            ch = self._chain_for(self._data)
            original_len = ch.n
            # (the column leaves the 248-byte rows through the threaded gather: numpy's strided copy takes ~45 ms at 10M splats)
            if self._rr is not None:
                with self._timed("gather", ch.ctx):
                    column = ch.resident_column("opacity")
            else:
                column = _lib.host_gather_columns(self._data, ["opacity"])[0]
            left = ch.ge_keep(column, float(logit_thresh))   # np.float64 threshold: an f64 comparison
            status_print(f"Alpha Filter (min {limit}): Retained {left} out of {original_len} splats.")
            return None
        # eager (host table in, host table out at every call): the reference's expression on the column as ONE contiguous array
        # (threaded gather; numpy's comparison on the 248-byte-stride view took 45 ms at 10M splats)
        mask = self._column('opacity') >= logit_thresh
        original_len = len(self.data)
        self.data = _lib.host_compact_rows(self.data, mask)
        status_print(f"Alpha Filter (min {limit}): Retained {len(self.data)} out of {original_len} splats.")
        return self.data

    def crop_by_bbox(self, min_x, min_y, min_z, max_x, max_y, max_z):
        """reference :215-231"""
        self._flush_rgb()
        if self.lazy and isinstance(self._data, np.ndarray) and len(self) > 0 and self._xyz_is_f32():
            left = self._chain_for(self._data).bbox_keep((min_x, min_y, min_z, max_x, max_y, max_z))
            debug_print(f"[DEBUG] Number of vertices after cropping: {left}")
            status_print(f"After cropping, retained {left} vertices.")
            return None
        d = self.data
        # eager: the reference's expression (:218-223) on contiguous copies of the three columns (one threaded gather) -- numpy's six
        # comparisons on 248-byte-stride views took 283 ms at 10M splats
        x, y, z = self._columns(("x", "y", "z"))
        mask = ((x >= min_x) & (x <= max_x) & (y >= min_y) & (y <= max_y) &
                (z >= min_z) & (z <= max_z))
        self.data = _lib.host_compact_rows(d, mask)
        debug_print(f"[DEBUG] Number of vertices after cropping: {len(self.data)}")
        status_print(f"After cropping, retained {len(self.data)} vertices.")
        return self.data

    # ------------------------------------------------------------------ scene transform (no counterpart in the reference)
    def apply_transform(self, rotation=None, translation=None, scale=None):
        """The similarity transform p' = scale * rotation @ p + translation of the whole table (csrc/transform.hip): positions,
        log-scales, orientation quaternions, normals and every SH band above DC move with the scene.  rotation: a proper 3x3
        rotation matrix (transform.rotation_from_euler_deg makes one), scale > 0; None: identity.  Every refusal
        (transform.plan_transform) is raised before any device work; identity arguments return at once.  Pending filters are
        materialised first.  Lazy with resident rows: they are transformed in HBM in place, and ``.data`` owes one download;
        otherwise the host table goes through the device into a new table (the caller's array is left alone)."""
        debug_print("[DEBUG] Executing 'apply_transform' function...")
        self._flush_rgb()
        if not isinstance(self._data, np.ndarray) or self._data.dtype.fields is None:
            raise TypeError("self.data must be a numpy structured array.")
        plan = _transform.plan_transform(self._data.dtype, rotation, scale, translation)
        if plan.identity:
            return None if self.lazy else self.data
        if self._chain is not None:
            self._materialize()
        n = len(self._data)
        if n:
            if self.lazy and self._rr is not None:
                self._rr.transform(plan, stage_ms=self.resident_ms)
                self._host_stale = True
            elif self.lazy:
                self._data = _lib.rows_transform_table(self._data, plan, stage_ms=self.resident_ms)   # (deferred fills stay deferred)
            else:
                self.data = _lib.rows_transform_table(self.data, plan)
        status_print(f"Transform applied to {n} splats.")
        return None if self.lazy else self.data

    # ------------------------------------------------------------------ splat budget (no counterpart in the reference)
    def limit_splats(self, max_count, rank_by="size", **view_options):
        """Keep the `max_count` most visible splats, in input order (csrc/limit.hip).  Visibility is the .splat writer's metric,
        exp((scale_0 + scale_1) + scale_2) * (1 / (1 + exp(-opacity))) in float32 with the exp of csrc/np_exp.h; rows are ranked
        by the writer's sort key of its negative -- a NaN metric goes first, an infinite one last --, equal keys by row index.
        Refusals come before any device work: ValueError for a budget that is no integer >= 1, TypeError for a field that is
        not float32; a table without the four fields is left as it is, with a warning.  Lazy: one more step of the device
        chain (the keys from the resident rows when there are some), returns None; eager: updates and returns ``.data``.
        ``last_limit``: the metric of the last row kept, how many rows of exactly that metric were kept, and rank_by.
        rank_by="views": the rows are ranked by what they contributed to a set of rendered views instead (prune_by_views'
        scoring pass and its options views, size, elevation, up, fov, cameras, max_work_bytes: the N rows with the largest
        summed blending weight are kept, equal sums by row index; ``last_limit["threshold"]`` is then that sum in units of
        2^-24, rounded toward zero to float32)."""
        _views.check_rank_by(rank_by)
        if rank_by == "views":
            return self._view_pass(None, max_count, view_options)
        if view_options:
            raise ValueError(f"limit_splats: {', '.join(sorted(view_options))} need rank_by='views'")
        debug_print(f"[DEBUG] Executing 'limit_splats' with max={max_count}")
        self._flush_rgb()
        N = _lib.limit_count(max_count)
        if not isinstance(self._data, np.ndarray) or self._data.dtype.fields is None:
            raise TypeError("self.data must be a numpy structured array.")
        if any(nm not in self._data.dtype.names for nm in _lib.LIMIT_FIELDS):
            status_print("Warning: Splat limit needs scale_0..2 and opacity. Limit skipped.")
            return None if self.lazy else self.data
        _lib.require_f4_fields(self._data, _lib.LIMIT_FIELDS, "limit_splats")
        for nm in _lib.LIMIT_FIELDS:        # (the device gather of resident rows copies words: no byte-swapped fields either)
            if self._data.dtype[nm] != np.dtype("<f4"):
                raise TypeError(f"limit_splats: field {nm!r} is {self._data.dtype[nm].str}; the keys are computed from little-endian "
                                f"float32 ('<f4') fields only")
        n = len(self)
        if N >= n:
            status_print(f"Splat Limit (max {N}): {n} splats, nothing to remove.")
            return None if self.lazy else self.data
        if self.lazy:
            columns = None
            if self._rr is None:
                if self._host_stale:
                    self._materialize()     # (the host path reads the table: the transformed rows first)
                columns = _lib.limit_columns_host(self._data)
            ch = self._chain_for(self._data)
            if self._rr is not None:
                with self._timed("limit", ch.ctx):
                    res = ch.limit_keep(N)
            else:
                res = ch.limit_keep(N, columns)
            kept = res["kept"]
        else:
            data = self.data
            res = _lib.limit_mask(_lib.limit_columns_host(data), N)
            self.data = _lib.host_compact_rows(data, res["mask"])
            kept = len(self.data)
        self.last_limit = {"threshold": res["threshold"], "ties_kept": res["ties_kept"], "rank_by": "size"}
        status_print(f"Splat Limit (max {N}): Retained {kept} out of {n} splats.")
        return None if self.lazy else self.data

    # ------------------------------------------------------------------ view-based pruning (no counterpart in the reference)
    def prune_by_views(self, min_contribution, views=_views.DEFAULT_VIEWS, size=_views.DEFAULT_SIZE, elevation=_views.DEFAULT_ELEVATION,
                       up="-y", fov=50, cameras=None, max_work_bytes=_render.DEFAULT_MAX_WORK_BYTES, max_count=None):
        """Drop what no view ever sees: the table as it stands -- the rows render_preview would render -- is rendered from
        `views` cameras on a ring about its bounding box (views.plan_views: golden-angle azimuths, equal-area elevation bands
        between the two `elevation` angles, each framed like the preview), or from the explicit `cameras`
        [(ex, ey, ez, tx, ty, tz), ...], which replace the ring (the answer for inside-out captures), and every splat whose
        largest blending weight alpha * T over all pixels of all views stays under `min_contribution` (0 < w < 1) is removed
        (csrc/render.hip's score kernel).  EVERY row that no view blends goes -- hidden ones, rows outside every
        image, and rows with non-finite geometry.  max_count: the budget of limit_splats(max_count, rank_by="views") applied to
        the survivors from the same scoring pass.
        Every refusal comes before any device work: ValueError for `views` not a whole number in 1 ... 1024, a threshold
        outside (0, 1), elevations not -90 <= lo <= hi <= 90, and render.plan_render's (TypeError for a geometry field that is
        not '<f4'); a table without x y z, scale_0..2, rot_0..3 or opacity is left as it is, with a warning.  A view that
        needs more instance workspace than `max_work_bytes` prints a warning and leaves the table exactly as it was.
        A pending survivor list and deferred fills are materialised first (in HBM when the rows are resident); the compaction
        is one more step of the device chain, and with resident rows ``.data`` owes one download.  Lazy returns None, eager
        updates and returns ``.data``.  ``last_view_scores``: views, visible (rows per view), never_seen, removed, rows."""
        return self._view_pass(_views.check_min_contribution(min_contribution), max_count,
                               dict(views=views, size=size, elevation=elevation, up=up, fov=fov, cameras=cameras, max_work_bytes=max_work_bytes))

    def _settle_in_hbm(self):
        """the pending survivor list and the deferred fills applied to the resident rows where they lie: one take into new
        resident rows, no download -- ``.data`` owes it (the state decimate leaves).  -> False when this object has no resident
        rows or they cannot be taken: the caller materialises on the host"""
        if not (self.lazy and self._rr is not None) or self._pending_rgb is not None:
            return False
        ch, zero = self._chain, self._pending_zero
        if not (self._compaction_pending() or zero):
            if ch is not None and ch.orig is not None:      # (a filter ran and removed nothing: the next chain starts from no list)
                self._chain = None
                ch.close()
            return True
        taken = ch.take(zero, None, stage_ms=self.resident_ms) if ch is not None else self._rr.take(None, self._rr.n, zero, stage_ms=self.resident_ms)
        if taken is None:
            return False
        self._chain, self._pending_zero = None, []
        if ch is not None:
            ch.close()
        self._drop_resident()
        self._rr, self._host_stale = taken, True
        return True

    def _view_pass(self, min_contribution, max_count, options):
        """prune_by_views and limit_splats(rank_by="views"): one scoring pass, then the threshold on the peaks, the budget on the
        totals, or both (DeviceChain.view_prune)"""
        debug_print(f"[DEBUG] Executing view scoring pass (min={min_contribution}, max={max_count})")
        self._flush_rgb()
        N = _lib.limit_count(max_count) if max_count is not None else None
        if not isinstance(self._data, np.ndarray) or self._data.dtype.fields is None:
            raise TypeError("self.data must be a numpy structured array.")
        what = "View Prune" if min_contribution is not None else "Splat Limit"
        unknown = set(options) - {"views", "size", "elevation", "up", "fov", "cameras", "max_work_bytes"}
        if unknown:
            raise TypeError(f"view scores: unknown option {', '.join(sorted(unknown))}")
        if any(nm not in self._data.dtype.names for nm in _render.GEOMETRY):
            # (the options are still checked: a refusal does not depend on the table)
            _views.plan_views((0, 0, 0), (0, 0, 0), **{k: v for k, v in options.items() if k != "max_work_bytes"})
            status_print(f"Warning: View scores need x y z, scale_0..2, rot_0..3 and opacity. {what} skipped.")
            return None if self.lazy else self.data
        opts = dict(options)
        budget = opts.pop("max_work_bytes", _render.DEFAULT_MAX_WORK_BYTES)
        _views.check_options(self._data.dtype, max_work_bytes=budget, **opts)
        head = _views.describe(opts.get("views", _views.DEFAULT_VIEWS), opts.get("size", _views.DEFAULT_SIZE), opts.get("cameras"))
        n = len(self)
        if n == 0:
            status_print(f"{what} ({head}): no splats.")
            return None if self.lazy else self.data
        if min_contribution is None and N >= n:     # (the budget alone, and the table meets it: no scoring pass)
            status_print(f"Splat Limit (max {N}, by {head}): {n} splats, nothing to remove.")
            return None if self.lazy else self.data
        # --- device work from here on
        temp = local = None
        try:
            if not self._settle_in_hbm():
                self._materialize()
            if self.lazy and self._rr is not None:
                rows, ch = self._rr, self._chain_for(self._data)
                prof = rows.profile()
            else:
                data = self.data
                prof = _lib.host_table_profile(data)
                temp = rows = _lib.ResidentRows.from_host(data)
                ch = self._chain_for(data) if self.lazy else _lib.DeviceChain(table=data)
                local = None if self.lazy else ch
            plans = [_views.plan_scores(self._data.dtype, cam, budget) for cam in _views.plan_views(prof["lo"], prof["hi"], **opts)]
            try:
                res = ch.view_prune(plans, rows, min_contribution, N, stage_ms=self.resident_ms)
            except _render.RenderRefused as e:
                status_print(f"Warning: {what} skipped, the table is unchanged: {e}")
                return None if self.lazy else self.data
            if local is not None:
                if local.n != local.n0:
                    self.data = _lib.host_take_rows(self._data, local.survivors())
        finally:
            if temp is not None:
                temp.close()
            if local is not None:
                local.close()
        kept = len(self)
        self.last_view_scores = {"views": res["views"], "visible": list(res["visible"]), "never_seen": res["never_seen"], "removed": n - kept,
                                 "rows": n}
        if min_contribution is not None:
            status_print(f"View Prune ({head}, min {min_contribution:g}): Retained {res['after_filter']} out of {n} splats "
                         f"({res['never_seen']} never seen).")
        if N is not None:
            lim = res["limit"]
            thr = None if lim["threshold_key"] is None else np.array([0xffffffff - lim["threshold_key"]], np.uint32).view(np.float32)[0]
            self.last_limit = {"threshold": thr, "ties_kept": lim["ties_kept"], "rank_by": "views"}
            before = res["after_filter"] if res["after_filter"] is not None else n
            if lim["threshold_key"] is None:
                status_print(f"Splat Limit (max {N}, by {head}): {before} splats, nothing to remove.")
            else:
                status_print(f"Splat Limit (max {N}, by {head}): Retained {lim['kept']} out of {before} splats.")
        return None if self.lazy else self.data

    # ------------------------------------------------------------------ voxel decimation (no counterpart in the reference)
    def decimate(self, voxel_size):
        """Replace all splats of every voxel of side `voxel_size` by the one Gaussian that has their combined visibility weight,
        mean and covariance (csrc/decimate.hip).  The cells are the density filter's; a row the merge cannot use --
        a non-finite position, a weight that is not a finite number above 0, a zero quaternion -- and a voxel's only row pass
        through as they are; rows leave in the order of their voxel's first row.  Refusals come before any device work:
        ValueError for a voxel size that is not a finite number above 0, TypeError for a needed field that is not '<f4'; a
        table without x y z, scale_0..2, rot_0..3 or opacity is left as it is, with a warning.  A voxel size too small for the
        scene's coordinates (a cell index beyond +-2^20) raises ValueError from the device's flag, and nothing changes.
        Lazy with resident rows: the chain's pending survivor list and cap_sh_degree's deferred fills are consumed by the
        kernels -- the table before the decimation is never downloaded --, ``.resident`` is the merged rows and ``.data``
        owes one download of them; otherwise the host table goes through the same device path and back.
        ``last_decimate``: groups, merged_groups, passed_through."""
        debug_print(f"[DEBUG] Executing 'decimate' with voxel size {voxel_size}")
        self._flush_rgb()
        h = _decimate.check_voxel_size(voxel_size)
        if not isinstance(self._data, np.ndarray) or self._data.dtype.fields is None:
            raise TypeError("self.data must be a numpy structured array.")
        if _decimate.missing_fields(self._data.dtype):
            status_print("Warning: Decimation needs x y z, scale_0..2, rot_0..3 and opacity. Decimation skipped.")
            return None if self.lazy else self.data
        plan = _decimate.plan_decimate(self._data.dtype, h, self._pending_zero)
        n = len(self)
        if self.lazy and self._rr is not None:
            ch, zero = self._chain, self._pending_zero
            merged = (ch.decimate(plan, zero, stage_ms=self.resident_ms) if ch is not None
                      else self._rr.decimate(plan, zero_names=zero, stage_ms=self.resident_ms))
            # (a refusal raised above: the chain, its list and the deferred fills are as they were)
            self._chain, self._pending_zero = None, []
            if ch is not None:
                ch.close()
            self._drop_resident()
            self._rr, self._host_stale = merged, True       # .data owes the one download of the merged rows
            info = merged.decimate_info
        else:
            if self.lazy:
                self._materialize()
                self._data, info = _lib.rows_decimate_table(self._data, plan, stage_ms=self.resident_ms)
            else:
                self.data, info = _lib.rows_decimate_table(self.data, plan)
        self.last_decimate = dict(info)
        status_print(f"Decimate (voxel {h:g}): Merged {n} splats into {info['groups']} ({info['merged_groups']} voxels held more than one).")
        return None if self.lazy else self.data

    # ------------------------------------------------------------------ the preview image (no counterpart in the reference)
    def render_preview(self, size=(960, 540), view=(35, 20), up="-y", fov=50, camera=None, sh_degree=None, background=(0, 0, 0),
                       max_work_bytes=_render.DEFAULT_MAX_WORK_BYTES, stage_ms=None):
        """-> the (height, width, 3) uint8 image of the table as it stands (csrc/render.hip), and ``.data`` is
        unchanged.  The camera is render.plan_camera's: framed on the table's bounding box from the azimuth and elevation `view`
        about `up`, or the explicit `camera` = (eye, target).  With resident rows the box comes from their profile and the
        image is rendered where they lie; otherwise the box is the host table's profile and the table is uploaded once.  Every
        refusal of render.plan_render comes before any device work; render.RenderRefused when the scene needs more instance
        workspace than `max_work_bytes`.  ``last_preview``: visible, instances, rows and the plan."""
        debug_print("[DEBUG] Executing 'render_preview'...")
        data, rr = self.data, self.resident
        if not isinstance(data, np.ndarray) or data.dtype.fields is None:
            raise TypeError("self.data must be a numpy structured array.")
        _render.check_size(size)
        _render.plan_render(data.dtype, _render.plan_camera((0, 0, 0), (0, 0, 0), size, view, up, fov, camera), sh_degree, background,
                            max_work_bytes)                     # (the refusals: none of them depends on the box)
        prof = rr.profile() if rr is not None else _lib.host_table_profile(data)
        cam = _render.plan_camera(prof["lo"], prof["hi"], size, view, up, fov, camera)
        plan = _render.plan_render(data.dtype, cam, sh_degree, background, max_work_bytes)
        info = {}
        if rr is not None:
            image = rr.render(plan, stage_ms=stage_ms)
            info.update(rr.render_info)
        else:
            image = _lib.render_table(data, plan, stage_ms=stage_ms, info=info)
        self.last_preview = dict(info, plan=plan)
        return image

    # ------------------------------------------------------------------ fidelity against another table (no counterpart in the reference)
    def compare_with(self, other, views=_fidelity.DEFAULT_VIEWS, size=_fidelity.DEFAULT_SIZE, elevation=_views.DEFAULT_ELEVATION, up="-y",
                     fov=50, cameras=None, lo=None, hi=None, stage_ms=None, max_work_bytes=_render.DEFAULT_MAX_WORK_BYTES):
        """-> the image-space loss of `other` (a host table or _lib.ResidentRows, left as it is) against this processor's
        table as it stands, the reference: both are rendered through views.plan_views of this table's bounding box (or of the
        box `lo` ... `hi`; explicit `cameras` replace the ring) and compared on the device (fidelity.compare_tables; DESIGN.md
        6u).  With resident rows they are rendered where they lie; otherwise the host table is uploaded once, as
        render_preview does.  ``.data`` is unchanged.  Every refusal of the options and of render.plan_render for either table
        comes before any device work; render.RenderRefused when a view needs more instance workspace than `max_work_bytes`.
        ``last_fidelity``: the result."""
        debug_print("[DEBUG] Executing 'compare_with'...")
        data, rr = self.data, self.resident
        if not isinstance(data, np.ndarray) or data.dtype.fields is None:
            raise TypeError("self.data must be a numpy structured array.")
        opts = _fidelity.check_options(views=None if cameras is not None else views, size=size, elevation=elevation, up=up, fov=fov,
                                       cameras=cameras)
        res = _fidelity.compare_tables(rr if rr is not None else data, other, views=opts["views"], size=opts["size"],
                                       elevation=opts["elevation"], up=opts["up"], fov=opts["fov"], cameras=opts["cameras"], lo=lo, hi=hi,
                                       max_work_bytes=max_work_bytes, stage_ms=stage_ms)
        self.last_fidelity = res
        return res

    # ------------------------------------------------------------------ table-shaping methods
    def cap_sh_degree(self, degree):
        """reference :276-314: zero the f_rest_* columns above `degree`.  One threaded pass over the rows (the reference
        fills up to 45 strided columns one by one); in lazy mode the fill is deferred until the host table has been
        compacted, so it only touches the rows that survive the filters (which never read those columns)."""
        if degree is None or degree >= 3:
            return None if self.lazy else self.data
        debug_print(f"[DEBUG] Capping SH degree to {degree}")
        start_idx = {0: 0, 1: 9, 2: 24}.get(degree, 45)
        if not isinstance(self._data, np.ndarray):
            raise TypeError("self.data must be a numpy structured array.")
        names = [f"f_rest_{i}" for i in range(start_idx, 45) if f"f_rest_{i}" in self._data.dtype.names]
        if self.lazy:
            self._pending_zero = sorted(set(self._pending_zero) | set(names))
            return None
        _lib.host_zero_columns(self.data, names)       # in place, like the reference (:313)
        return self.data

    @staticmethod
    def _compute_rgb_from_sh(vertices):
        """reference :316-343: (N,3) uint8 colours from the SH DC term, or None without DC columns.  The power runs on the GPU
        with a rounding certificate (csrc/chain.hip:rgb_from_sh_kernel): same bytes as numpy's float32 expression."""
        names = vertices.dtype.names
        for prefix in ("", "scalar_", "scalar_scalar_"):
            if prefix + "f_dc_0" in names:
                cols = [vertices[prefix + "f_dc_%d" % c] for c in range(3)]
                break
        else:
            return None
        _lib.require_hip()
        if any(c.dtype != np.float32 for c in cols):   # numpy would promote differently: the reference's expression as is
            f_dc = np.column_stack(cols)
            rgb = np.power(np.clip(0.5 + f_dc * 0.28209479177387814, 0.0, 1.0), 1.0 / 2.2)
            return (rgb * 255).astype(np.uint8)
        # (round 6: the three columns leave the table in ONE threaded pass and go through the device as one array -- three strided
        #  numpy copies of a 248-byte-stride column cost ~50 ms each at 10M splats)
        names3 = [prefix + "f_dc_%d" % c for c in range(3)]
        n = len(vertices)
        # (n, 3), the colours' own layout; large tables into the arena's page-locked "rgb_in" under the "rgb" lease (as _xyz_rows does)
        with _xyz_rows(vertices, names3, buf_name="rgb_in") as mat:
            return _lib.rgb_from_sh(mat.reshape(-1)).reshape(n, 3)

    def _add_rgb_resident(self):
        """add_rgb_from_sh on the rows in HBM: the colours of every row of the table as it is, computed and left on the device
        (DeviceChain.resident_rgb) for the one take of _materialize.  -> False when the host path takes the call: RGB fields
        exist, no plain f_dc_0..2 fields, or more uncertain elements than the chain's list holds"""
        names = self._data.dtype.names
        if "red" in names or any("f_dc_%d" % c not in names for c in range(3)):
            return False
        ch = self._chain_for(self._data)
        with self._timed("gather", ch.ctx):
            colors = ch.resident_rgb(["f_dc_%d" % c for c in range(3)])
        if colors is None:
            return False
        self._pending_rgb = colors
        debug_print("[DEBUG] RGB added to data.")
        return True

    def _colors_of(self, table):
        """add_rgb_from_sh's colours for the rows of `table` (reference :236-248, with its two debug lines), or None when the
        table has colours already or no SH DC term to compute them from"""
        names = table.dtype.names
        if "red" in names:
            debug_print("[DEBUG] RGB fields already exist.")
            return None
        if "f_dc_0" not in names and "scalar_f_dc_0" not in names:
            debug_print("[DEBUG] No SH DC components found, cannot compute RGB.")
            return None
        return self._compute_rgb_from_sh(table)

    def add_rgb_from_sh(self):
        """reference :233-274: append (red, green, blue) u1 fields computed from the SH DC term"""
        debug_print("[DEBUG] Executing 'add_rgb_from_sh' function...")
        self._flush_rgb()
        if self.lazy and self._rr is not None and len(self) > 0 and self._add_rgb_resident():
            return
        if self._host_stale:
            self._materialize()         # (the host path reads the table: the transformed rows first)
        if self.lazy and self._compaction_pending() and isinstance(self._data, np.ndarray) and self._chain.n > 0:
            # a compaction is pending: colours for the rows of the table as it is (per-row arithmetic: the survivors' colours are what
            # the reference computes on the filtered table), appended by the ONE pass that compacts it (_materialize)
            colors = self._colors_of(self._data)
            if colors is not None:
                self._pending_rgb = colors
                debug_print("[DEBUG] RGB added to data.")
            return
        data = self.data
        colors = self._colors_of(data)
        if colors is not None:
            self.data = _lib.host_append_u8_columns(data, RGB, colors)   # :262-274 in one threaded pass
            debug_print("[DEBUG] RGB added to data.")

    def apply_auto_bbox(self):
        """reference :345-354: prints the tight bounding box of what is left (no change to the data).  On the device chain
        the box comes from the rows in HBM (no materialisation) unless it has a zero extreme."""
        debug_print("[DEBUG] Auto-Correction of Bounding Box (Calculating tight fit)...")
        if len(self) == 0:
            status_print("Auto-BBox: No points remaining. Bounding box is undefined.")
            return
        if self._chain is not None and _lib.f32_inexact_field(self._data, XYZ) is None:
            lo, hi = self._chain.bbox()     # (numpy's values, `nan` on an axis that holds a NaN)
        else:   # (a chain over coordinates float32 does not hold -- a row filter's -- is materialised: the reduction runs on the table)
            # the reference's reductions (:348-349) on contiguous copies of the columns (one threaded gather; six numpy reductions
            # over 248-byte-stride views took 92 ms at 10M splats)
            cols = self._columns(XYZ)
            lo = [np.min(c) for c in cols]
            hi = [np.max(c) for c in cols]
        # a zero extreme prints as 0.0000 or -0.0000: which zero numpy returns depends on the layout it reduces (a contiguous copy
        # and the reference's strided field view can differ) and the device box's zero has no defined sign -- so that one value
        # is the reference's own expression on the strided view
        for a, nm in enumerate(XYZ):
            if lo[a] == 0:
                lo[a] = np.min(self.data[nm])
            if hi[a] == 0:
                hi[a] = np.max(self.data[nm])
        status_print(f"Auto-BBox Applied: [{lo[0]:.4f}, {lo[1]:.4f}, {lo[2]:.4f}] to [{hi[0]:.4f}, {hi[1]:.4f}, {hi[2]:.4f}]")

    # ------------------------------------------------------------------ names a newer reference might add
    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        try:
            _Ref = _reference_class()
        except Exception as e:  # pragma: no cover - depends on the environment
            raise AttributeError(
                f"DataProcessor.{name} is not part of the v0.8 interface this drop-in implements and the reference package "
                f"(gsconverter) is not importable to forward it to: {e}") from e
        ref_attr = getattr(_Ref, name)
        if not callable(ref_attr):
            return ref_attr

        def forward(*args, **kwargs):
            ref = _Ref(self.data)
            try:
                return getattr(ref, name)(*args, **kwargs)
            finally:
                self.data = ref.data
        return forward


class ChainedDataProcessor(DataProcessor):
    """what ``install()`` binds to ``gsconverter.converter.DataProcessor``: the orchestrator ignores the filters' return
    values (converter.py:196-236) and reads ``processor.data`` once at the end (:259), so the device-resident chain applies"""

    def __init__(self, data, resident=None):
        super().__init__(data, lazy=True, resident=resident)
