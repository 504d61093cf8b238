"""``write_ply_3dgs`` / ``write_ply_cc`` -- the reference's ``Ply3DGSFormat.write`` (formats/ply_3dgs.py:62-121) and
``PlyCCFormat.write`` (formats/ply_cc.py:64-132) with their copy loop on the MI355X, and no plyfile.

  | step (ply_3dgs.py / ply_cc.py)                      | here                                                              |
  |-----------------------------------------------------|-------------------------------------------------------------------|
  | :65-66 / :67-68 has_rgb, std_order                  | plan_write(): `'red' in names` alone                              |
  | :69-78 / :69-77 crop_sh: `np.any(f_rest_i != 0)`    | one pass over the resident rows for every present f_rest_* at     |
  |        from i = 44 down                             | once (gsx_ply_rest_nonzero_dev); numpy where a field is not <f4   |
  | :80-103 / :79-111 the output dtype                  | plan_write(): names, order, types, padded and dropped fields      |
  | :104-109 / :112-116 np.zeros, the column copies     | plan_write(): fields merged into runs; gsx_ply_pack_dev           |
  |                                                     | (csrc/ply_write.hip): one launch, whole rows                      |
  | :111-120 / :118-131 plyfile's container             | ply_container.header() and the rows, then the extra elements      |

The file is the reference's byte for byte ("3DGS / CloudCompare PLY writer").  What the device path does not take
is refused with a reason (WritePlan.refusal): a field that has to be written and is none of the eight PLY scalar types, a
big-endian field, rows wider than 512 bytes in the table or in the file, more than 128 runs.  A refused table goes to
`fallback` (the reference's own write, when plyfile is there), else UnsupportedPlyError.
"""
from __future__ import annotations

import time

import numpy as np

from .. import _lib
from ..utils import debug_print, status_print
from .compressed_ply_reader import UnsupportedPlyError, plyfile_available  # noqa: F401
from .ply_container import PLY_TYPE_NAMES, header, little_endian
from .ply_reader import COLOURS, DIALECTS, N_REST, get_standard_order

MAX_STRIDE = _lib.PLY_WRITE_MAX_STRIDE
MAX_RUNS = _lib.PLY_WRITE_MAX_RUNS
NORMALS = ("nx", "ny", "nz")
CC_PLAIN = {"x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"}               # ply_cc.py:86: no scalar_ in front


def rest_index(name: str) -> int:
    """i of a standard f_rest_i, else -1"""
    if name.startswith("f_rest_") and name[7:].isdigit() and str(int(name[7:])) == name[7:] and int(name[7:]) < N_REST:
        return int(name[7:])
    return -1


class WriteField:
    """one field of the file's vertex element: its name there, its type, where it comes from (source None: zeros)"""
    __slots__ = ("name", "type", "source", "src_offset", "dst_offset", "nbytes")

    def __init__(self, name, typ, source, src_offset, dst_offset, nbytes):
        self.name, self.type, self.source, self.src_offset, self.dst_offset, self.nbytes = name, typ, source, src_offset, dst_offset, nbytes

    def entry(self):
        """(source byte offset or None, destination byte offset, bytes)"""
        return self.src_offset, self.dst_offset, self.nbytes


class WritePlan:
    """what a writer does with a table, from its dtype alone (and last_idx under crop_sh): the file's dtype and property list,
    one WriteField per output field, the fields merged into runs; `refusal` says why the device path does not take the table"""

    def __init__(self):
        self.dialect = self.dtype = self.properties = self.fields = self.runs = self.refusal = self.last_idx = None
        self.has_rgb = self.crop_sh = self.identity = False
        self.in_stride = self.out_stride = 0

    def entries(self):
        return [f.entry() for f in self.fields]

    def layout(self) -> "_lib.PlyWriteLayout":
        lay = _lib.PlyWriteLayout()
        lay.in_stride, lay.out_stride, lay.n_runs = self.in_stride, self.out_stride, len(self.runs)
        for k, (so, do, nb) in enumerate(self.runs):
            lay.src_offset[k], lay.dst_offset[k], lay.bytes[k] = -1 if so is None else so, do, nb
        return lay


def merge_runs(entries) -> list:
    """[(source offset or None, destination offset, bytes)] in file order -> the same with neighbours merged where both are
    zero fill, or the second follows the first in the table as it does in the file"""
    runs = []
    for so, do, nb in entries:
        if runs:
            ps, pd, pn = runs[-1]
            if pd + pn == do and ((so is None and ps is None) or (so is not None and ps is not None and ps + pn == so)):
                runs[-1] = (ps, pd, pn + nb)
                continue
        runs.append((so, do, nb))
    return runs


def plan_write(dtype: np.dtype, dialect: str, crop_sh: bool = False, last_idx: "int | None" = None) -> WritePlan:
    """ply_3dgs.py:65-103 (dialect "3dgs") or ply_cc.py:67-111 ("cc") on a table's dtype -> WritePlan.  Touches no device.

    :65 / :67 has_rgb is `'red' in names` alone; :66 / :68 std_order holds nx ny nz; :70-78 / :70-77 under crop_sh every f_rest_j
    with j > last_idx (the highest present f_rest index holding a value != 0, -1 for none: the caller's scan) leaves std_order,
    a cut by index; :84-94 / :88-100 a standard name present is written with the table's own type, an absent f_rest_* is a zero
    f4 column unless crop_sh, absent nx ny nz always are, every other absent name is left out; :98-101 / :104-109 the extras
    are the table's fields in neither std_order nor get_standard_order(True), in table order; ply_cc.py:90, :97, :107 every output
    name outside CC_PLAIN gets scalar_ in front."""
    if dialect not in DIALECTS:
        raise ValueError("plan_write: dialect %r (one of %s)" % (dialect, ", ".join(DIALECTS)))
    dtype = np.dtype(dtype)
    if dtype.names is None:
        raise ValueError("plan_write: a structured dtype is needed")
    crop_sh = bool(crop_sh)
    if crop_sh and last_idx is None:
        raise ValueError("plan_write: crop_sh needs last_idx")
    p = WritePlan()
    p.dialect, p.crop_sh, p.last_idx, p.in_stride = dialect, crop_sh, (int(last_idx) if crop_sh else None), dtype.itemsize
    names = dtype.names
    p.has_rgb = "red" in names
    std_order = get_standard_order(p.has_rgb)
    if crop_sh:
        std_order = [n for n in std_order if not rest_index(n) > p.last_idx]
    prefix = (lambda n: n if n in CC_PLAIN else "scalar_" + n) if dialect == "cc" else (lambda n: n)
    listed = []                                                                     # (output name, source name or None)
    for n in std_order:
        if n in names:
            listed.append((prefix(n), n))
        elif (rest_index(n) >= 0 and not crop_sh) or n in NORMALS:
            listed.append((prefix(n), None))
    full_std = set(get_standard_order(True))
    in_std = set(std_order)
    for n in names:
        if n not in in_std and n not in full_std:
            listed.append(("scalar_" + n if dialect == "cc" else n, n))
    # what has to be written: PLY scalars, little-endian
    types = []
    for out_name, src in listed:
        if src is None:
            types.append("<f4")
            continue
        ft = dtype[src]
        if ft.str[1:] not in PLY_TYPE_NAMES or ft.kind not in "iuf" or ft.shape:
            if p.refusal is None:
                p.refusal = "field %r is %s (a PLY property is one of %s)" % (src, ft, ", ".join(PLY_TYPE_NAMES))
            types.append(None)
            continue
        if ft.str[0] == ">" and p.refusal is None:
            p.refusal = "field %r is big-endian (%s)" % (src, ft.str)
        types.append("<" + ft.str[1:] if ft.itemsize > 1 else ft.str)
    if any(t is None for t in types):
        return p
    p.dtype = np.dtype([(o, t) for (o, _), t in zip(listed, types)])                # (np.dtype raises for a repeated name, as :103 / :111)
    p.properties = [(PLY_TYPE_NAMES[p.dtype[o].str[1:]], o) for o in p.dtype.names]
    p.out_stride = p.dtype.itemsize
    p.fields = [WriteField(o, t, src, None if src is None else dtype.fields[src][1], p.dtype.fields[o][1], p.dtype[o].itemsize)
                for (o, src), t in zip(listed, types)]
    p.runs = merge_runs(p.entries())
    if p.refusal is None:
        if p.in_stride > MAX_STRIDE or p.out_stride > MAX_STRIDE:
            p.refusal = "rows of %d bytes in the table and %d in the file (the device path takes up to %d)" % (p.in_stride, p.out_stride, MAX_STRIDE)
        elif len(p.runs) > MAX_RUNS:
            p.refusal = "%d runs a row (the device path takes up to %d)" % (len(p.runs), MAX_RUNS)
    # the table's rows are the file's rows already: one run over the whole row (same order, no holes, nothing padded or dropped)
    p.identity = p.refusal is None and p.runs == [(0, 0, p.in_stride)] and p.in_stride == p.out_stride
    return p


def rest_fields(dtype: np.dtype):
    """-> (offsets[45], present mask, every present f_rest_* is little-endian float32)"""
    offsets, present, f4 = [0] * N_REST, 0, True
    for n in dtype.names:
        i = rest_index(n)
        if i >= 0:
            offsets[i], present = dtype.fields[n][1], present | (1 << i)
            f4 = f4 and _lib.is_f4(dtype[n])
    return offsets, present, f4


def last_nonzero_rest(data: np.ndarray) -> int:
    """ply_3dgs.py:71-76 / ply_cc.py:71-76 as they stand, with numpy"""
    with np.errstate(all="ignore"):
        for i in range(N_REST - 1, -1, -1):
            f = "f_rest_%d" % i
            if f in data.dtype.names and np.any(data[f] != 0):
                return i
    return -1


def _clock(stage_ms, name, t0):
    if stage_ms is not None:
        stage_ms[name] = round(stage_ms.get(name, 0.0) + (time.perf_counter() - t0) * 1e3, 3)


def _write(data, path, dialect, stage_ms, device, fallback, kwargs):
    crop_sh = bool(kwargs.get("crop_sh", False))
    extra_elements = kwargs.get("extra_elements", []) or []
    if not isinstance(data, np.ndarray) or data.dtype.names is None or data.ndim != 1:
        raise ValueError("write_ply_%s: a 1-D structured table is needed" % dialect)
    n = len(data)

    def refuse(why):
        if fallback is None:
            raise UnsupportedPlyError("%s: %s -- the GPU PLY writer takes tables of little-endian PLY scalars with rows of up to %d "
                                      "bytes; this one needs the reference's writer (plyfile)" % (path, why, MAX_STRIDE))
        debug_print(f"[DEBUG] PLY: {why}; the reference's writer takes it")
        return fallback()

    t0 = time.perf_counter()
    offsets, present, rest_f4 = rest_fields(data.dtype)
    scan_on_device = crop_sh and present and n > 0 and rest_f4 and data.dtype.itemsize <= MAX_STRIDE
    plan = rows = None
    if not scan_on_device:
        last_idx = None
        if crop_sh:
            last_idx = last_nonzero_rest(data) if present and n > 0 else -1
            _clock(stage_ms, "sh_detect", t0)
            t0 = time.perf_counter()
        plan = plan_write(data.dtype, dialect, crop_sh, last_idx)
        _clock(stage_ms, "plan", t0)
        if plan.refusal is not None:
            return refuse(plan.refusal)
    if n > 0 and (plan is None or not plan.identity):
        table = np.ascontiguousarray(data)                                          # a non-contiguous view is made contiguous first
        plan, rows = _lib.ply_pack_table(table, (lambda last: plan_write(data.dtype, dialect, crop_sh, last)) if plan is None else (lambda last: plan),
                                         scan=(offsets, present) if scan_on_device else None, stage_ms=stage_ms, device=device)
        if plan.refusal is not None:
            return refuse(plan.refusal)
    if crop_sh:
        debug_print(f"[DEBUG] crop_sh=True. Detected last active SH index: {plan.last_idx}")
    if n > 0 and rows is None:                                                      # identity: the caller's rows are the file's
        rows = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    t0 = time.perf_counter()
    elements = [("vertex", n, plan.properties)]
    bodies = []
    for e in extra_elements:
        arr = little_endian(np.asarray(e.data))
        elements.append((e.name, len(arr), [(PLY_TYPE_NAMES[arr.dtype[f].str[1:]], f) for f in arr.dtype.names]))
        bodies.append(arr)
    with open(path, "wb") as f:
        f.write(header(elements))
        if n > 0:
            f.write(memoryview(rows))
        for arr in bodies:
            f.write(arr.tobytes())
    _clock(stage_ms, "file_write", t0)
    return plan


def _reference_write(dialect):
    """the reference's own write as a fallback, when plyfile and the reference are really there"""
    if not plyfile_available():
        return None
    try:
        if dialect == "3dgs":
            from gsconverter.formats.ply_3dgs import Ply3DGSFormat as cls  # type: ignore
        else:
            from gsconverter.formats.ply_cc import PlyCCFormat as cls  # type: ignore
    except ImportError:
        return None
    write = getattr(cls.write, "__wrapped__", cls.write)
    return lambda data, path, **kw: write(cls(), data, path, **kw)


def write_ply_3dgs(data: np.ndarray, path: str, stage_ms: "dict | None" = None, device: int = 0, fallback=None, **kwargs):
    """ply_3dgs.py:62-121: `data` (a 1-D structured table) -> a binary little-endian PLY at `path`, the reference's file byte
    for byte.  kwargs: the reference's `crop_sh` and `extra_elements` (objects with .name and .data, plyfile's or
    PlyExtraElement; a big-endian array is byte-swapped on the way out).  -> the WritePlan that was carried out.

    fallback: a function () -> None that writes the file the reference's way, for the tables the device path does not take
    (WritePlan.refusal); without one the reference's own write is used when plyfile and the reference are there, else such
    tables raise UnsupportedPlyError.  stage_ms: a dict that receives the stage clocks plan, upload, sh_detect, pack, download,
    file_write (tools/probe_ply_write.py); a table whose rows are the file's already (WritePlan.identity) is written as it is
    and has no upload, pack or download -- unless crop_sh asks for the scan of its resident rows first.  n = 0 writes the header
    and the extra elements only."""
    debug_print(f"[DEBUG] Writing 3DGS PLY file to {path}")
    if fallback is None:
        ref = _reference_write("3dgs")
        fallback = None if ref is None else (lambda: ref(data, path, **kwargs))
    plan = _write(data, path, "3dgs", stage_ms, device, fallback, kwargs)
    if isinstance(plan, WritePlan):
        if kwargs.get("extra_elements"):
            status_print(f"Maintained {len(kwargs['extra_elements'])} extra PLY elements.")         # :118
        status_print(f"3DGS PLY write completed. {len(data)} points.")                              # :121
    return plan


def write_ply_cc(data: np.ndarray, path: str, stage_ms: "dict | None" = None, device: int = 0, fallback=None, **kwargs):
    """ply_cc.py:64-132 -> a binary little-endian PLY at `path`; see write_ply_3dgs"""
    debug_print(f"[DEBUG] Writing CC PLY file to {path}")
    if fallback is None:
        ref = _reference_write("cc")
        fallback = None if ref is None else (lambda: ref(data, path, **kwargs))
    plan = _write(data, path, "cc", stage_ms, device, fallback, kwargs)
    if isinstance(plan, WritePlan):
        if kwargs.get("extra_elements"):
            print(f"Maintained {len(kwargs['extra_elements'])} extra PLY elements.")                # :129 plain print
        debug_print(f"CloudCompare PLY write completed. {len(data)} points.")                       # :132
    return plan


def _bind(original, writer):
    def write(self, data, path, **kwargs):
        fallback = (lambda: original(self, data, path, **kwargs)) if plyfile_available() else None
        writer(data, path, fallback=fallback, **kwargs)
    write.__wrapped__ = original
    return write


def bind_write_3dgs(original):
    """-> a replacement for ``Ply3DGSFormat.write`` that packs the rows on the device and writes the container itself; tables
    the device path does not take go to `original` (the reference's write) when plyfile is there"""
    return _bind(original, write_ply_3dgs)


def bind_write_cc(original):
    """-> a replacement for ``PlyCCFormat.write``; see bind_write_3dgs"""
    return _bind(original, write_ply_cc)
