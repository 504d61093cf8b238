"""``read_ply_3dgs`` / ``read_ply_cc`` -- the reference's ``Ply3DGSFormat.read`` (formats/ply_3dgs.py:8-60) and
``PlyCCFormat.read`` (formats/ply_cc.py:8-62) with their mapping loop on the MI355X, and no plyfile.

  | step (ply_3dgs.py / ply_cc.py)                     | here                                                               |
  |----------------------------------------------------|--------------------------------------------------------------------|
  | :10 PlyData.read                                   | compressed_ply_reader.parse_header; the vertex body is read        |
  |                                                    | straight into page-locked staging, the other elements on the host  |
  | :10 PlyData.read of a `format ascii` file          | ascii_body=True: the vertex lines are tokenised and parsed on the  |
  |                                                    | device (csrc/ply_text.hip) into the binary rows plyfile would hand |
  |                                                    | on, the other elements on the host under the same token rules      |
  | :12-13 no `vertex` element: ValueError             | the same message, before anything else                             |
  | :16 self.extra_elements                            | read_extra_elements(): objects with .name, .data (bind_read_*: real |
  |                                                    | plyfile elements when plyfile is there)                            |
  | :21-28 / :21-26 source prefix                      | source_prefix()                                                    |
  | :30-40 / :28-40 extra fields                       | plan(): the 3DGS reader keeps the name, the CC reader strips       |
  |                                                    | `scalar_`; the source's type is kept                               |
  | :43-45 has_rgb, define_dtype, np.zeros             | plan(): define_dtype(), packed and little-endian                   |
  | :48-58 / :48-60 `converted_data[t] = vertices[s]`  | plan(): one descriptor per output field; gsx_ply_unpack_dev        |
  |                                                    | (csrc/ply_read.hip): one launch, whole rows                        |

The rows are the reference's bit for bit ("3DGS / CloudCompare PLY reader").  What the device path does not take is
refused with a reason (Plan.refusal): an ascii body without ascii_body=True (with it: one whose lines or numbers break the rules
of DESIGN.md "ASCII PLY bodies", named with element and line), list properties, a duplicated vertex property, red / green / blue of
another type than uchar, an extra field whose source has another type, a big-endian file with extra fields, rows wider than
512 bytes, more than 128 output fields.  A refused file goes to `fallback` (the reference's own read, when plyfile is there),
else UnsupportedPlyError.

The one known deviation: a body that ends early raises _lib.read_exact's ValueError, as the other readers do -- plyfile raises
its own PlyElementParseError, a class that cannot be matched without plyfile.  (A header this parser does not understand raises
PlyHeaderError, a ValueError, where plyfile raises PlyHeaderParseError.)
"""
from __future__ import annotations

import time

import numpy as np

from .. import _lib
from ..utils import debug_print
from .compressed_ply_reader import PLY_TYPES, PlyHeader, PlyHeaderError, UnsupportedPlyError, parse_header, plyfile_available  # noqa: F401

DIALECTS = ("3dgs", "cc")
MAX_STRIDE = _lib.PLY_READ_MAX_STRIDE
MAX_FIELDS = _lib.PLY_READ_MAX_FIELDS
N_REST = 45                                                                         # structures.py:36 at sh_degree=3
COLOURS = ["red", "green", "blue"]


def get_standard_order(has_rgb: bool = False) -> list:
    """GaussianStruct.get_standard_order (structures.py:6-20)"""
    order = (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + ["f_rest_%d" % i for i in range(N_REST)]
             + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"])
    return order + COLOURS if has_rgb else order


def define_dtype(has_rgb: bool, extra_fields) -> list:
    """GaussianStruct.define_dtype(has_scal=False, has_rgb=has_rgb, extra_fields=extra_fields) (structures.py:23-59) at
    sh_degree=3 -> [(name, type)]: an extra field whose name is there already is dropped (:56)"""
    dtype = [(f, "f4") for f in get_standard_order(False)]
    if has_rgb:
        dtype += [(f, "u1") for f in COLOURS]
    for name, typ in extra_fields or ():
        if not any(d[0] == name for d in dtype):
            dtype.append((name, typ))
    return dtype


def source_prefix(source_names, dialect: str) -> str:
    """ply_3dgs.py:21-28 / ply_cc.py:21-26"""
    if dialect == "3dgs":
        if "scalar_f_dc_0" in source_names:
            return "scalar_scal_" if "scalar_scal_f_dc_0" in source_names else "scalar_"
        return "scal_" if "scal_f_dc_0" in source_names else ""
    if "scalar_f_dc_0" in source_names:
        return "scalar_"
    return "scalar_scal_" if "scalar_scal_f_dc_0" in source_names else ""


class Field:
    """one output field: where it comes from (source None: it stays zero) and where it goes"""
    __slots__ = ("name", "type", "dst_offset", "dst_bytes", "source", "src_type", "src_offset", "raw")

    def __init__(self, name, typ, dst_offset):
        self.name, self.type, self.dst_offset, self.dst_bytes = name, typ, dst_offset, np.dtype(typ).itemsize
        self.source = self.src_type = None
        self.src_offset = -1
        self.raw = typ != "f4"                # red green blue and the extras: byte copies

    def descriptor(self):
        """(src byte offset or -1, src type code, dst byte offset, dst bytes)"""
        code = _lib.PLY_T_RAW if self.raw else _lib.PLY_TYPE_CODES[self.src_type or "f4"]
        return self.src_offset, code, self.dst_offset, self.dst_bytes


class Plan:
    """what a reader does with a file, from its header alone: the output dtype and one Field per output field; `refusal` says
    why the device path does not take the file (then `fields` may be None)"""

    def __init__(self):
        self.dialect = self.prefix = self.dtype = self.fields = self.refusal = None
        self.has_rgb = self.big_endian = self.ascii = False
        self.extra_fields = []
        self.count = self.in_stride = self.out_stride = 0
        self.body_offset = None

    @property
    def identity(self) -> bool:
        """the file's rows ARE the output rows: little-endian, equal strides, every field a bit copy from its own offset"""
        return (self.refusal is None and not self.big_endian and not self.ascii and self.in_stride == self.out_stride
                and all(f.source is not None and f.src_offset == f.dst_offset and (f.raw or f.src_type == "f4") for f in self.fields))

    def descriptors(self):
        return [f.descriptor() for f in self.fields]

    def layout(self) -> "_lib.PlyReadLayout":
        lay = _lib.PlyReadLayout()
        lay.in_stride, lay.out_stride, lay.n_fields, lay.big_endian = self.in_stride, self.out_stride, len(self.fields), int(self.big_endian)
        for i, (so, code, do, nb) in enumerate(self.descriptors()):
            lay.src_offset[i], lay.src_type[i], lay.dst_offset[i], lay.dst_bytes[i] = so, code, do, nb
        return lay


def plan(header: PlyHeader, dialect: str, ascii_body: bool = False) -> Plan:
    """ply_3dgs.py:12-58 (dialect "3dgs") or ply_cc.py:12-60 ("cc") on a parsed header -> Plan.  Touches no device.
    ascii_body: an ascii body is no refusal (Plan.ascii is set: the rows come from the text, body_offset is not known from the
    header); every other refusal stays.

    :12-13 a missing `vertex` raises the reference's ValueError; :21-28 / :21-26 the source prefix; :30-40 / :28-40 the extra
    fields (source names outside {prefix + std} | {std}, std = get_standard_order(has_rgb=True), which holds nx ny nz already --
    ply_cc.py:30 appends them once more, to a set); :43 has_rgb is `'red' in source_names` alone; :44 define_dtype; :48-58 /
    :48-60 per output field the direct name, else prefix + name, else (CC only, :59-60) scalar_ + name, else it stays zero."""
    if dialect not in DIALECTS:
        raise ValueError("plan: dialect %r (one of %s)" % (dialect, ", ".join(DIALECTS)))
    vertex = header.element("vertex")
    if vertex is None:
        raise ValueError("PLY file does not contain 'vertex' element")
    p = Plan()
    p.dialect, p.count, p.big_endian = dialect, vertex.count, header.format == "binary_big_endian"
    # what no reading of the header can be planned for
    p.ascii = header.format == "ascii"
    if p.ascii and not ascii_body:
        p.refusal = "an ascii body"
    for e in header.elements:
        if p.refusal is None and e.has_list():
            p.refusal = "list property %r of element %r" % (next(n for n, t in e.props if isinstance(t, tuple)), e.name)
    source_names = vertex.names()
    if p.refusal is None and len(set(source_names)) != len(source_names):
        p.refusal = "property %r appears twice in element 'vertex'" % next(n for i, n in enumerate(source_names) if n in source_names[:i])
    if vertex.has_list() or len(set(source_names)) != len(source_names):
        return p
    src_type = dict(vertex.props)
    src_offset, off = {}, 0
    for n, t in vertex.props:
        src_offset[n] = off
        off += np.dtype(t).itemsize
    p.in_stride, p.body_offset = off, vertex.body_offset
    p.prefix = source_prefix(source_names, dialect)
    std = get_standard_order(has_rgb=True)
    std_source_names = {p.prefix + n for n in std} | set(std)
    for n in source_names:
        if n not in std_source_names:
            internal = n[7:] if dialect == "cc" and n.startswith("scalar_") else n
            p.extra_fields.append((internal, src_type[n]))
    p.has_rgb = "red" in source_names
    listed = define_dtype(p.has_rgb, p.extra_fields)
    p.dtype = np.dtype([(n, "<" + t if np.dtype(t).itemsize > 1 else t) for n, t in listed])
    p.fields, p.out_stride = [], p.dtype.itemsize
    for n, t in listed:
        f = Field(n, t, p.dtype.fields[n][1])
        for cand in (n, p.prefix + n) + (("scalar_" + n,) if dialect == "cc" else ()):
            if cand in src_type:
                f.source, f.src_type, f.src_offset = cand, src_type[cand], src_offset[cand]
                break
        p.fields.append(f)
    if p.refusal is not None:
        return p
    n_std = len(get_standard_order(p.has_rgb))
    for f in p.fields:
        if f.source is not None and f.raw and f.src_type != f.type:
            if f.name in COLOURS:
                p.refusal = "property %r is %s (the device path reads uchar colours: numpy's cast to uint8 is platform-defined)" % (f.source, f.src_type)
            else:
                p.refusal = "extra field %r is %s in the rows and %s in property %r" % (f.name, f.type, f.src_type, f.source)
            return p
    if p.big_endian and len(p.fields) > n_std:
        p.refusal = "a big-endian body with extra fields (%s)" % ", ".join(f.name for f in p.fields[n_std:])
    elif p.in_stride > MAX_STRIDE or p.out_stride > MAX_STRIDE:
        p.refusal = "rows of %d bytes in the file and %d in the table (the device path takes up to %d)" % (p.in_stride, p.out_stride, MAX_STRIDE)
    elif len(p.fields) > MAX_FIELDS:
        p.refusal = "%d output fields (the device path takes up to %d)" % (len(p.fields), MAX_FIELDS)
    return p


class PlyExtraElement:
    """a non-vertex element as the readers hand it on: what the reference's writers use of a plyfile element"""

    def __init__(self, name: str, data: np.ndarray):
        self.name, self.data = name, data

    def __repr__(self):
        return "PlyExtraElement(%r, %d rows)" % (self.name, len(self.data))


def read_extra_elements(path: str, header: PlyHeader) -> list:
    """:16 every element but `vertex`, read on the host into a structured array in the file's byte order (binary bodies of
    scalar properties)"""
    order = ">" if header.format == "binary_big_endian" else "<"
    out = []
    with open(path, "rb") as f:
        for e in header.elements:
            if e.name == "vertex":
                continue
            dt = np.dtype([(n, order + t if np.dtype(t).itemsize > 1 else t) for n, t in e.props])
            data = np.empty(e.count, dt)
            if data.nbytes:
                f.seek(e.body_offset)
                _lib.read_exact(f, data.view(np.uint8).reshape(-1), path, " in element %r" % e.name)
            out.append(PlyExtraElement(e.name, data))
    return out


def _refused(path: str, reason: str, fallback):
    if fallback is None:
        raise UnsupportedPlyError("%s: %s -- the GPU PLY reader takes binary files, and with ascii_body=True ascii files, of scalar "
                                  "properties with rows of up to %d bytes; this one needs the reference's reader (plyfile)" % (path, reason, MAX_STRIDE))
    debug_print(f"[DEBUG] PLY: {reason}; the reference's reader takes it")
    return fallback(path)


def _read_ascii(path: str, h: PlyHeader, p: Plan, t0, stage_ms, device, profile, keep, stats, chunk_bytes):
    """the elements of an ascii file in the file's order: `vertex` through _lib.ply_text_table, the others on the host under the
    same token rules (_lib.ply_text_host); each element starts where the one before it ended -> (rows, extras)"""
    vertex = h.element("vertex")
    pos, extras, rows = h.header_bytes, [], None
    for e in h.elements:
        st = {}
        if e is not vertex:
            data = _lib.ply_text_host(path, pos, e.count, e.props, stats=st, element=e.name)
            extras.append(PlyExtraElement(e.name, data))
            pos = st["end_offset"]
            continue
        if stage_ms is not None:
            stage_ms["parse"] = round((time.perf_counter() - t0) * 1e3, 3)
        if p.count == 0:                                                            # :45 np.zeros(0, dtype): no launch
            rows = np.zeros(0, p.dtype)
            st = {"tokens": 0, "host_tokens": 0, "chunks": 0, "end_offset": pos}
        else:
            rows = _lib.ply_text_table(path, pos, p.count, vertex.props, p.layout(), p.dtype, stage_ms=stage_ms, device=device, stats=st,
                                       chunk_bytes=chunk_bytes, **_lib.profile_kw(profile), **_lib.keep_kw(keep))
        pos = st["end_offset"]
        if stats is not None:
            stats.update(st)
    return rows, extras


def _read(path: str, dialect: str, stage_ms, fallback, device, profile=None, keep=None, ascii_body=False, stats=None, chunk_bytes=None):
    t0 = time.perf_counter()
    h = parse_header(path)
    p = plan(h, dialect, ascii_body)
    if p.refusal is not None:
        return _refused(path, p.refusal, fallback)
    if p.ascii:
        try:
            rows, extras = _read_ascii(path, h, p, t0, stage_ms, device, profile, keep, stats, chunk_bytes)
        except _lib.PlyTextError as e:
            return _refused(path, "an ascii body that plyfile's two generations read differently or not at all: %s" % e, fallback)
        debug_print(f"[DEBUG] Loaded {p.count} points from ascii PLY ({dialect})")
        return rows, extras
    extras = read_extra_elements(path, h)
    if stage_ms is not None:
        stage_ms["parse"] = round((time.perf_counter() - t0) * 1e3, 3)
    if p.count == 0:                                                                # :45 np.zeros(0, dtype)
        return np.zeros(0, p.dtype), extras
    if p.identity:                                  # the canonical trainer output: the file's rows are the table's
        t1 = time.perf_counter()
        rows = np.empty(p.count, p.dtype)
        with open(path, "rb") as f:
            f.seek(p.body_offset)
            _lib.read_exact(f, rows.view(np.uint8).reshape(-1), path, " in element 'vertex'")
        if stage_ms is not None:
            stage_ms["file_read"] = round((time.perf_counter() - t1) * 1e3, 3)
    else:
        rows = _lib.ply_unpack_table(path, p.body_offset, p.count, p.layout(), p.dtype, stage_ms=stage_ms, device=device, **_lib.profile_kw(profile), **_lib.keep_kw(keep))
    debug_print(f"[DEBUG] Loaded {p.count} points from PLY ({dialect})")
    return rows, extras


def read_ply_3dgs(path: str, stage_ms: "dict | None" = None, fallback=None, device: int = 0, profile: "dict | None" = None, keep: "dict | None" = None,
                  ascii_body: bool = False, stats: "dict | None" = None, chunk_bytes: "int | None" = None):
    """ply_3dgs.py:8-60 -> (rows, extra_elements): the reference's structured array (define_dtype(has_scal=False, has_rgb,
    extra_fields) at sh_degree=3, packed, little-endian) and the non-vertex elements.

    fallback: a function path -> (rows, extra_elements) for the files the device path does not take (Plan.refusal); without
    one such files raise UnsupportedPlyError.  stage_ms: a dict that receives the stage clocks parse, file_read, upload, kernel,
    download (tools/probe_ply_read.py); a file whose rows are the table's already (Plan.identity) is read into the result and
    has no upload, kernel or download.  A body that ends early raises _lib.read_exact's ValueError (plyfile's own exception
    class cannot be matched without plyfile).  profile: a dict that receives the returned
    table's profile (_lib.TableProfile.as_dict): from one more pass over the transcoded rows before their download (stage clock
    "profile"), or from the threaded host pass for a file that is read into the result.  keep: a dict that receives the decoded rows in HBM as keep["rows"] (_lib.ResidentRows; the caller
    closes it) when the returned table's rows are resident; it stays empty otherwise (a file that is read into the result among them).
    ascii_body: take a file of `format ascii` too (off by default: such a file is refused like the others): its vertex lines are
    parsed on the device (_lib.ply_text_table; stage clocks parse, file_read, upload, scan, kernel, patch, unpack, download), its
    other elements on the host under the same token rules; a body that breaks them ("ASCII PLY bodies") is refused
    with the element and the line.  stats: a dict that receives tokens, host_tokens (the tokens the host settled) and chunks of
    an ascii read.  chunk_bytes: the text per upload of an ascii read (default _lib.PLY_TEXT_CHUNK_BYTES)."""
    debug_print(f"[DEBUG] Reading 3DGS PLY file from {path}")
    return _lib.with_keep(keep, lambda: _lib.with_profile(profile, lambda: _read(path, "3dgs", stage_ms, fallback, device, profile, keep, ascii_body, stats, chunk_bytes)))


def read_ply_cc(path: str, stage_ms: "dict | None" = None, fallback=None, device: int = 0, profile: "dict | None" = None, keep: "dict | None" = None,
                ascii_body: bool = False, stats: "dict | None" = None, chunk_bytes: "int | None" = None):
    """ply_cc.py:8-62 -> (rows, extra_elements); see read_ply_3dgs"""
    debug_print(f"[DEBUG] Reading CC PLY file from {path}")
    return _lib.with_keep(keep, lambda: _lib.with_profile(profile, lambda: _read(path, "cc", stage_ms, fallback, device, profile, keep, ascii_body, stats, chunk_bytes)))


def _bind(original, reader):
    def read(self, path, **kwargs):
        def fallback(p):
            rows = original(self, p, **kwargs)
            return rows, getattr(self, "extra_elements", [])
        have = plyfile_available()
        rows, extras = reader(path, fallback=fallback if have else None)
        if have and any(isinstance(e, PlyExtraElement) for e in extras):
            import plyfile
            extras = [plyfile.PlyElement.describe(e.data, e.name) if isinstance(e, PlyExtraElement) else e for e in extras]
        self.extra_elements = extras
        return rows
    read.__wrapped__ = original
    return read


def bind_read_3dgs(original):
    """-> a replacement for ``Ply3DGSFormat.read`` that maps the rows on the device and sets ``self.extra_elements`` (plyfile
    elements when plyfile is there, else PlyExtraElement); files the device path does not take go to `original` (the
    reference's read) when plyfile is there"""
    return _bind(original, read_ply_3dgs)


def bind_read_cc(original):
    """-> a replacement for ``PlyCCFormat.read``; see bind_read_3dgs"""
    return _bind(original, read_ply_cc)
