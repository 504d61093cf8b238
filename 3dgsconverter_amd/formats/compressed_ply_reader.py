"""``read_compressed_ply`` -- the reference's ``CompressedPlyFormat.read`` (formats/compressed_ply.py:14-124) with its decode on the
MI355X, and no plyfile.

  | step (formats/compressed_ply.py)                  | here                                                                |
  |---------------------------------------------------|---------------------------------------------------------------------|
  | :16-17 PlyData.read                               | parse_header: the PLY header, each property's byte offset and each  |
  |                                                   | element's row stride; the bodies are read straight into staging     |
  | :20-24 no `chunk` element: Ply3DGSFormat().read   | handed to the reference's own read, untouched (as are ascii and     |
  |                                                   | big-endian bodies and list properties: refusal())                   |
  | :26-60 sh names, degree, metadata, np.zeros rows  | read_compressed_ply, before any device work                         |
  | :63-122 the per-chunk decode loop                 | gsx_cply_unpack_dev (csrc/cply_read.hip): one pass, every row       |

The rows are the reference's bit for bit, NaN bits included ("Compressed-PLY reader").  The reference's errors come
first and from the header alone: a missing `vertex` element raises KeyError, a missing property the ValueError numpy raises
(``no field of name <name>``), in the order the reference's loop reads them.
"""
from __future__ import annotations

import time

import numpy as np

from .. import _lib
from ..utils import debug_print

CHUNK_SIZE = 256   # :12

# :167-174 order (gsx_cply_read_layout.chunk_offset)
CHUNK_FIELDS = (["min_x", "min_y", "min_z", "max_x", "max_y", "max_z"] + ["min_scale_x", "min_scale_y", "min_scale_z"]
                + ["max_scale_x", "max_scale_y", "max_scale_z"] + ["min_r", "min_g", "min_b", "max_r", "max_g", "max_b"])
VERTEX_FIELDS = ["packed_position", "packed_rotation", "packed_scale", "packed_color"]
BASE_FIELDS = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2",
               "rot_0", "rot_1", "rot_2", "rot_3"]   # :49-56

# the order in which the reference's loop first reads each property (:70-104): numpy's error names the first one missing
READ_ORDER = ([("vertex", "packed_position")] + [("chunk", f) for f in CHUNK_FIELDS[0:6]] + [("vertex", "packed_rotation")]
              + [("vertex", "packed_scale")] + [("chunk", f) for f in CHUNK_FIELDS[6:12]] + [("vertex", "packed_color")]
              + [("chunk", f) for f in CHUNK_FIELDS[12:18]])

PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
             "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
WANT_TYPE = {"chunk": "f4", "vertex": "u4", "sh": "u1"}   # what the device path takes (the reference's own writer's types)


class PlyHeaderError(ValueError):
    """not a PLY header this parser understands"""


class UnsupportedPlyError(ValueError):
    """valid PLY that the device path does not take, with no reference reader (plyfile) to hand it to"""


class PlyElement:
    def __init__(self, name: str, count: int):
        self.name, self.count = name, count
        self.props = []          # (name, numpy type str, or ("list", count type, item type))
        self.offset = {}         # property -> byte offset inside a row (scalar properties only)
        self.stride = 0
        self.body_offset = None  # byte offset of the element's body in the file (binary bodies without list properties)

    def names(self):
        return [p[0] for p in self.props]

    def has_list(self) -> bool:
        return any(isinstance(t, tuple) for _, t in self.props)


class PlyHeader:
    def __init__(self):
        self.format = None
        self.elements = []
        self.header_bytes = 0

    def element(self, name):
        for e in self.elements:
            if e.name == name:
                return e
        return None

    def refusal(self) -> "str | None":
        """-> why the device path does not take this file (the reference's own read does), or None"""
        if self.element("chunk") is None:
            return "no 'chunk' element (the reference reads it as a 3DGS PLY)"
        if self.format != "binary_little_endian":
            return "a %s body" % self.format
        for e in self.elements:
            if e.has_list():
                return "list property %r of element %r" % (next(p for p, t in e.props if isinstance(t, tuple)), e.name)
        for kind in ("chunk", "vertex", "sh"):
            e = self.element(kind)
            if e is None:
                continue
            for p, t in e.props:
                if (kind != "sh" and p not in (CHUNK_FIELDS if kind == "chunk" else VERTEX_FIELDS)) or t == WANT_TYPE[kind]:
                    continue
                return "property %r of element %r is %s (the device path reads %s)" % (p, kind, t, WANT_TYPE[kind])
        sh, vertex = self.element("sh"), self.element("vertex")
        if sh is not None and sh.props:
            if len(sh.props) > _lib.CPLY_READ_MAX_SH:
                return "%d sh properties (the device path reads up to %d)" % (len(sh.props), _lib.CPLY_READ_MAX_SH)
            if vertex is not None and sh.count < min(vertex.count, CHUNK_SIZE * self.element("chunk").count):
                return "an sh element of %d rows for %d vertices" % (sh.count, vertex.count)
        return None


def parse_header(path: str) -> PlyHeader:
    """The PLY header of `path`: format, elements, properties; for a binary body without list properties also every scalar
    property's byte offset, every element's row stride and the byte offset of its body."""
    h = PlyHeader()
    with open(path, "rb") as f:
        first = f.readline()
        if first.rstrip(b"\r\n") != b"ply":
            raise PlyHeaderError("%s: not a PLY file (first line %r)" % (path, first[:32]))
        while True:
            raw = f.readline()
            if not raw:
                raise PlyHeaderError("%s: no end_header" % path)
            words = raw.decode("ascii", "replace").split()
            if not words or words[0] in ("comment", "obj_info"):
                continue
            key = words[0]
            if key == "end_header":
                break
            if key == "format":
                if len(words) != 3 or words[1] not in ("ascii", "binary_little_endian", "binary_big_endian"):
                    raise PlyHeaderError("%s: bad format line %r" % (path, raw))
                h.format = words[1]
            elif key == "element":
                if len(words) != 3:
                    raise PlyHeaderError("%s: bad element line %r" % (path, raw))
                h.elements.append(PlyElement(words[1], int(words[2])))
            elif key == "property":
                if not h.elements:
                    raise PlyHeaderError("%s: property before any element" % path)
                if len(words) == 5 and words[1] == "list":
                    if words[2] not in PLY_TYPES or words[3] not in PLY_TYPES:
                        raise PlyHeaderError("%s: bad property line %r" % (path, raw))
                    h.elements[-1].props.append((words[4], ("list", PLY_TYPES[words[2]], PLY_TYPES[words[3]])))
                elif len(words) == 3 and words[1] in PLY_TYPES:
                    h.elements[-1].props.append((words[2], PLY_TYPES[words[1]]))
                else:
                    raise PlyHeaderError("%s: bad property line %r" % (path, raw))
            else:
                raise PlyHeaderError("%s: unknown header line %r" % (path, raw))
        h.header_bytes = f.tell()
    if h.format is None:
        raise PlyHeaderError("%s: no format line" % path)
    if h.format != "ascii" and not any(e.has_list() for e in h.elements):
        pos = h.header_bytes
        for e in h.elements:
            off = 0
            for p, t in e.props:
                e.offset[p] = off
                off += np.dtype(t).itemsize
            e.stride = off
            e.body_offset = pos
            pos += e.stride * e.count
    return h


def sh_degree(n_coeffs: int) -> int:
    """:37-43"""
    if n_coeffs >= 45:
        return 3
    if n_coeffs >= 24:
        return 2
    if n_coeffs >= 9:
        return 1
    return 0


def output_dtype(sh_names) -> np.dtype:
    """:49-60 -- np.dtype raises as the reference does for an sh property that repeats a base name"""
    return np.dtype([(n, "f4") for n in BASE_FIELDS] + [(n, "f4") for n in sh_names])


def check_properties(h: PlyHeader):
    """the reference's first failing read in its loop (:70-104), when that loop runs at all: numpy's ValueError"""
    chunk, vertex = h.element("chunk"), h.element("vertex")
    if chunk.count == 0 or vertex.count == 0:
        return
    for kind, name in READ_ORDER:
        if name not in (chunk if kind == "chunk" else vertex).names():
            raise ValueError("no field of name %s" % name)


def layout_of(h: PlyHeader) -> "_lib.CplyReadLayout":
    chunk, vertex, sh = h.element("chunk"), h.element("vertex"), h.element("sh")
    lay = _lib.CplyReadLayout()
    lay.chunk_stride, lay.vertex_stride = chunk.stride, vertex.stride
    for i, f in enumerate(CHUNK_FIELDS):
        lay.chunk_offset[i] = chunk.offset[f]
    for i, f in enumerate(VERTEX_FIELDS):
        lay.vertex_offset[i] = vertex.offset[f]
    names = sh.names() if sh is not None else []
    lay.n_sh = len(names)
    lay.sh_stride = sh.stride if names else 0
    for i, f in enumerate(names):
        lay.sh_offset[i] = sh.offset[f]
    return lay


def read_compressed_ply(path: str, stage_ms: "dict | None" = None, fallback=None, on_metadata=None, profile: "dict | None" = None, keep: "dict | None" = None):
    """:14-124 -> (rows, metadata): the reference's structured array (BASE_FIELDS, then the sh element's properties in file
    order, all <f4) and its metadata dict (count, sh_degree, chunks).

    fallback: a function path -> (rows, metadata) for the files the device path does not take (PlyHeader.refusal: no `chunk`
    element, an ascii or big-endian body, list properties, other property types); without one such files raise
    UnsupportedPlyError.  on_metadata: called with the metadata as soon as it is known (where the reference sets
    ``self.metadata``, before its loop can fail).  stage_ms: a dict that receives per-stage clocks (tools/probe_cply_read.py).
    profile: a dict that receives the returned table's profile (_lib.TableProfile.as_dict), the zero rows past 256 x chunks
    included, from one more pass over the decoded rows before their download (stage clock "profile").  keep: a dict that receives the decoded rows in HBM as keep["rows"] (_lib.ResidentRows; the caller
    closes it) when the returned table's rows are resident; it stays empty otherwise.  The zero rows past 256 x chunks are zeroed on the device too."""
    return _lib.with_keep(keep, lambda: _lib.with_profile(profile, lambda: _read(path, stage_ms, fallback, on_metadata, profile, keep)))


def _read(path, stage_ms, fallback, on_metadata, profile, keep=None):
    debug_print(f"[DEBUG] Reading Compressed PLY file from {path}")
    t0 = time.perf_counter()
    h = parse_header(path)
    why = h.refusal()
    if why is not None:
        if fallback is None:
            raise UnsupportedPlyError("%s: %s -- the GPU compressed-PLY reader takes binary little-endian files with `chunk`, `vertex` "
                                      "and optional `sh` elements of scalar properties; this one needs the reference's reader "
                                      "(plyfile)" % (path, why))
        debug_print(f"[DEBUG] Compressed PLY: {why}; the reference's reader takes it")
        return fallback(path)
    chunk, vertex, sh = h.element("chunk"), h.element("vertex"), h.element("sh")
    if vertex is None:
        raise KeyError("vertex")           # plyfile's PlyData['vertex']
    sh_names = sh.names() if sh is not None else []
    metadata = {"count": vertex.count, "sh_degree": sh_degree(len(sh_names)), "chunks": chunk.count}
    if on_metadata is not None:
        on_metadata(metadata)
    dtype = output_dtype(sh_names)
    check_properties(h)
    if stage_ms is not None:
        stage_ms["parse"] = round((time.perf_counter() - t0) * 1e3, 3)
    n_dec = min(vertex.count, CHUNK_SIZE * chunk.count)
    if n_dec == 0:                         # the loop decodes nothing: :60's zeros
        return np.zeros(vertex.count, dtype), metadata
    segments = {"chunk": (chunk.body_offset, chunk.stride * chunk.count), "vertex": (vertex.body_offset, vertex.stride * n_dec),
                "sh": (sh.body_offset, sh.stride * n_dec) if sh_names else None}
    rows = _lib.cply_unpack_table(path, segments, layout_of(h), chunk.count, vertex.count, dtype, stage_ms=stage_ms, **_lib.profile_kw(profile), **_lib.keep_kw(keep))
    debug_print(f"Compressed PLY read completed. {vertex.count} points in {chunk.count} chunks.")
    return rows, metadata


def plyfile_available() -> bool:
    """is a real plyfile importable (the reference's own reader needs it)?"""
    try:
        import plyfile
    except ImportError:
        return False
    return hasattr(getattr(plyfile, "PlyData", None), "read")


def bind_read(original):
    """-> a replacement for ``CompressedPlyFormat.read`` that decodes on the device and sets ``self.metadata``; files the device
    path does not take go to `original` (the reference's read) when plyfile is there"""
    def read(self, path, **kwargs):
        def fallback(p):
            rows = original(self, p, **kwargs)
            return rows, getattr(self, "metadata", None)
        rows, _ = read_compressed_ply(path, fallback=fallback if plyfile_available() else None,
                                      on_metadata=lambda m: setattr(self, "metadata", m))
        return rows
    read.__wrapped__ = original
    return read
