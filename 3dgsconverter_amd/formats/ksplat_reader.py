"""``read_ksplat`` -- the reference's ``KSplatFormat.read`` (formats/ksplat.py:29-317) with its per-row decode on the MI355X.

  | step (formats/ksplat.py)                          | here                                                                |
  |---------------------------------------------------|---------------------------------------------------------------------|
  | :31-102 file header, section headers, metadata    | parse_headers: the same struct calls on the same slices             |
  | :104-145 payload walk: lengths, centres, rows     | plan: byte offsets and sizes from the headers and the file size     |
  | :148-156 one bucket index per splat (Python list) | prefix sums of the partially filled buckets' lengths, searched on   |
  |                                                   | the device (a few thousand words, never one index per row)          |
  | :161-261 the vectorised decode of a section       | gsx_ksplat_unpack_dev (csrc/ksplat_read.hip): one launch a section  |
  | :266-315 define_dtype, np.zeros, per-field scatter| the kernel writes every row whole, in define_dtype's field order    |

The rows are the reference's bit for bit, NaN bits included ("KSplat reader").  The reference has no checks of its
own: on a malformed file it raises whatever struct or numpy raise.  ``plan`` reproduces those exceptions -- type, and numpy's
or struct's own message -- from the headers and the file size alone, in the reference's order, before the device is touched.
Files the device path does not take (``UnsupportedKSplatError``) go to the reference's own read when there is one.
"""
from __future__ import annotations

import os
import struct
import time

import numpy as np

from .. import _lib
from ..utils import debug_print
from .ksplat_writer import HEADER_BYTES, MAGIC, SCALE_RANGE, SECTION_BYTES

BASE_BEFORE = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]       # structures.py:39-47
BASE_AFTER = ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
# :73-86: key, struct format, byte offset inside a section header, in the order the reference unpacks them
SECTION_FIELDS = (("splatCount", "I", 0), ("maxSplatCount", "I", 4), ("bucketSize", "I", 8), ("bucketCount", "I", 12),
                  ("bucketBlockSize", "f", 16), ("bucketStorageSizeBytes", "H", 20), ("compressionScaleRange", "I", 24),
                  ("storageSizeBytes", "I", 28), ("fullBucketCount", "I", 32), ("partiallyFilledBucketCount", "I", 36),
                  ("shDegree", "H", 40))
MAX_SECTIONS = 4096            # section headers the device path takes (one launch each)
MAX_BUCKET_ENTRIES = 1 << 36   # the reference builds a Python list this long (:152-155); past this it is refused, not imitated
NOT_MULTIPLE = "buffer size must be a multiple of element size"            # np.frombuffer
NOT_SCALAR_INDEX = "only integer scalar arrays can be converted to a scalar index"   # [][ndarray]


class UnsupportedKSplatError(ValueError):
    """a .ksplat file the device path does not take, with no reference reader to hand it to"""


def n_coeffs_of(degree: int) -> int:
    return 3 * ((degree + 1) ** 2 - 1)     # structures.py:36


def define_dtype(degree: int) -> np.dtype:
    """GaussianStruct.define_dtype(has_scal=False, has_rgb=False, sh_degree=degree) (structures.py:23-59)"""
    return np.dtype([(f, "f4") for f in BASE_BEFORE] + [("f_rest_%d" % i, "f4") for i in range(n_coeffs_of(degree))]
                    + [(f, "f4") for f in BASE_AFTER])


def sh_count_of(degree: int) -> int:
    """:138-140 -- 0 for anything but 1 and 2, degree 3 included"""
    return 9 if degree == 1 else (24 if degree == 2 else 0)


def row_bytes(level: int, sh_count: int) -> int:
    """:128-142 -- any level >= 2 reads the sh as u8"""
    if level == 0:
        return 44 + 4 * sh_count
    return 24 + (2 if level == 1 else 1) * sh_count


def parse_headers(path: str, on_metadata=None):
    """:31-102 -> (metadata, byte offset of the payload, file size).  The metadata dict is handed to `on_metadata` as soon as it
    exists (where the reference sets ``self.metadata``); its section list fills while the headers are read."""
    u = lambda fmt, data, off: struct.unpack_from(fmt, data, off)[0]   # noqa: E731  (:19-21 _unpack_at)
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(HEADER_BYTES)
        v_major, v_minor = head[0], head[1]
        if (v_major, v_minor) != MAGIC:
            debug_print(f"[DEBUG] Warning: KSplat version mismatch. Expected {MAGIC[0]}.{MAGIC[1]}, got {v_major}.{v_minor}")
        max_section_count = u("I", head, 4)
        u("I", head, 8)                     # sectionCount and maxSplatCount: read, not used
        u("I", head, 12)
        splat_count = u("I", head, 16)
        level = u("H", head, 20)
        min_sh, max_sh = u("f", head, 36), u("f", head, 40)
        debug_print(f"[DEBUG] KSplat: v{v_major}.{v_minor}, Splats={splat_count}, Compression={level}")
        metadata = {"v_major": v_major, "v_minor": v_minor, "splat_count": splat_count, "compression_level": level,
                    "min_sh": min_sh, "max_sh": max_sh, "sections": []}
        if on_metadata is not None:
            on_metadata(metadata)
        pos = len(head)
        for _ in range(max_section_count):   # maxSectionCount, not sectionCount; stops at the first empty read
            if len(metadata["sections"]) >= MAX_SECTIONS:
                raise UnsupportedKSplatError("more than %d section headers" % MAX_SECTIONS)
            data = f.read(SECTION_BYTES)
            if not data:
                break
            pos += len(data)
            info = {key: u(fmt, data, off) for key, fmt, off in SECTION_FIELDS}
            if info["compressionScaleRange"] == 0 and level >= 1:
                info["compressionScaleRange"] = SCALE_RANGE
            metadata["sections"].append(info)
    return metadata, pos, size


class SectionPlan:
    """where one section lies in the payload and what the kernel needs of its header"""
    __slots__ = ("lengths_offset", "n_lengths", "centres_offset", "n_centres", "rows_offset", "row_bytes", "sh_count", "n_rows",
                 "bucket_size", "n_full", "full_rows", "scale_range", "scale_factor", "out_row", "prefix_offset", "degree")


class Plan:
    __slots__ = ("level", "degree", "sections", "n_rows", "payload_offset", "body_bytes", "prefix")


def _partial_lengths(f, payload_offset, sp: SectionPlan) -> np.ndarray:
    f.seek(payload_offset + sp.lengths_offset)
    return np.frombuffer(f.read(4 * sp.n_lengths), dtype="<u4")


def plan(path: str, metadata: dict, payload_offset: int, size: int) -> Plan:
    """:104-210 from the headers and the file size: every section's offsets and counts, the reference's exception where its
    numpy calls would fail on this file (in its order), UnsupportedKSplatError for what the device path does not take."""
    level = metadata["compression_level"]
    heads = metadata["sections"]
    degree = max(s["shDegree"] for s in heads) if heads else 3          # :271-273
    plen = size - payload_offset

    def avail(a, b):   # len(payload_data[a:b])
        return max(0, min(b, plen) - min(a, plen))

    p = Plan()
    p.level, p.degree, p.sections, p.payload_offset = level, degree, [], payload_offset
    off, out_row, body_end, prefixes, n_prefix = 0, 0, 0, [], 0
    with open(path, "rb") as f:
        for s in heads:
            sp = SectionPlan()
            pfb, bc, n = s["partiallyFilledBucketCount"], s["bucketCount"], s["splatCount"]
            sp.lengths_offset, sp.n_lengths = off, 0
            if pfb > 0:                                                 # :113-115
                nb = avail(off, off + 4 * pfb)
                if nb % 4:
                    raise ValueError(NOT_MULTIPLE)
                sp.n_lengths = nb // 4
                off += 4 * pfb
            sp.centres_offset, sp.n_centres = off, 0
            if bc > 0:                                                  # :120-122
                nb = avail(off, off + 12 * bc)
                if nb % 4:
                    raise ValueError(NOT_MULTIPLE)
                if (nb // 4) % 3:
                    raise ValueError("cannot reshape array of size %d into shape (3)" % (nb // 4))
                sp.n_centres = nb // 12
                off += 12 * bc
            sp.degree = s["shDegree"]
            sp.sh_count = sh_count_of(sp.degree)
            sp.row_bytes = row_bytes(level, sp.sh_count)
            sp.rows_offset = off
            nb = avail(off, off + n * sp.row_bytes)                     # :144
            off += s["maxSplatCount"] * sp.row_bytes
            fb, bs = s["fullBucketCount"], s["bucketSize"]
            lengths = None
            if level >= 1:                                              # :149-156
                if fb * bs > MAX_BUCKET_ENTRIES:
                    raise UnsupportedKSplatError("full buckets of %d rows in a section of %d" % (fb * bs, n))
                if sp.n_lengths < pfb:
                    raise IndexError("index %d is out of bounds for axis 0 with size %d" % (sp.n_lengths, sp.n_lengths))
                lengths = _partial_lengths(f, payload_offset, sp).astype(np.int64) if pfb else np.zeros(0, np.int64)
            if nb % sp.row_bytes:                                       # :197
                raise ValueError(NOT_MULTIPLE)
            k = nb // sp.row_bytes
            sp.bucket_size, sp.n_full, sp.full_rows, sp.prefix_offset = bs, fb, 0, n_prefix
            sp.scale_range = sp.scale_factor = np.float32(0)
            if level >= 1:
                ends = fb * bs + np.cumsum(lengths)                     # rows up to and including each partially filled bucket
                covered = int(ends[-1]) if pfb else fb * bs
                m = min(covered, n)                                     # :156
                if fb + pfb > 0x7FFFFFFF and m > 0:
                    raise UnsupportedKSplatError("%d buckets in a section" % (fb + pfb))
                if bc == 0:                                             # :204 `[][b_indices]`
                    raise TypeError(NOT_SCALAR_INDEX)
                sp.full_rows = min(fb * bs, m)
                # :204 the first bucket index, in row order, past the centres that are there
                bad = None
                if sp.full_rows and (sp.full_rows + bs - 1) // bs > sp.n_centres:
                    bad = sp.n_centres
                elif pfb and m > sp.full_rows:
                    starts = ends - lengths
                    reach = np.nonzero((lengths > 0) & (starts < m) & (fb + np.arange(pfb) >= sp.n_centres))[0]
                    if len(reach):
                        bad = fb + int(reach[0])
                if bad is not None:
                    raise IndexError("index %d is out of bounds for axis 0 with size %d" % (bad, sp.n_centres))
                if k != m:                                              # :210 (k, 3) + (m, 3)
                    if k == 1 or m == 1:
                        raise UnsupportedKSplatError("%d splat rows broadcast against %d bucket assignments" % (k, m))
                    raise ValueError("operands could not be broadcast together with shapes (%d,3) (%d,3) " % (k, m))
                with np.errstate(all="ignore"):
                    sr = s["compressionScaleRange"]
                    sp.scale_factor = np.float32((s["bucketBlockSize"] / 2.0) / sr)   # :206, rounded to float32 once
                    sp.scale_range = np.float32(sr)                                  # :207, :210
                if pfb:
                    prefixes.append(np.minimum(ends, 0xFFFFFFFF).astype(np.uint32))
                    n_prefix += pfb
            sp.n_rows, sp.out_row = k, out_row
            out_row += k
            if k:
                body_end = max(body_end, sp.rows_offset + k * sp.row_bytes, (sp.centres_offset + 12 * sp.n_centres) if level >= 1 else 0)
            p.sections.append(sp)
    if degree > 3:   # (after the walk: the reference reaches define_dtype only when no section has raised)
        raise UnsupportedKSplatError("a section of SH degree %d (the device path writes rows of degree 0 ... 3)" % degree)
    p.n_rows, p.body_bytes = out_row, body_end
    p.prefix = np.concatenate(prefixes) if prefixes else np.zeros(0, np.uint32)
    return p


def device_sections(p: Plan):
    out = []
    for sp in p.sections:
        if sp.n_rows == 0:
            continue
        out.append(_lib.KsplatReadSection(sp.rows_offset, sp.centres_offset, sp.n_rows, sp.out_row, sp.full_rows, sp.prefix_offset,
                                          sp.bucket_size, sp.n_full, sp.n_lengths if p.level >= 1 else 0, sp.n_centres,
                                          sp.sh_count, float(sp.scale_range), float(sp.scale_factor)))
    return out


def _installed_original():
    """the reference's own ``KSplatFormat.read`` when install() has saved one -> a function path -> (rows, metadata), or None"""
    from ..install import _saved
    original = _saved.get(("ksplatformat", "read"))
    if original is None:
        return None

    def fallback(path):
        import gsconverter.formats.ksplat as mod  # type: ignore
        fmt = mod.KSplatFormat()
        rows = original(fmt, path)
        return rows, getattr(fmt, "metadata", None)
    return fallback


def read_ksplat(path: str, stage_ms: "dict | None" = None, device: int = 0, *, fallback=None, on_metadata=None,
                profile: "dict | None" = None, keep: "dict | None" = None):
    """:29-317 -> (rows, metadata): the reference's structured array (define_dtype of the largest section degree, all <f4; nx ny
    nz and the f_rest fields a section does not carry are 0) and its metadata dict.

    fallback: a function path -> (rows, metadata) for the files the device path does not take; by default the reference's own
    read when install() has saved one, else such files raise UnsupportedKSplatError.  on_metadata: called with the metadata as
    soon as the reference would have set ``self.metadata``.  stage_ms: a dict that receives the stage clocks parse, file_read,
    upload, kernel, download (tools/probe_ksplat_read.py).  profile: a dict that receives the returned table's profile
    (_lib.TableProfile.as_dict) from one more pass over the decoded rows before their download (stage clock "profile").  keep: a dict that receives the decoded rows in HBM as keep["rows"] (_lib.ResidentRows; the caller
    closes it) when the returned table's rows are resident; it stays empty otherwise."""
    return _lib.with_keep(keep, lambda: _lib.with_profile(profile, lambda: _read(path, stage_ms, device, fallback, on_metadata, profile, keep)))


def _read(path, stage_ms, device, fallback, on_metadata, profile, keep=None):
    debug_print(f"[DEBUG] Reading .ksplat file from {path}")
    t0 = time.perf_counter()
    try:
        metadata, payload_offset, size = parse_headers(path, on_metadata)
        p = plan(path, metadata, payload_offset, size)
    except UnsupportedKSplatError as e:
        fallback = fallback or _installed_original()
        if fallback is None:
            raise UnsupportedKSplatError("%s: %s -- the GPU .ksplat reader does not take this file and there is no reference "
                                         "reader to hand it to" % (path, e)) from None
        debug_print(f"[DEBUG] KSplat: {e}; the reference's reader takes it")
        return fallback(path)
    dtype = define_dtype(p.degree)
    if stage_ms is not None:
        stage_ms["parse"] = round((time.perf_counter() - t0) * 1e3, 3)
    if p.n_rows == 0:                      # :275-277, or sections without rows
        return np.zeros(0, dtype), metadata
    rows = _lib.ksplat_unpack_table(path, p.payload_offset, p.body_bytes, p.level, device_sections(p), p.prefix, n_coeffs_of(p.degree),
                                    p.n_rows, dtype, stage_ms=stage_ms, device=device, **_lib.profile_kw(profile), **_lib.keep_kw(keep))
    debug_print(f"[DEBUG] KSplat read completed. {p.n_rows} splats in {len(p.sections)} sections.")
    return rows, metadata


def bind_read(original):
    """-> a replacement for ``KSplatFormat.read`` that decodes on the device, sets ``self.metadata`` as the reference does and
    returns the rows alone; a file the device path does not take goes to `original` (the reference's read)"""
    def read(self, path, **kwargs):
        def fallback(p):
            rows = original(self, p, **kwargs)
            return rows, getattr(self, "metadata", None)
        rows, _ = read_ksplat(path, fallback=fallback, on_metadata=lambda m: setattr(self, "metadata", m))
        return rows
    read.__wrapped__ = original
    return read
