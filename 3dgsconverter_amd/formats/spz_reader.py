"""``read_spz`` -- the reference's ``SpzFormat.read`` (formats/spz.py:18-47, :175-296) with its per-field decode on the MI355X.

  | step (formats/spz.py)                           | here                                                                 |
  |-------------------------------------------------|----------------------------------------------------------------------|
  | :21-29 read the file, `gzip.decompress`         | a streamed inflate in bounded chunks straight into page-locked       |
  |                                                 | staging (an un-gzipped file is read into it); no second full copy     |
  | :31-43 the 16-byte header and its three errors  | the same `struct.unpack`, the same messages, in the same order       |
  | :175-251 `np.frombuffer` per section            | one size check: "buffer is smaller than requested size" is the only  |
  |                                                 | message that chain can raise (each offset is covered by the section  |
  |                                                 | before it)                                                           |
  | :182-250 the vectorised decode, field by field  | gsx_spz_unpack_dev (csrc/spz_read.hip): one launch, whole rows       |

The rows are the reference's bit for bit ("SPZ reader").  A damaged gzip stream raises what the reference raises,
because on any failure of the streamed inflate the reference's own statement runs on the file's bytes.  What shows only when a
gzip stream ends -- a bad CRC, a body shorter than the header promises -- is raised with the staging held and nothing uploaded;
every other error comes before the device is touched.  Files the device path does not take (``UnsupportedSpzError``: an SH
degree above 3) go to the reference's own read when there is one.
"""
from __future__ import annotations

import gzip
import os
import struct
import time
import zlib

import numpy as np

from .. import _lib
from ..utils import debug_print
from .spz_writer import HEADER, MAGIC

BASE_BEFORE = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]       # structures.py:39-47
BASE_AFTER = ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
COLOURS = ["red", "green", "blue"]                                                  # :50
CHUNK = 1 << 20                # bytes read and inflated at a time
TOO_SHORT = "Decompressed SPZ data too short for header"                            # spz.py:32
SMALLER = "buffer is smaller than requested size"                                   # np.frombuffer


class UnsupportedSpzError(ValueError):
    """a .spz file the device path does not take, with no reference reader to hand it to"""


def define_dtype(degree: int) -> np.dtype:
    """GaussianStruct.define_dtype(has_scal=False, has_rgb=True, sh_degree=degree) (structures.py:23-59), packed"""
    n_coeffs = 3 * ((degree + 1) ** 2 - 1)
    return np.dtype([(f, "<f4") for f in BASE_BEFORE] + [("f_rest_%d" % i, "<f4") for i in range(n_coeffs)]
                    + [(f, "<f4") for f in BASE_AFTER] + [(f, "u1") for f in COLOURS])


def inflate_chunks(f, chunk: int = CHUNK):
    """the gzip members of the open file `f`, inflated: a generator of at most `chunk` bytes at a time.  As gzip.decompress
    does, it follows one member with the next and skips zero bytes between and after them; a stream that ends early, fails its
    CRC or is followed by anything else raises (zlib.error or EOFError: the caller turns to the reference's statement)."""
    d, buf = zlib.decompressobj(wbits=31), b""
    while True:
        if not buf:
            buf = f.read(chunk)
            if not buf:
                break
        if d is None:
            buf = buf.lstrip(b"\x00")
            if not buf:
                continue
            d = zlib.decompressobj(wbits=31)
        out = d.decompress(buf, chunk)
        buf = d.unconsumed_tail
        if out:
            yield out
        if d.eof:
            buf, d = d.unused_data, None
    while d is not None and not d.eof:           # the file has ended: what the stream still holds
        out = d.decompress(b"", chunk)
        if not out:
            break
        yield out
    if d is not None and not d.eof:
        raise EOFError("Compressed file ended before the end-of-stream marker was reached")


class Source:
    """the bytes behind a generator of chunks, taken in order: a few for the header, the body into a buffer, the rest counted"""

    def __init__(self, chunks):
        self._it, self._left = iter(chunks), memoryview(b"")

    def _next(self) -> bool:
        while not len(self._left):
            c = next(self._it, None)
            if c is None:
                return False
            self._left = memoryview(c)
        return True

    def read(self, n: int) -> bytes:
        parts = []
        while n and self._next():
            parts.append(bytes(self._left[:n]))
            self._left = self._left[len(parts[-1]):]
            n -= len(parts[-1])
        return b"".join(parts)

    def readinto(self, view) -> int:
        view, got = memoryview(view), 0
        while got < len(view) and self._next():
            k = min(len(view) - got, len(self._left))
            view[got:got + k] = self._left[:k]
            self._left = self._left[k:]
            got += k
        return got

    def drain(self) -> int:
        """inflate and drop what is left, so that a truncated stream or a bad CRC behind the needed bytes still fails"""
        n = len(self._left)
        self._left = memoryview(b"")
        for c in self._it:
            n += len(c)
        return n


def parse_header(head: bytes):
    """:31-43 -> (version, n, degree, fractional_bits); flags and reserved are read and ignored"""
    if len(head) < _lib.SPZ_HEADER_BYTES:
        raise ValueError(TOO_SHORT)
    magic, version, n, degree, bits, _flags, _reserved = struct.unpack(HEADER, head)
    if magic != MAGIC:
        raise ValueError(f"Invalid SPZ magic number: {hex(magic)}")
    if version < 1 or version > 3:
        raise ValueError(f"Unsupported SPZ version: {version}")
    debug_print(f"[DEBUG] SPZ Header: Ver={version}, N={n}, SH={degree}, Bits={bits}")
    return version, n, degree, bits


def _installed_original():
    """the reference's own ``SpzFormat.read`` when install() has saved one -> a function path -> rows, or None"""
    from ..install import _saved
    original = _saved.get(("spzformat", "read"))
    if original is None:
        return None

    def fallback(path):
        import gsconverter.formats.spz as mod  # type: ignore
        return original(mod.SpzFormat(), path)
    return fallback


def _decode(path, src: "Source | None", head: bytes, avail: "int | None", fill_stage, t0, stage_ms, device, fallback, profile=None, keep=None):
    """the header `head`, then the body: from `src` (an inflated stream; its length shows only at its end) or, without one,
    from byte 16 of the file (`avail` body bytes)"""
    try:
        version, n, degree, bits = parse_header(head)
    except ValueError:
        if src is not None:
            src.drain()                          # the reference inflates first: a damaged stream's error comes before the header's
        raise
    if degree > 3:                               # (:178 the reference builds 3 ((d + 1)^2 - 1) zero f_rest fields, :265 reads no sh)
        fallback = fallback or _installed_original()
        if fallback is None:
            raise UnsupportedSpzError("%s: SH degree %d (the device path writes rows of degree 0 ... 3) -- the GPU SPZ reader does "
                                      "not take this file and there is no reference reader to hand it to" % (path, degree))
        debug_print(f"[DEBUG] SPZ: SH degree {degree}; the reference's reader takes it")
        return fallback(path)
    dtype = define_dtype(degree)
    need = _lib.spz_body_bytes(version, degree, n)
    if stage_ms is not None:
        stage_ms["parse"] = round((time.perf_counter() - t0) * 1e3, 3)
    if src is None and avail < need:
        raise ValueError(SMALLER)
    if n == 0:
        if src is not None:
            src.drain()
        return np.zeros(0, dtype)

    def fill(host):
        if src is None:
            with open(path, "rb") as f:
                f.seek(_lib.SPZ_HEADER_BYTES)
                _lib.read_exact(f, host[:need], path, unit="body bytes")
            return
        got = src.readinto(host[:need])
        src.drain()
        if got < need:
            raise ValueError(SMALLER)
    rows = _lib.spz_unpack_table(fill, need, version, degree, bits, n, dtype, stage_ms=stage_ms, device=device, fill_stage=fill_stage, **_lib.profile_kw(profile), **_lib.keep_kw(keep))
    debug_print(f"[DEBUG] SPZ read completed. {n} splats of degree {degree}.")
    return rows


def read_spz(path: str, stage_ms: "dict | None" = None, device: int = 0, *, fallback=None, profile: "dict | None" = None, keep: "dict | None" = None) -> np.ndarray:
    """:18-47 -> the reference's structured array: define_dtype(has_rgb=True) of the file's SH degree, float32 fields then red
    green blue as bytes, packed; nx ny nz zero.

    fallback: a function path -> rows for the files the device path does not take; by default the reference's own read when
    install() has saved one, else such files raise UnsupportedSpzError.  stage_ms: a dict that receives the stage clocks parse,
    inflate (file_read for a file that is not gzipped), upload, kernel, download (tools/probe_spz_read.py).  profile: a dict that receives the returned table's profile
    (_lib.TableProfile.as_dict) from one more pass over the decoded rows before their download (stage clock "profile").  keep: a dict that receives the decoded rows in HBM as keep["rows"] (_lib.ResidentRows; the caller
    closes it) when the returned table's rows are resident; it stays empty otherwise."""
    return _lib.with_keep(keep, lambda: _lib.with_profile(profile, lambda: _read(path, stage_ms, device, fallback, profile, keep)))


def _read(path, stage_ms, device, fallback, profile, keep=None):
    debug_print(f"[DEBUG] Reading .spz file from {path}")
    t0 = time.perf_counter()
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(_lib.SPZ_HEADER_BYTES)
    if not (size > 2 and head[:2] == b"\x1f\x8b"):                                  # :25
        return _decode(path, None, head, size - len(head), "file_read", t0, stage_ms, device, fallback, profile, keep)
    try:
        with open(path, "rb") as f:
            src = Source(inflate_chunks(f))
            return _decode(path, src, src.read(_lib.SPZ_HEADER_BYTES), None, "inflate", t0, stage_ms, device, fallback, profile, keep)
    except (zlib.error, EOFError):
        pass
    with open(path, "rb") as f:                                                      # :22, :29 -- the reference's statement raises
        raw = gzip.decompress(f.read())
    src = Source([memoryview(raw)[_lib.SPZ_HEADER_BYTES:]])                          # (a stream only gzip's own reader accepts)
    return _decode(path, src, raw[:_lib.SPZ_HEADER_BYTES], None, "inflate", t0, stage_ms, device, fallback, profile, keep)


def bind_read(original):
    """-> a replacement for ``SpzFormat.read`` that decodes on the device; a file the device path does not take goes to
    `original` (the reference's read)"""
    def read(self, path, **kwargs):
        return read_spz(path, fallback=lambda p: original(self, p, **kwargs))
    read.__wrapped__ = original
    return read
