"""Build tests/golden/spz_read_ref.npz from the REFERENCE's own SPZ reader (build box only: needs the reference).

The reference's ``SpzFormat().read`` (formats/spz.py:18-47, :175-296) runs unchanged on every case.  The input files come from
tests/spz_read_numpy.py's builders (random bytes in every section, every version and degree, edge fractional bits, gzip
containers of several kinds) and are stored whole.  Per case the spec records the reference's dtype names / types and its rows
(whole for small cases, sha256 of the row bytes for larger ones), or the exception it raised: type and message.  The degree-4
case records names and row count only.

    python tests/devtools/make_golden_spz_read.py
"""
import io
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import spz_read_numpy as srn  # noqa: E402
from oracle import refload  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "spz_read_ref.npz")
WHOLE_BELOW = 6000           # row bytes up to this are stored whole


def reference_read(path):
    refload.load()
    import gsconverter.formats.spz as mod  # type: ignore
    try:
        with np.errstate(all="ignore"):
            return mod.SpzFormat().read(path), None
    except Exception as e:  # noqa: BLE001 -- the reference's own error is the expected result
        return None, [type(e).__module__ + "." + type(e).__name__, str(e)]


def cases():
    """-> [(name, file bytes)]"""
    rng = np.random.default_rng(20261017)
    out = []

    def payload(version, degree, n, bits=12, **head):
        return srn.header(version, n, degree, bits, **head) + srn.random_body(version, degree, n, rng)

    for version in (1, 2, 3):
        for degree in (0, 1, 2, 3):
            out.append(("v%d_d%d" % (version, degree), srn.wrap(payload(version, degree, 23 + 5 * degree + version), 0)))
    for bits in (0, 12, 24, 127, 128, 255):
        out.append(("bits%d" % bits, srn.wrap(payload(2, 1, 19, bits), 0)))
    for version in (1, 3):
        out.append(("n0_v%d" % version, srn.wrap(payload(version, 2, 0), 0)))
    out.append(("n0_plain", payload(3, 0, 0)))
    p = payload(3, 2, 150)
    out.append(("plain", p))
    for level in (0, 6, 9):
        out.append(("gzip%d" % level, srn.wrap(p, level)))
    cut = 16 + 1234
    two = srn.wrap(p[:cut], 6) + srn.wrap(p[cut:], 0)
    out.append(("two_members", two))
    out.append(("two_members_header_split", srn.wrap(p[:7], 1) + srn.wrap(p[7:], 1)))
    out.append(("zero_padding", srn.wrap(p, 6) + bytes(700)))
    out.append(("zero_padding_between", srn.wrap(p[:cut], 6) + bytes(33) + srn.wrap(p[cut:], 6) + bytes(5)))
    out.append(("err_trailing_garbage", srn.wrap(p, 6) + b"garbage after the stream"))
    g = srn.wrap(p, 6)
    out.append(("err_truncated_stream", g[:len(g) // 2]))
    out.append(("err_truncated_trailer", g[:-3]))
    bad = bytearray(g)
    bad[-8] ^= 0x55
    out.append(("err_crc", bytes(bad)))
    bad = bytearray(g)
    bad[-1] ^= 0x01
    out.append(("err_length", bytes(bad)))
    bad = bytearray(g)
    bad[len(g) // 2] ^= 0xFF
    out.append(("err_damaged_deflate", bytes(bad)))
    out.append(("err_crc_and_magic", _flip_crc(srn.wrap(b"XXXX" + p[4:], 0))))
    out.append(("err_short_plain", p[:11]))
    out.append(("err_short_gzip", srn.wrap(p[:15], 6)))
    out.append(("err_empty", b""))
    out.append(("err_one_byte", b"\x1f"))
    out.append(("err_gzip_magic_only", b"\x1f\x8b"))
    out.append(("err_gzip_magic_plus_one", b"\x1f\x8b\x08"))
    out.append(("err_magic", struct.pack("<I", 0x12345678) + p[4:]))
    out.append(("err_magic_gzip", srn.wrap(struct.pack("<I", 0xDEADBEEF) + p[4:], 6)))
    for v in (0, 4):
        out.append(("err_version%d" % v, srn.wrap(p[:4] + struct.pack("<I", v) + p[8:], 0)))
    out.append(("err_version4_plain", p[:4] + struct.pack("<I", 4) + p[8:]))
    for version, degree in ((2, 3), (1, 1), (3, 0)):
        n = 21
        full = payload(version, degree, n)
        ends = np.cumsum([n * b for b in srn.section_bytes(version, degree)])
        for k, e in enumerate(ends):
            if k == 5 and degree == 0:
                continue
            out.append(("err_short_v%d_d%d_s%d" % (version, degree, k), srn.wrap(full[:16 + int(e) - 1], 0 if k % 2 else None)))
    out.append(("err_short_no_body", srn.wrap(p[:16], 0)))
    out.append(("bytes_after_body", srn.wrap(p + bytes(range(77)), 0)))
    out.append(("bytes_after_body_plain", p + b"\xff" * 5))
    out.append(("flags_reserved", srn.wrap(payload(3, 1, 17, flags=0xA5, reserved=0x5A), 6)))
    out.append(("degree4", srn.wrap(srn.header(3, 9, 4) + srn.random_body(3, 0, 9, rng), 0)))
    out.append(("larger_v3", srn.wrap(payload(3, 3, 700), 0)))
    out.append(("larger_v1", srn.wrap(payload(1, 2, 900), 6)))
    return out


def _flip_crc(g: bytes) -> bytes:
    b = bytearray(g)
    b[-6] ^= 0x10
    return bytes(b)


def main():
    import tempfile
    spec, arrays = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, data in cases():
            path = os.path.join(tmp, name + ".spz")
            with open(path, "wb") as f:
                f.write(data)
            arrays[name + "__file"] = np.frombuffer(data, np.uint8)
            rows, err = reference_read(path)
            rec = {}
            if err is not None:
                rec["error"] = err
            else:
                rec["names"] = list(rows.dtype.names)
                rec["rows"] = len(rows)
                if name != "degree4":
                    rec["dtype"] = [rows.dtype[f].str for f in rows.dtype.names]
                    rec["itemsize"] = rows.dtype.itemsize
                    raw = np.ascontiguousarray(rows).view(np.uint8).reshape(-1)
                    if raw.nbytes <= WHOLE_BELOW:
                        arrays[name + "__rows"] = raw.copy()
                    else:
                        arrays[name + "__sha256"] = np.frombuffer(srn.sha(rows), np.uint8)
                    rec["nan_words"] = int(sum(np.isnan(rows[f]).sum() for f in rows.dtype.names if rows.dtype[f].kind == "f"))
            spec[name] = rec
            print(name, rec.get("error") or ("%d rows, %d NaN words" % (rec["rows"], rec.get("nan_words", 0))))
    arrays["spec"] = np.frombuffer(json.dumps(spec, sort_keys=True).encode(), np.uint8)
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print(OUT, len(buf.getvalue()), "bytes")


if __name__ == "__main__":
    main()
