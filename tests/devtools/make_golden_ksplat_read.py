"""Build tests/golden/ksplat_read_ref.npz from the REFERENCE's own .ksplat reader (build box only: needs the reference).

The reference's ``KSplatFormat().read`` (formats/ksplat.py:29-317) runs unchanged on every case.  The input files are stored
whole: files the reference's own writer made, files from tests/ksplat_read_numpy.py's builder (several sections, many partially
filled buckets, padding, random row bytes, edge centres and block sizes) and malformed files.  Per case the spec records the
reference's dtype names / types, its metadata and its rows (whole for small cases, sha256 of the row bytes for larger ones), or
the exception it raised: type and message.

    python tests/devtools/make_golden_ksplat_read.py
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
import ksplat_read_numpy as krn  # noqa: E402
from oracle import refload  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ksplat_read_ref.npz")
WHOLE_BELOW = 12000          # row bytes up to this are stored whole


def reference_format():
    refload.load()
    import gsconverter.formats.ksplat as mod  # type: ignore
    return mod.KSplatFormat()


def reference_read(path):
    fmt = reference_format()
    try:
        rows = fmt.read(path)
    except Exception as e:  # noqa: BLE001 -- the reference's own error is the expected result
        return None, fmt.metadata, [type(e).__name__, str(e)]
    return rows, fmt.metadata, None


def scene(n, degree, rng):
    t = np.zeros(n, krn.define_dtype(degree))
    for f in t.dtype.names:
        t[f] = (rng.standard_normal(n) * (3.0 if f in "xyz" else 0.8)).astype(np.float32)
    return t


def f32(bits):
    return np.frombuffer(struct.pack("<I", bits), np.float32)[0]


def patch(path, edits=(), cut=None, append=b""):
    with open(path, "rb") as f:
        b = bytearray(f.read())
    for off, fmt, val in edits:
        struct.pack_into(fmt, b, off, val)
    if cut is not None:
        b = b[:cut]
    with open(path, "wb") as f:
        f.write(bytes(b) + append)


def cases(tmp):
    rng = np.random.default_rng(20261016)
    out = []

    def ref_written(name, n, degree, level, **kw):
        path = os.path.join(tmp, name + ".ksplat")
        reference_format().write(scene(n, degree, rng), path, level, **kw)
        out.append((name, path))
        return path

    def built(name, level, sections, **kw):
        path = krn.build_file(os.path.join(tmp, name + ".ksplat"), level, sections, **kw)
        out.append((name, path))
        return path

    S = krn.section
    SEC0 = krn.HEADER_BYTES                                   # first section header
    for level in (0, 1, 2, 7):
        for degree in (0, 1, 2):
            ref_written("ref_l%d_d%d" % (level, degree), 70 + 9 * degree + level, degree, level, bucket_size=32)
    for n in (0, 1, 255, 256, 257):
        ref_written("ref_n%d" % n, n, 1 if n > 1 else 0, 1)
    for bs in (1, 7, 5000):
        ref_written("ref_bucket%d" % bs, 60, 0, 2, bucket_size=bs)
    for blk in (0.37, -2.0):
        ref_written("ref_block%g" % blk, 50, 1, 1, block_size=blk, bucket_size=16)
    p = ref_written("ref_range0", 40, 0, 1, bucket_size=16)
    patch(p, [(SEC0 + 24, "<I", 0)])
    p = ref_written("ref_range0_level0", 40, 0, 0, bucket_size=16)
    patch(p, [(SEC0 + 24, "<I", 0)])
    p = ref_written("ref_version", 10, 0, 1)
    patch(p, [(0, "<B", 3), (1, "<B", 9)])
    for level in (0, 1, 2):
        built("header_degree3_l%d" % level, level, [S(level, 0, 33, rng, bucket_size=8, header_degree=3)])
    built("two_sections", 1, [S(1, 2, 90, rng, bucket_size=32, max_splats=100), S(1, 0, 41, rng, bucket_size=7, block_size=1.5)])
    built("three_sections", 2, [S(2, 1, 37, rng, bucket_size=5, max_splats=64), S(2, 2, 70, rng, bucket_size=64, max_splats=71),
                                S(2, 0, 19, rng, bucket_size=256, scale_range=1000)])
    built("three_sections_l0", 0, [S(0, 0, 20, rng), S(0, 2, 31, rng, max_splats=40), S(0, 1, 9, rng)])
    built("sections_l1_odd_rows", 1, [S(1, 1, 33, rng, bucket_size=4, max_splats=35), S(1, 1, 50, rng, bucket_size=50)])
    lens = rng.integers(0, 9, 60).astype(np.uint32)
    built("many_partial", 2, [S(2, 1, int(lens.sum()) + 24, rng, bucket_size=8, full_buckets=3, partial=lens)])
    built("partial_cover_more", 1, [S(1, 0, 30, rng, bucket_size=8, full_buckets=2, partial=[5, 0, 0, 40, 7])])
    built("full_cover_more", 1, [S(1, 0, 30, rng, bucket_size=8, full_buckets=9, partial=[3])])
    for level in (0, 1, 2):
        built("random_l%d" % level, level, [S(level, 2, 150, rng, bucket_size=16, block_size=0.37)])
    # NaN / infinite centres and block sizes: x86's NaN bits
    n = 67
    cen = np.zeros((9, 3), np.float32)
    cen.view(np.uint32)[:] = np.array([[0x7F800000, 0xFF800000, 0x7FC00000], [0x7F800123, 0xFFA00456, 0x7FC00789],
                                       [0x7F812345, 0x3F800000, 0xFFFFFFFF], [0x00000001, 0x80000005, 0x00400000],
                                       [0x7F7FFFFF, 0xFF7FFFFF, 0x80000000], [0x7F800000, 0x7F800000, 0x7F800000],
                                       [0xFF800000, 0xFF800000, 0xFF800000], [0x3F800000, 0xC0000000, 0x40400000],
                                       [0x7FC00ABC, 0x7F800000, 0xFFC00DEF]], np.uint32)
    rows = rng.integers(0, 256, (n, 24), dtype=np.uint8)
    rows.view(np.uint16)[::4, :3] = 32767                      # position == the range: 0 * inf
    for tag, blk in (("inf", f32(0x7F800000)), ("ninf", f32(0xFF800000)), ("nan", f32(0x7FC12345)), ("snan", f32(0xFF812345)),
                     ("zero", 0.0), ("tiny", f32(0x00000003)), ("huge", f32(0x7F7FFFFF)), ("one", 1.0)):
        built("edge_block_%s" % tag, 1, [S(1, 0, n, rng, rows=rows, bucket_size=8, block_size=blk, centres=cen)])
    built("edge_range", 2, [S(2, 0, n, rng, rows=rows, bucket_size=8, block_size=3.0, scale_range=0xFFFFFFFF, centres=cen),
                            S(2, 0, n, rng, rows=rows, bucket_size=8, block_size=3.0, scale_range=1, centres=cen),
                            S(2, 0, n, rng, rows=rows, bucket_size=8, block_size=f32(0x7F800000), scale_range=5, centres=cen)])
    built("edge_level0_nan", 0, [S(0, 1, 40, rng)])           # random float32 bits: NaN payloads must pass through
    built("max_sections_larger", 1, [S(1, 0, 12, rng, bucket_size=4)], max_section_count=5)
    built("no_sections", 1, [])
    built("no_sections_declared", 0, [], max_section_count=3)
    built("zero_rows_section", 1, [S(1, 1, 0, rng, bucket_size=4, bucket_count=2), S(1, 0, 5, rng, bucket_size=4)])
    built("zero_rows_no_buckets", 1, [S(1, 0, 0, rng, bucket_size=4)])
    built("level0_no_buckets", 0, [S(0, 0, 6, rng, bucket_count=0, full_buckets=0, partial=[])])
    # ---- malformed files: the reference's own exceptions
    p = built("err_empty_file", 1, [])
    patch(p, cut=0)
    p = built("err_short_header", 1, [])
    patch(p, cut=30)
    p = built("err_short_section_header", 1, [S(1, 0, 12, rng, bucket_size=4)])
    patch(p, cut=SEC0 + 38)
    p = built("err_cut_mid_row", 1, [S(1, 1, 40, rng, bucket_size=8)])
    patch(p, cut=os.path.getsize(p) - 17)
    p = built("err_cut_whole_rows", 2, [S(2, 0, 40, rng, bucket_size=8)])
    patch(p, cut=os.path.getsize(p) - 24 * 6)
    p = built("cut_whole_rows_level0", 0, [S(0, 0, 40, rng)])
    patch(p, cut=os.path.getsize(p) - 44 * 6)
    p = built("err_cut_mid_row_level0", 0, [S(0, 1, 40, rng)])
    patch(p, cut=os.path.getsize(p) - 5)
    p = built("err_cut_in_centres", 1, [S(1, 0, 40, rng, bucket_size=8)])
    patch(p, cut=SEC0 + 1024 + 12 * 2 + 7)
    p = built("err_cut_in_centres_words", 1, [S(1, 0, 40, rng, bucket_size=8)])
    patch(p, cut=SEC0 + 1024 + 12 * 2 + 8)
    p = built("err_cut_in_lengths", 1, [S(1, 0, 40, rng, bucket_size=8, full_buckets=0, partial=[8, 8, 8, 8, 8])])
    patch(p, cut=SEC0 + 1024 + 6)
    p = built("err_cut_lengths_words", 1, [S(1, 0, 40, rng, bucket_size=8, full_buckets=0, partial=[8, 8, 8, 8, 8])])
    patch(p, cut=SEC0 + 1024 + 8)
    built("err_buckets_cover_fewer", 1, [S(1, 0, 40, rng, bucket_size=8, full_buckets=2, partial=[5, 3], bucket_count=6)])
    built("err_bucket_index_past_count", 1, [S(1, 0, 40, rng, bucket_size=8, bucket_count=3)])
    built("err_bucket_index_past_count_partial", 2, [S(2, 0, 40, rng, bucket_size=8, full_buckets=1, partial=[3, 0, 0, 9, 20], bucket_count=3)])
    built("err_no_buckets_with_rows", 1, [S(1, 0, 10, rng, bucket_size=4, bucket_count=0)])
    built("err_second_section", 1, [S(1, 0, 12, rng, bucket_size=4), S(1, 0, 12, rng, bucket_size=4, bucket_count=1)])
    return out


def main():
    import tempfile
    spec, arrays = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, path in cases(tmp):
            with open(path, "rb") as f:
                arrays[name + "__file"] = np.frombuffer(f.read(), np.uint8)
            rows, meta, err = reference_read(path)
            rec = {"metadata": meta}
            if err is not None:
                rec["error"] = err
            else:
                rec["names"] = list(rows.dtype.names)
                rec["dtype"] = [rows.dtype[f].str for f in rows.dtype.names]
                rec["rows"] = len(rows)
                raw = np.ascontiguousarray(rows).view(np.uint8)
                if raw.nbytes <= WHOLE_BELOW:
                    arrays[name + "__rows"] = raw.view(np.uint32).copy()
                else:
                    arrays[name + "__sha256"] = np.frombuffer(krn.sha(rows), np.uint8)
                rec["nan_words"] = int(np.isnan(raw.view(np.float32)).sum())
            spec[name] = rec
            print(name, rec.get("error") or ("%d rows, %d NaN words" % (rec["rows"], rec["nan_words"])))
    arrays["spec"] = np.frombuffer(json.dumps(spec, sort_keys=True).encode(), np.uint8)
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print(OUT, len(buf.getvalue()), "bytes")


if __name__ == "__main__":
    main()
