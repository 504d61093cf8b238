"""Build tests/golden/cply_read_ref.npz, or with --wide tests/golden/cply_read_wide_ref.npz, from the REFERENCE's own
compressed-PLY reader (build box only: needs the reference).

The reference's ``CompressedPlyFormat.read`` (formats/compressed_ply.py:14-124) runs unchanged; only ``plyfile.PlyData.read``
(plyfile is not installed here) is replaced by a small numpy parser of the binary container.  The input files are stored whole:
files the reference's own writer made from oracle.cply scenes (its ``_write_ply_file`` intercepted, the elements written in
plyfile's layout), and synthetic files with edge words and edge bounds.  Outputs are stored whole for small cases, as sha256
of the row bytes for larger ones.

The wide file (wide_cases) holds sh elements of 38, 89, 192 and 256 properties -- one per tile geometry of csrc/cply_read.hip
past the degree-3 width -- the NaN chunks of edge_bounds under a 100-property sh element, and a 257-property file that the
reference reads and the device path refuses.  It has an rng of its own: cases() and cply_read_ref.npz are not touched by it.

    python tests/devtools/make_golden_cply_read.py            # cply_read_ref.npz
    python tests/devtools/make_golden_cply_read.py --wide     # cply_read_wide_ref.npz
"""
import io
import json
import os
import struct
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cply_read_numpy as crn  # noqa: E402
from oracle import cply as ocply, refload  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "cply_read_ref.npz")
OUT_WIDE = os.path.join(ROOT, "tests", "golden", "cply_read_wide_ref.npz")
WHOLE_BELOW = 40000          # row bytes up to this are stored whole


class _Element:
    def __init__(self, data):
        self.data = data


class _PlyData:
    """what the reference's read uses of plyfile.PlyData: `name in plydata` and `plydata[name].data`"""

    def __init__(self, elements):
        self._el = elements

    def __contains__(self, name):
        return name in self._el

    def __getitem__(self, name):
        return _Element(self._el[name])

    @staticmethod
    def read(path):
        return _PlyData(crn.read_ply(path))


def reference_read(path):
    stub = types.ModuleType("plyfile")
    stub.PlyData = _PlyData
    stub.PlyElement = object
    sys.modules["plyfile"] = stub
    refload.load()
    import gsconverter.formats.compressed_ply as mod  # type: ignore
    fmt = mod.CompressedPlyFormat()
    try:
        rows = fmt.read(path)
    except Exception as e:  # noqa: BLE001 -- the reference's own error is the expected result
        return None, getattr(fmt, "metadata", None), "%s: %s" % (type(e).__name__, e)
    return rows, fmt.metadata, None


def f32(bits):
    return np.frombuffer(struct.pack("<I", bits), np.float32)[0]


def chunk_table(nc, rng):
    ch = np.zeros(nc, [(f, "<f4") for f in crn.CHUNK_FIELDS])
    for group in (0, 6, 12):
        for k in range(3):
            lo, hi = crn.CHUNK_FIELDS[group + k], crn.CHUNK_FIELDS[group + 3 + k]
            a = (rng.standard_normal(nc) * 4).astype(np.float32)
            ch[lo], ch[hi] = a, a + np.abs(rng.standard_normal(nc) * 2).astype(np.float32)
    return ch


def vertex_table(n, rng):
    vt = np.zeros(n, [(f, "<u4") for f in crn.VERTEX_FIELDS])
    for f in crn.VERTEX_FIELDS:
        vt[f] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return vt


def sh_table(n, m, rng):
    sh = np.zeros(n, [("f_rest_%d" % i, "u1") for i in range(m)])
    sh.view(np.uint8).reshape(n, m)[:] = rng.integers(0, 256, (n, m), dtype=np.uint8)
    return sh


def edge_bounds():
    """one chunk row per edge: (lo, hi) bit pairs applied to every axis pair of the row"""
    inf, ninf = 0x7F800000, 0xFF800000
    pairs = [
        (0x3F800000, 0x3F800000),              # min == max
        (0x40000000, 0x3F800000),              # max < min
        (ninf, inf), (inf, inf), (ninf, ninf), (0x3F800000, inf), (ninf, 0x3F800000), (inf, 0x3F800000),
        (0x7F800123, 0x3F800000),              # signalling NaN min with a payload
        (0x3F800000, 0xFFA00456),              # NaN max with a payload, negative
        (0x7FC00789, 0xFF800ABC),              # both NaN
        (0x7F812345, inf),                     # NaN min, inf max
        (0x00000001, 0x00000003),              # denormals
        (0x80000005, 0x00000002),
        (0x00400000, 0x00800000),              # largest denormal / smallest normal
        (0x80000000, 0x00000000),              # -0, +0
        (0xFF7FFFFF, 0x7F7FFFFF),              # -max, +max: the float32 difference overflows
    ]
    ch = np.zeros(len(pairs), [(f, "<u4") for f in crn.CHUNK_FIELDS])
    for i, (lo, hi) in enumerate(pairs):
        for group in (0, 6, 12):
            for k in range(3):
                ch[crn.CHUNK_FIELDS[group + k]][i] = lo
                ch[crn.CHUNK_FIELDS[group + 3 + k]][i] = hi
    return ch.view([(f, "<f4") for f in crn.CHUNK_FIELDS])


def edge_words(n, rng):
    vt = vertex_table(n, rng)
    special = np.array([0, 0xFFFFFFFF, 0x3FFFFFFF, 0x40000000, 0x7FFFFFFF, 0x80000000, 0xBFFFFFFF, 0xC0000000, 0x000003FF,
                        0x7FF00000, 0x001FF800, 0x801FF7FF, 0x55555555, 0xAAAAAAAA, 0x000000FF, 0xFF000000], np.uint32)
    for j, f in enumerate(crn.VERTEX_FIELDS):
        k = np.arange(n) % (3 * len(special))
        sel = k < len(special)
        vt[f][sel] = np.roll(special, j)[k[sel]]
    for L in range(4):                         # every `largest` with the extreme 10-bit values
        for v in (0, 1, 511, 512, 1022, 1023):
            i = rng.integers(0, n)
            vt["packed_rotation"][i] = (L << 30) | (v << 20) | ((1023 - v) << 10) | v
    return vt


def cases(tmp):
    rng = np.random.default_rng(20261016)
    out = []

    def add(name, elements, fmt="binary_little_endian"):
        path = os.path.join(tmp, name + ".ply")
        crn.write_ply(path, elements, fmt)
        out.append((name, path))

    for deg, n, kind in ((0, 700, "clustered"), (1, 600, "uniform"), (2, 513, "clustered"), (3, 1000, "clustered")):
        scene = ocply.cply_scene(n, deg, kind)
        got = refload.reference_cply(scene)
        els = [("chunk", got["chunk"]), ("vertex", got["vertex"])] + ([("sh", got["sh"])] if got["sh"] is not None else [])
        add("ref_deg%d_%s" % (deg, kind), els)
    eb = edge_bounds()
    n_e = 256 * len(eb)
    add("edge_bounds", [("chunk", eb), ("vertex", vertex_table(n_e, rng)), ("sh", sh_table(n_e, 3, rng))])
    add("edge_words", [("chunk", chunk_table(6, rng)), ("vertex", edge_words(1400, rng))])
    add("partial_last_chunk", [("chunk", chunk_table(3, rng)), ("vertex", vertex_table(2 * 256 + 37, rng)), ("sh", sh_table(549, 24, rng))])
    add("fewer_chunks", [("chunk", chunk_table(2, rng)), ("vertex", vertex_table(700, rng)), ("sh", sh_table(700, 9, rng))])
    add("more_chunks", [("chunk", chunk_table(5, rng)), ("vertex", vertex_table(300, rng))])
    add("no_chunks", [("chunk", chunk_table(0, rng)), ("vertex", vertex_table(40, rng))])
    add("empty_vertex", [("chunk", chunk_table(1, rng)), ("vertex", vertex_table(0, rng)), ("sh", sh_table(0, 45, rng))])
    add("single_row", [("chunk", chunk_table(1, rng)), ("vertex", vertex_table(1, rng)), ("sh", sh_table(1, 45, rng))])
    # permuted property order, extra properties of other types, and an element before `chunk`
    ch = chunk_table(4, rng)
    ch_p = np.zeros(4, [("pad", "<f8")] + [(f, "<f4") for f in reversed(crn.CHUNK_FIELDS)] + [("tag", "u1")])
    for f in crn.CHUNK_FIELDS:
        ch_p[f] = ch[f]
    vt = vertex_table(1000, rng)
    vt_p = np.zeros(1000, [("packed_color", "<u4"), ("extra", "<i2"), ("packed_scale", "<u4"), ("packed_rotation", "<u4"),
                           ("w", "u1"), ("packed_position", "<u4")])
    for f in crn.VERTEX_FIELDS:
        vt_p[f] = vt[f]
    sh = sh_table(1000, 45, rng)
    sh_p = np.zeros(1000, [("f_rest_%d" % i, "u1") for i in rng.permutation(45)])
    for f in sh.dtype.names:
        sh_p[f] = sh[f]
    meta = np.zeros(2, [("a", "<i4"), ("b", "<f8")])
    add("permuted", [("camera", meta), ("chunk", ch_p), ("vertex", vt_p), ("sh", sh_p)])
    # the reference's errors: its loop reads packed_position, then min_x ... max_z, ... packed_color, min_r ... max_b
    ch_nr = np.zeros(1, [(f, "<f4") for f in crn.CHUNK_FIELDS if f != "min_g"])
    add("missing_min_g", [("chunk", ch_nr), ("vertex", vertex_table(10, rng))])
    vt_nc = np.zeros(10, [(f, "<u4") for f in crn.VERTEX_FIELDS if f != "packed_color"])
    add("missing_packed_color", [("chunk", chunk_table(1, rng)), ("vertex", vt_nc)])
    add("missing_both", [("chunk", ch_nr), ("vertex", vt_nc)])
    add("missing_but_empty", [("chunk", ch_nr), ("vertex", vertex_table(0, rng))])
    return out


# the chunk rows of edge_bounds() whose bounds reach each return of x86_nan (row_tile.h): an invalid operation of two numbers
# (-inf .. inf gives inf * 0 where a slot holds 0, inf .. inf gives inf - inf in every row), both NaN (max's bits win), a NaN
# max alone, a NaN min alone.  The chunk with both bounds NaN must be a whole one: there `(nv / t) * d + min` adds two NaNs,
# and which of them numpy's vectorised add returns depends on the element's place in the array -- on the AVX-512 build host
# the elements behind the last whole vector of 8 of an array longer than 8 take min's bits, all others max's.  A chunk of 256
# rows has no such tail, a partial last chunk has one, and its bits are the host's, not the reference's.
NAN_CHUNKS = [2, 3, 10, 9, 8]


def wide_cases(tmp):
    rng = np.random.default_rng(20261018)
    out = []

    def add(name, elements):
        path = os.path.join(tmp, name + ".ply")
        crn.write_ply(path, elements)
        out.append((name, path))

    def renamed(sh, names):
        return sh.view([(f, "u1") for f in names])

    # 290 rows: two chunks, the second one 34 rows, which ends inside a tile of 128, 64 or 32 rows
    n = 256 + 34
    add("sh38", [("chunk", chunk_table(2, rng)), ("vertex", vertex_table(n, rng)), ("sh", sh_table(n, 38, rng))])
    add("sh89_permuted", [("chunk", chunk_table(2, rng)), ("vertex", vertex_table(n, rng)),
                          ("sh", renamed(sh_table(n, 89, rng), ["f_rest_%d" % i for i in rng.permutation(89)]))])
    add("sh192_other_names", [("chunk", chunk_table(2, rng)), ("vertex", vertex_table(n, rng)),
                              ("sh", renamed(sh_table(n, 192, rng), ["coeff_%03d" % (191 - i) if i % 3 else "b%d" % i for i in range(192)]))])
    add("sh256", [("chunk", chunk_table(2, rng)), ("vertex", vertex_table(n, rng)), ("sh", sh_table(n, 256, rng))])
    # the NaN cold path at 64-row tiles: edge_bounds() trimmed to its NaN chunks (the 17 whole ones would take 505 KB of
    # random bytes), the last one 70 rows, which ends inside a tile
    n_e = 256 * (len(NAN_CHUNKS) - 1) + 70
    add("edge_bounds_sh100", [("chunk", edge_bounds()[NAN_CHUNKS]), ("vertex", vertex_table(n_e, rng)), ("sh", sh_table(n_e, 100, rng))])
    # one property more than the device path takes: the reference reads it
    add("sh257_refused", [("chunk", chunk_table(1, rng)), ("vertex", vertex_table(40, rng)), ("sh", sh_table(40, 257, rng))])
    return out


def record(make_cases, out_path):
    import tempfile
    spec, arrays = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, path in make_cases(tmp):
            with open(path, "rb") as f:
                arrays[name + "__file"] = np.frombuffer(f.read(), np.uint8)
            rows, meta, err = reference_read(path)
            rec = {"metadata": meta}
            if err is not None:
                rec["error"] = err
            else:
                rec["names"] = list(rows.dtype.names)
                rec["dtype"] = [rows.dtype[f].str for f in rows.dtype.names]
                raw = np.ascontiguousarray(rows).view(np.uint8)
                if raw.nbytes <= WHOLE_BELOW:
                    arrays[name + "__rows"] = raw.copy()
                else:
                    arrays[name + "__sha256"] = np.frombuffer(crn.sha(rows), np.uint8)
                mine, mmeta = crn.read(path)
                assert mine.dtype == rows.dtype and mine.tobytes() == rows.tobytes() and mmeta == meta, name
                rec["nan_rows"] = int(np.isnan(raw.view(np.float32)).any() if raw.nbytes else 0)
            spec[name] = rec
            print(name, rec.get("error") or ("%d rows" % rec["metadata"]["count"]))
    arrays["spec"] = np.frombuffer(json.dumps(spec, sort_keys=True).encode(), np.uint8)
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    with open(out_path, "wb") as f:
        f.write(buf.getvalue())
    print(out_path, len(buf.getvalue()), "bytes")
    return spec


def main():
    record(cases, OUT)


def main_wide():
    spec = record(wide_cases, OUT_WIDE)
    assert not any("error" in r for r in spec.values()) and spec["edge_bounds_sh100"]["nan_rows"] == 1
    assert [spec[k]["metadata"]["sh_degree"] for k in ("sh38", "sh89_permuted", "sh192_other_names", "sh256", "sh257_refused")] == [2, 3, 3, 3, 3]
    assert os.path.getsize(OUT_WIDE) <= os.path.getsize(OUT)


if __name__ == "__main__":
    main_wide() if sys.argv[1:] == ["--wide"] else main()
