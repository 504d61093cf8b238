"""A vectorised numpy restatement of the reference's compressed-PLY reader (gsconverter/formats/compressed_ply.py:14-124), used
by the host tests and the large checks: the same statements, in the same dtypes and order, over every row at once instead of
per 256-splat chunk.  Also a minimal binary PLY parser and writer (the container the reference reads through plyfile)."""
import hashlib

import numpy as np

CHUNK_FIELDS = (["min_x", "min_y", "min_z", "max_x", "max_y", "max_z"] + ["min_scale_x", "min_scale_y", "min_scale_z"]
                + ["max_scale_x", "max_scale_y", "max_scale_z"] + ["min_r", "min_g", "min_b", "max_r", "max_g", "max_b"])
VERTEX_FIELDS = ["packed_position", "packed_rotation", "packed_scale", "packed_color"]
BASE = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2",
        "rot_0", "rot_1", "rot_2", "rot_3"]
TYPES = {"char": "i1", "uchar": "u1", "short": "i2", "ushort": "u2", "int": "i4", "uint": "u4", "float": "f4", "double": "f8",
         "int8": "i1", "uint8": "u1", "int16": "i2", "uint16": "u2", "int32": "i4", "uint32": "u4", "float32": "f4", "float64": "f8"}
NAMES = {"i1": "char", "u1": "uchar", "i2": "short", "u2": "ushort", "i4": "int", "u4": "uint", "f4": "float", "f8": "double"}
SH_C0 = 0.28209479177387814


def write_ply(path, elements, fmt="binary_little_endian"):
    """elements: [(name, structured array)] -> a PLY file (scalar properties; the layout plyfile writes)"""
    head = ["ply", "format %s 1.0" % fmt]
    for name, arr in elements:
        head.append("element %s %d" % (name, len(arr)))
        for f in arr.dtype.names:
            head.append("property %s %s" % (NAMES[arr.dtype[f].str[1:]], f))
    head.append("end_header")
    order = ">" if fmt == "binary_big_endian" else "<"
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        for _, arr in elements:
            f.write(np.ascontiguousarray(arr).astype(arr.dtype.newbyteorder(order), copy=False).tobytes())


def read_ply(path):
    """binary little-endian PLY with scalar properties -> {element name: structured array} in header order"""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.index(b"end_header") + len(b"end_header")
    end = raw.index(b"\n", end) + 1
    elements = []
    for line in raw[:end].decode("ascii").splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "format":
            assert w[1] == "binary_little_endian", w
        elif w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property":
            assert w[1] != "list"
            elements[-1][2].append((w[2], "<" + TYPES[w[1]]))
    out, pos = {}, end
    for name, count, props in elements:
        dt = np.dtype(props)
        out[name] = np.frombuffer(raw, dt, count, pos).copy()
        pos += dt.itemsize * count
    return out


def sh_degree(m):
    return 3 if m >= 45 else 2 if m >= 24 else 1 if m >= 9 else 0


def decode(chunks, vertices, sh=None):
    """the reference's rows and metadata from the parsed elements"""
    n = len(vertices)
    sh_names = list(sh.dtype.names) if sh is not None else []
    dtype = np.dtype([(f, "f4") for f in BASE] + [(f, "f4") for f in sh_names])
    data = np.zeros(n, dtype)
    meta = {"count": n, "sh_degree": sh_degree(len(sh_names)), "chunks": len(chunks)}
    m = min(n, 256 * len(chunks))
    if m == 0:
        return data, meta
    ci = np.arange(m) // 256
    v = vertices[:m]
    c = {f: chunks[f][ci] for f in CHUNK_FIELDS}

    def den(nv, t, lo, hi):                                 # :346-347, with the float32 subtraction of :80
        out = (nv / t) * (c[hi] - c[lo]).astype(np.float64) + c[lo].astype(np.float64)
        # which NaN x86 returns depends on the operands' shapes (numpy's array-array loops pick another than its array-scalar
        # and scalar-scalar ones): chunks with a NaN bound are redone with the reference's own scalar statement
        for k in np.nonzero(np.isnan(chunks[lo]) | np.isnan(chunks[hi]))[0]:
            sl = slice(256 * k, min(m, 256 * (k + 1)))
            out[sl] = (nv[sl] / t) * (chunks[hi][k] - chunks[lo][k]) + chunks[lo][k]
        return out
    with np.errstate(all="ignore"):
        p = v["packed_position"]
        data["x"][:m] = den((p >> 21) & 0x7FF, 2047, "min_x", "max_x")
        data["y"][:m] = den((p >> 11) & 0x3FF, 1023, "min_y", "max_y")
        data["z"][:m] = den(p & 0x7FF, 2047, "min_z", "max_z")
        s = v["packed_scale"]
        data["scale_0"][:m] = den((s >> 21) & 0x7FF, 2047, "min_scale_x", "max_scale_x")
        data["scale_1"][:m] = den((s >> 11) & 0x3FF, 1023, "min_scale_y", "max_scale_y")
        data["scale_2"][:m] = den(s & 0x7FF, 2047, "min_scale_z", "max_scale_z")
        col = v["packed_color"]
        for k, (shift, a) in enumerate(((24, "r"), (16, "g"), (8, "b"))):
            cr = den((col >> shift) & 0xFF, 255.0, "min_" + a, "max_" + a)
            data["f_dc_%d" % k][:m] = (cr - 0.5) / SH_C0
        a = np.clip((col & 0xFF) / 255.0, 1e-6, 1.0 - 1e-6)
        data["opacity"][:m] = np.log(a / (1.0 - a))
        r = v["packed_rotation"]
        largest = r >> 30
        dv = [((r >> sh_) & 0x3FF) / 1023.0 for sh_ in (20, 10, 0)]
        dv = [(x - 0.5) / 0.7071067811865476 for x in dv]
        missing = np.sqrt(np.clip(1.0 - (dv[0] ** 2 + dv[1] ** 2 + dv[2] ** 2), 0, 1))
        q = np.zeros((m, 4), np.float32)
        for L in range(4):
            sel = largest == L
            others = [i for i in range(4) if i != L]
            q[sel, L] = missing[sel]
            for j, i in enumerate(others):
                q[sel, i] = dv[j][sel]
        for i in range(4):
            data["rot_%d" % i][:m] = q[:, i]
        for name in sh_names:
            data[name][:m] = (sh[name][:m] / 256.0 - 0.5) * 8.0
    return data, meta


def read(path):
    el = read_ply(path)
    return decode(el["chunk"], el["vertex"], el.get("sh"))


def sha(rows: np.ndarray) -> bytes:
    return hashlib.sha256(np.ascontiguousarray(rows).tobytes()).digest()


def scene_file(path, n, degree, seed, chunks=None, n_sh=None):
    """a synthetic file of n rows: random words, random finite bounds (min <= max), `chunks` chunk rows (default ceil(n / 256));
    the sh element has the degree's width, or `n_sh` properties (any width, 0 = no sh element) when that is given"""
    rng = np.random.default_rng(seed)
    nc = (n + 255) // 256 if chunks is None else chunks
    ch = np.zeros(nc, [(f, "<f4") for f in CHUNK_FIELDS])
    for group in (0, 6, 12):
        for k in range(3):
            lo, hi = CHUNK_FIELDS[group + k], CHUNK_FIELDS[group + 3 + k]
            a = (rng.standard_normal(nc) * 5).astype(np.float32)
            ch[lo] = a
            ch[hi] = a + np.abs(rng.standard_normal(nc) * 3).astype(np.float32)
    vt = np.zeros(n, [(f, "<u4") for f in VERTEX_FIELDS])
    for f in VERTEX_FIELDS:
        vt[f] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    els = [("chunk", ch), ("vertex", vt)]
    m = {0: 0, 1: 9, 2: 24, 3: 45}[degree] if n_sh is None else n_sh
    if m:
        sh = np.zeros(n, [("f_rest_%d" % i, "u1") for i in range(m)])
        raw = rng.integers(0, 256, (n, m), dtype=np.uint8)
        sh.view(np.uint8).reshape(n, m)[:] = raw
        els.append(("sh", sh))
    write_ply(path, els)
    return path


ROT_EDGE = (0, 1, 511, 512, 1022, 1023)
PATTERN_ROWS, PATTERN_SH = 4096, 45
# odd multipliers (so i * m runs through a slot's whole range), no two alike: position y, z | scale y, x | r g b a
PATTERN_MUL = {"pos": (5, 7), "scale": (11, 13), "colour": (1, 3, 5, 7)}


def pattern_tables():
    """(chunk, vertex, sh) of pattern_file: 4096 rows in 16 chunks.  Row i holds
      position  x = i mod 2048 (bits 21-31), y = 5 i mod 1024 (bits 11-20), z = 7 i mod 2048 (bits 0-10);
      scale     the same scheme from the other end: z = i mod 2048, y = 11 i mod 1024, x = 13 i mod 2048;
      colour    r = i, g = 3 i, b = 5 i, alpha = 7 i, each mod 256;
      rotation  combination i mod 864 of largest (4) x the edge codes 0, 1, 511, 512, 1022, 1023 in each 10-bit slot (6^3);
      sh        slot k = ((2 k + 1) i + k) mod 256, k < 45;
    every one of the 18 bounds of every chunk is a float32 of its own (min < max)."""
    n = PATTERN_ROWS
    i = np.arange(n, dtype=np.uint64)
    vt = np.zeros(n, [(f, "<u4") for f in VERTEX_FIELDS])
    a, b = PATTERN_MUL["pos"]
    vt["packed_position"] = ((i % 2048) << 21 | (i * a % 1024) << 11 | (i * b % 2048)).astype(np.uint32)
    a, b = PATTERN_MUL["scale"]
    vt["packed_scale"] = ((i * b % 2048) << 21 | (i * a % 1024) << 11 | (i % 2048)).astype(np.uint32)
    m = PATTERN_MUL["colour"]
    vt["packed_color"] = ((i * m[0] % 256) << 24 | (i * m[1] % 256) << 16 | (i * m[2] % 256) << 8 | (i * m[3] % 256)).astype(np.uint32)
    e = np.array(ROT_EDGE, np.uint64)
    c = i % (4 * 6 ** 3)
    vt["packed_rotation"] = ((c // 216) << 30 | e[c // 36 % 6] << 20 | e[c // 6 % 6] << 10 | e[c % 6]).astype(np.uint32)
    sh = np.zeros(n, [("f_rest_%d" % k, "u1") for k in range(PATTERN_SH)])
    for k in range(PATTERN_SH):
        sh["f_rest_%d" % k] = ((2 * k + 1) * i + k) % 256
    nc = n // 256
    ch = np.zeros(nc, [(f, "<f4") for f in CHUNK_FIELDS])
    for group in (0, 6, 12):
        for k in range(3):
            axis = group // 2 + k                                     # 0 .. 8
            lo = (-8.0 + 2.0 * axis + np.arange(nc) / 16.0).astype(np.float32)   # exact in float32, as is the width
            ch[CHUNK_FIELDS[group + k]] = lo
            ch[CHUNK_FIELDS[group + 3 + k]] = lo + np.float32(1.0 + (4 + axis) / 256.0)
    allb = np.stack([ch[f] for f in CHUNK_FIELDS])
    assert len(np.unique(allb)) == allb.size and all((ch[CHUNK_FIELDS[g + k]] < ch[CHUNK_FIELDS[g + 3 + k]]).all() for g in (0, 6, 12) for k in range(3))
    return ch, vt, sh


def pattern_file(path):
    ch, vt, sh = pattern_tables()
    write_ply(path, [("chunk", ch), ("vertex", vt), ("sh", sh)])
    return path
