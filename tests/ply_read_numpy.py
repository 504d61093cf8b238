"""A numpy restatement of the reference's two PLY readers (gsconverter/formats/ply_3dgs.py:8-60, formats/ply_cc.py:8-62) without
plyfile, used by the host tests, the GPU tests and the golden generator: a parser of the binary PLY container that yields every
element as a structured array in the FILE's byte order (what plyfile hands the reference), the reference's statements on it --
the same names, the same lookups in the same order, numpy's own `dst[field] = src[field]` -- and the builders of the test
files (edge values per source type, layouts, header padding)."""
import numpy as np

TYPES = {"char": "i1", "uchar": "u1", "short": "i2", "ushort": "u2", "int": "i4", "uint": "u4", "float": "f4", "double": "f8",
         "int8": "i1", "uint8": "u1", "int16": "i2", "uint16": "u2", "int32": "i4", "uint32": "u4", "float32": "f4", "float64": "f8"}
NAMES = {"i1": "char", "u1": "uchar", "i2": "short", "u2": "ushort", "i4": "int", "u4": "uint", "f4": "float", "f8": "double"}
SOURCE_TYPES = ["i1", "u1", "i2", "u2", "i4", "u4", "f4", "f8"]
FLOAT_FIELDS = (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + ["f_rest_%d" % i for i in range(45)]
                + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"])     # structures.py:10-17
COLOURS = ["red", "green", "blue"]
CC_PLAIN = {"x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"}                                    # ply_cc.py:86


# ---------------------------------------------------------------------------------------------------------- the container

def header_text(elements, fmt="binary_little_endian", body_mod16=None):
    """elements: [(name, count, [(property, type str)])] -> the header's bytes; body_mod16: comment padding so that the body
    starts at a file offset congruent to it mod 16"""
    head = ["ply", "format %s 1.0" % fmt]
    for name, count, props in elements:
        head.append("element %s %d" % (name, count))
        for p, t in props:
            head.append("property %s %s" % (NAMES[t], p))
    tail = "end_header\n"
    text = "\n".join(head) + "\n"
    if body_mod16 is not None:
        pad = (body_mod16 - (len(text) + len(tail) + len("comment \n"))) % 16
        text += "comment " + "p" * pad + "\n"
    return (text + tail).encode("ascii")


def write_ply(path, elements, fmt="binary_little_endian", body_mod16=None):
    """elements: [(name, structured array)] -> a PLY file of scalar properties in the byte order `fmt` names"""
    order = ">" if fmt == "binary_big_endian" else "<"
    spec = [(name, len(arr), [(f, arr.dtype[f].str[1:]) for f in arr.dtype.names]) for name, arr in elements]
    with open(path, "wb") as f:
        f.write(header_text(spec, fmt, body_mod16))
        for _, arr in elements:
            dt = np.dtype([(n, order + arr.dtype[n].str[1:]) for n in arr.dtype.names])
            out = np.empty(len(arr), dt)
            for n in arr.dtype.names:
                out[n] = arr[n]
            f.write(out.tobytes())
    return path


def parse(path):
    """a binary PLY of scalar properties -> [(element name, structured array in the file's byte order)] in header order"""
    with open(path, "rb") as f:
        raw = f.read()
    if not raw.startswith(b"ply"):
        raise ValueError("not a PLY file")
    end = raw.index(b"end_header") + len(b"end_header")
    end = raw.index(b"\n", end) + 1
    elements, order = [], None
    for line in raw[:end].decode("ascii").splitlines():
        w = line.split()
        if not w or w[0] in ("comment", "obj_info", "ply", "end_header"):
            continue
        if w[0] == "format":
            order = {"binary_little_endian": "<", "binary_big_endian": ">"}[w[1]]
        elif w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property":
            assert w[1] != "list", line
            elements[-1][2].append((w[2], order + TYPES[w[1]] if TYPES[w[1]][1] != "1" else "|" + TYPES[w[1]]))
    out, pos = [], end
    for name, count, props in elements:
        dt = np.dtype(props)
        if pos + dt.itemsize * count > len(raw):
            raise ValueError("early end of file in element %r" % name)
        out.append((name, np.frombuffer(raw, dt, count, pos).copy()))
        pos += dt.itemsize * count
    return out


class Element:
    def __init__(self, name, data):
        self.name, self.data = name, data


class PlyData:
    """what the reference's readers use of plyfile.PlyData: `name in plydata`, `plydata.elements` (objects with .name) and
    `plydata[name].data`"""

    def __init__(self, elements):
        self.elements = [Element(n, d) for n, d in elements]

    def __contains__(self, name):
        return any(e.name == name for e in self.elements)

    def __getitem__(self, name):
        return next(e for e in self.elements if e.name == name)

    @staticmethod
    def read(path):
        return PlyData(parse(path))


# ---------------------------------------------------------------------------------------------------------- the readers

def get_standard_order(has_rgb=False):
    return FLOAT_FIELDS + COLOURS if has_rgb else list(FLOAT_FIELDS)


def define_dtype(has_rgb, extra_fields):
    """structures.py:23-59 at has_scal=False, sh_degree=3"""
    dtype = [(f, "f4") for f in FLOAT_FIELDS]
    if has_rgb:
        dtype.extend([(f, "u1") for f in COLOURS])
    for name, typ in extra_fields:
        if not any(d[0] == name for d in dtype):
            dtype.append((name, typ))
    return dtype


def convert(vertices, dialect):
    """ply_3dgs.py:18-60 / ply_cc.py:18-62 on the vertex element's array"""
    source_names = vertices.dtype.names
    source_prefix = ""
    if dialect == "3dgs":
        if "scalar_f_dc_0" in source_names:
            source_prefix = "scalar_"
            if "scalar_scal_f_dc_0" in source_names:
                source_prefix = "scalar_scal_"
        elif "scal_f_dc_0" in source_names:
            source_prefix = "scal_"
    else:
        if "scalar_f_dc_0" in source_names:
            source_prefix = "scalar_"
        elif "scalar_scal_f_dc_0" in source_names:
            source_prefix = "scalar_scal_"
    std_base_names = get_standard_order(has_rgb=True)
    std_source_names = {source_prefix + name for name in std_base_names} | set(std_base_names)
    extra_fields = []
    for name in source_names:
        if name not in std_source_names:
            internal = name[7:] if dialect == "cc" and name.startswith("scalar_") else name
            extra_fields.append((internal, vertices.dtype[name].str))
    has_rgb = "red" in source_names
    internal_dtype = define_dtype(has_rgb, extra_fields)
    converted = np.zeros(len(vertices), dtype=internal_dtype)
    with np.errstate(all="ignore"):
        for target, _ in internal_dtype:
            if target in source_names:
                converted[target] = vertices[target]
            elif source_prefix + target in source_names:
                converted[target] = vertices[source_prefix + target]
            elif dialect == "cc" and "scalar_" + target in source_names:
                converted[target] = vertices["scalar_" + target]
    return converted


def read(path, dialect):
    """-> (rows, [(name, array)] of the other elements)"""
    elements = parse(path)
    if not any(n == "vertex" for n, _ in elements):
        raise ValueError("PLY file does not contain 'vertex' element")
    rows = convert(next(d for n, d in elements if n == "vertex"), dialect)
    return rows, [(n, d) for n, d in elements if n != "vertex"]


# ---------------------------------------------------------------------------------------------------------- test files

def _f64(bits):
    return np.array(bits, np.uint64).view(np.float64)


def edge_values(typ, n=256, seed=0):
    """`n` values of source type `typ` with the edges the conversion to float32 can get wrong, the rest random bit patterns"""
    rng = np.random.default_rng([seed, SOURCE_TYPES.index(typ)])
    if typ in ("i1", "u1"):
        return (np.arange(n) % 256).astype(np.uint8).view(typ)
    if typ in ("i2", "u2"):
        v = rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint16)
        v[:8] = [0, 1, 0x7fff, 0x8000, 0x8001, 0xffff, 0xfffe, 0x00ff]
        return v.view(typ)
    if typ in ("i4", "u4"):
        v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        e = [0, 1, 0xffffffff, 0x7fffffff, 0x80000000, 0x80000001, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 2, (1 << 24) + 3,
             (1 << 25) + 1, (1 << 25) + 2, (1 << 25) + 3, (1 << 25) + 6, (1 << 31) + 128, (1 << 31) + 384, (1 << 31) + 129, (1 << 32) - 128,
             (1 << 32) - 129, (1 << 32) - 127, 0x7fffffc0, 0x7fffffbf, 0x7fffffc1, (1 << 30) + 64, (1 << 30) + 192]
        e += [(-x) & 0xffffffff for x in ((1 << 24) + 1, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6, 1, (1 << 31) - 64)]
        v[:len(e)] = e
        return v.view(typ)
    if typ == "f4":
        v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        e = [0, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fa00123, 0x00000001, 0x80000001,
             0x007fffff, 0x00800000, 0x7f7fffff, 0xff7fffff, 0x3f800000]
        v[:len(e)] = e
        return v.view("f4")
    assert typ == "f8"
    v = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    # half of the random patterns inside float32's exponent range, a quarter in its subnormal range
    k = np.arange(n)
    ex = np.where(k % 4 < 2, rng.integers(897, 1151, n), rng.integers(1023 - 155, 1023 - 124, n)).astype(np.uint64)
    sel = k % 4 != 3
    v[sel] = (v[sel] & np.uint64(0x800fffffffffffff)) | (ex[sel] << np.uint64(52))
    tie = k % 8 == 1                                        # exact halfway points at 24 bits, with the even / odd bit random
    v[tie] = (v[tie] & ~np.uint64((1 << 29) - 1)) | np.uint64(1 << 28)
    flt_max = 0x47efffffe0000000
    half_above = 0x47effffff0000000                          # FLT_MAX + half an ulp: the tie that rounds to inf
    e = [0, 1 << 63, 0x7ff0000000000000, 0xfff0000000000000,
         0x7ff8000000000000, 0xfff8000000000000,              # quiet NaNs
         0x7ff8000000000001, 0xfff8000000000001,              # ... payload in the low bits only
         0x7ffc000020000000, 0xfffc0000e0000000,              # ... payload in the high bits
         0x7ff0000000000001, 0xfff0000000000001,              # signalling NaNs, payload in the low bits only
         0x7ff4000000000000, 0xfff4000000000000,              # ... in the high bits
         0x7ff0000020000000, 0xfff7ffffffffffff, 0x7ff0000010000000,
         flt_max, flt_max | (1 << 63), half_above, half_above | (1 << 63), half_above - 1, half_above + 1, (half_above + 1) | (1 << 63),
         0x47f0000000000000, 0x7fefffffffffffff, 0xffefffffffffffff,                       # 2^128, +-DBL_MAX
         0x3ff0000010000000, 0x3ff0000010000001, 0x3ff000000fffffff,                       # 1 + 2^-24: tie to even (down), above, below
         0x3ff0000030000000, 0x3ff0000030000001, 0x3ff000002fffffff,                       # 1 + 3 2^-24: tie to even (up)
         0x3fefffffffffffff, 0x3feffffff0000000, 0x3fefffffefffffff,                       # just below 1
         0x3810000000000000, 0xb810000000000000,                                           # 2^-126
         0x380fffffffffffff, 0x380ffffff0000000, 0x380fffffe0000000, 0x380fffffefffffff,   # below it: round up to it / largest subnormal
         0x3800000000000000, 0x37f0000000000000,                                           # 2^-127, 2^-128
         0x36a0000000000000, 0xb6a0000000000000,                                           # 2^-149
         0x3690000000000000, 0x3690000000000001, 0xb690000000000001, 0x368fffffffffffff,   # 2^-150 (tie to 0), its successor, below
         0x3680000000000000, 0xb680000000000000,                                           # 2^-151
         0x36a8000000000000, 0x36a8000000000001, 0x36b4000000000000, 0x36b4000000000001,   # 1.5 and 2.5 x 2^-149: ties
         0x36b3ffffffffffff, 0x36c2000000000000,
         0x0000000000000001, 0x8000000000000001, 0x000fffffffffffff, 0x0010000000000000]   # float64 subnormals, DBL_MIN
    v[:len(e)] = np.array(e, np.uint64)
    return v.view("f8")


def float_table(n, rng, names=FLOAT_FIELDS, typ="f4"):
    """n rows of float fields `names`, random finite values"""
    t = np.zeros(n, [(f, "<" + typ) for f in names])
    for f in names:
        t[f] = (rng.standard_normal(n) * 3).astype(typ)
    return t


def build(n, fields, rng):
    """fields: [(name, type str)] -> a structured array of n rows: floats random normal, integers random over their range"""
    t = np.zeros(n, [(f, ("<" + ty) if ty[1] != "1" else ty) for f, ty in fields])
    for f, ty in fields:
        if ty[0] == "f":
            t[f] = (rng.standard_normal(n) * 3).astype(ty)
        else:
            info = np.iinfo(ty)
            t[f] = rng.integers(info.min, int(info.max) + 1, n, dtype=np.int64).astype(ty)
    return t


def canonical_fields(degree=3, typ="f4"):
    """the trainer's layout: x y z nx ny nz f_dc f_rest(degree) opacity scale rot"""
    n_rest = 3 * ((degree + 1) ** 2 - 1)
    return [(f, typ) for f in FLOAT_FIELDS if not f.startswith("f_rest_") or int(f[7:]) < n_rest]


def cc_fields(degree=3, rgb=True, extras=(("scalar_confidence", "f4"), ("scalar_label", "i4"))):
    """CloudCompare's own layout (ply_cc.py:83-109): x y z, the colours as uchar, nx ny nz, scalar_* fields, scalar_ extras"""
    out = [(f, "f4") for f in ("x", "y", "z")] + ([(c, "u1") for c in COLOURS] if rgb else []) + [(f, "f4") for f in ("nx", "ny", "nz")]
    out += [("scalar_" + f, t) for f, t in canonical_fields(degree) if f not in CC_PLAIN]
    return out + list(extras)


def type_matrix_table(typ, n=256):
    """every standard float field of source type `typ`, field k holding edge_values(typ) rolled by k rows"""
    ev = edge_values(typ, n)
    t = np.zeros(n, [(f, ("<" + typ) if typ[1] != "1" else typ) for f in FLOAT_FIELDS])
    for k, f in enumerate(FLOAT_FIELDS):
        t[f] = np.roll(ev, k)
    return t


def random_layout(seed, n=1000):
    """-> (structured array, dialect): shuffled property order, random types on the standard fields, random missing fields,
    0 ... 4 extras, a random prefix, the dialect at random.  A prefix the dialect does not detect turns every prefixed field
    into an extra; a draw whose rows would pass 512 bytes is drawn again without 8-byte types."""
    rng = np.random.default_rng(seed)
    dialect = ("3dgs", "cc")[int(rng.integers(2))]
    prefix = ["", "scalar_", "scal_", "scalar_scal_"][int(rng.integers(4))]
    for attempt in range(8):
        types = SOURCE_TYPES if attempt == 0 else SOURCE_TYPES[:7]
        fields = []
        for f in FLOAT_FIELDS:
            if rng.random() < 0.12 and f != "f_dc_0":
                continue
            ty = types[int(rng.integers(len(types)))] if rng.random() < 0.5 else "f4"
            name = f if (f in CC_PLAIN or (rng.random() < 0.15 and f != "f_dc_0")) else prefix + f
            fields.append((name, ty))
        if rng.random() < 0.6:
            fields += [(c, "u1") for c in COLOURS if c == "red" or rng.random() < 0.8]
        for i in range(int(rng.integers(5))):
            fields.append((("scalar_" if rng.random() < 0.5 else "") + "extra%d" % i, types[int(rng.integers(len(types)))]))
        fields = [fields[i] for i in rng.permutation(len(fields))]
        table = build(0, fields, rng)
        if table.dtype.itemsize <= 512 and convert(table, dialect).dtype.itemsize <= 512:
            return build(n, fields, rng), dialect
    raise AssertionError("random_layout(%r): no draw within 512 bytes" % (seed,))
