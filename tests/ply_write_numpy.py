"""A numpy restatement of the reference's two PLY writers (gsconverter/formats/ply_3dgs.py:62-121, formats/ply_cc.py:64-132)
without plyfile, used by the host tests, the GPU tests and the golden generator: the reference's statements on the table -- the
same names in the same order, the same lookups, numpy's own `np.zeros` and `out[name] = data[name]` -- and the container as
plyfile lays it out (tests/ply_read_numpy.py: write_ply); the stand-in for plyfile under which the reference's own writers run;
and the builders of the test tables."""
import io
import os
import tempfile

import numpy as np

import ply_read_numpy as pn

FULL_STD = set(pn.get_standard_order(True)) | {"nx", "ny", "nz"}                   # ply_3dgs.py:98 / ply_cc.py:104


def last_idx_of(data, dialect):
    """ply_3dgs.py:71-76 (`!= 0`) / ply_cc.py:71-76 (truthiness)"""
    with np.errstate(all="ignore"):
        for i in range(44, -1, -1):
            f = "f_rest_%d" % i
            if f in data.dtype.names and (np.any(data[f] != 0) if dialect == "3dgs" else np.any(data[f])):
                return i
    return -1


def convert(data, dialect, crop_sh=False):
    """ply_3dgs.py:65-109 / ply_cc.py:67-116 -> (the vertex element's array, last_idx or None)"""
    names = data.dtype.names
    std_order = pn.get_standard_order(has_rgb="red" in names)
    last_idx = None
    if crop_sh:
        last_idx = last_idx_of(data, dialect)
        std_order = [n for n in std_order if not (n.startswith("f_rest_") and int(n.split("_")[-1]) > last_idx)]
    out_name = (lambda n: n if n in pn.CC_PLAIN else "scalar_" + n) if dialect == "cc" else (lambda n: n)
    listed, mapping = [], {}
    for n in std_order:
        if n in names:
            listed.append((out_name(n), data.dtype[n].str))
            mapping[n] = out_name(n)
        elif n.startswith("f_rest_"):
            if not crop_sh:
                listed.append((out_name(n), "f4"))
        elif n in ("nx", "ny", "nz"):
            listed.append((n, "f4"))
    for n in names:
        if n not in std_order and n not in FULL_STD:
            o = "scalar_" + n if dialect == "cc" else n
            listed.append((o, data.dtype[n].str))
            mapping[n] = o
    out = np.zeros(len(data), dtype=np.dtype(listed))
    for n, o in mapping.items():
        out[o] = data[n]
    return out, last_idx


def file_bytes(elements):
    """[(name, array)] -> the bytes of the binary little-endian PLY that holds them (pn.write_ply)"""
    fd, path = tempfile.mkstemp(suffix=".ply")
    os.close(fd)
    try:
        pn.write_ply(path, elements)
        with open(path, "rb") as f:
            return f.read()
    finally:
        os.unlink(path)


def write(data, dialect, crop_sh=False, extra_elements=()):
    """-> (output dtype, the vertex rows' bytes, the file's bytes, last_idx or None)"""
    vertex, last_idx = convert(data, dialect, crop_sh)
    blob = file_bytes([("vertex", vertex)] + [(e.name, e.data) for e in extra_elements])
    return vertex.dtype, vertex.tobytes(), blob, last_idx


def properties(dtype):
    """-> [[property type, name]] as the header lists them"""
    return [[pn.NAMES[dtype[n].str[1:]], n] for n in dtype.names]


# ---------------------------------------------------------------------------------------------------------- plyfile's stand-in

class StandInElement:
    """PlyElement.describe(data, name): keeps the array"""

    def __init__(self, data, name):
        self.data, self.name = data, name

    @staticmethod
    def describe(data, name):
        return StandInElement(data, name)


class StandInPlyData:
    """PlyData(elements, byte_order='<').write(path): serialises with ply_read_numpy.write_ply"""

    def __init__(self, elements, text=False, byte_order="<"):
        assert byte_order == "<" and not text
        self.elements = list(elements)

    def write(self, path):
        pn.write_ply(path, [(e.name, e.data) for e in self.elements])


class Extra:
    """an extra element as the writers take it: .name and .data"""

    def __init__(self, name, data):
        self.name, self.data = name, data


# ---------------------------------------------------------------------------------------------------------- tables and their storage

def dtype_descr(dtype):
    """a structured dtype (holes and field order included) -> a JSON-able description; dtype_from() is its inverse"""
    return {"names": list(dtype.names), "formats": [dtype[n].str for n in dtype.names], "offsets": [int(dtype.fields[n][1]) for n in dtype.names],
            "itemsize": int(dtype.itemsize)}


def dtype_from(descr):
    return np.dtype({"names": descr["names"], "formats": descr["formats"], "offsets": descr["offsets"], "itemsize": descr["itemsize"]})


def table_bytes(data):
    """the table whole: every byte of every row, holes included"""
    c = np.ascontiguousarray(data)
    return np.frombuffer(c.tobytes() if c.dtype.itemsize == 0 else c.view(np.uint8).reshape(-1).tobytes(), np.uint8).copy()


def table_from(blob, descr, rows):
    return np.frombuffer(bytes(blob), dtype_from(descr), rows).copy()


class Case:
    """one golden case: the table as the writer gets it (a view where the case says so), the kwargs, and per dialect what the
    reference wrote"""

    def __init__(self, name, rec, g):
        self.name, self.rec = name, rec
        base = table_from(g[name + "__table"], rec["dtype"], rec["base_rows"])
        self.table = base[::rec["step"]] if rec["step"] != 1 else base
        self.crop_sh = bool(rec["kwargs"].get("crop_sh", False))
        self.extras = [Extra(e["name"], table_from(g["%s__extra%d" % (name, k)], e["dtype"], e["rows"])) for k, e in enumerate(rec["extra_elements"])]
        self.kwargs = dict(rec["kwargs"], extra_elements=self.extras) if self.extras else dict(rec["kwargs"])
        self.writers = rec["writers"]
        self.files = {d: g["%s__%s__file" % (name, d)].tobytes() for d in rec["writers"]}

    def vertex_rows(self, dialect):
        """the vertex element's body inside the expected file"""
        blob = self.files[dialect]
        start = blob.index(b"end_header\n") + len(b"end_header\n")
        return blob[start:start + len(self.table) * self.writers[dialect]["itemsize"]]


def load_cases(path):
    """the golden file -> {name: Case}"""
    import json
    g = np.load(path)
    spec = json.loads(bytes(g["spec"]).decode())
    return {name: Case(name, rec, g) for name, rec in spec.items()}


def npz_bytes(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getvalue()
