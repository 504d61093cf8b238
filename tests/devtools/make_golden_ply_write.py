"""Build tests/golden/ply_write_ref.npz from the REFERENCE's own PLY writers (build box only: needs the reference).

The reference's ``Ply3DGSFormat.write`` (formats/ply_3dgs.py:62-121) and ``PlyCCFormat.write`` (formats/ply_cc.py:64-132) run
unchanged; only ``plyfile`` (not installed here) is a stand-in (tests/ply_write_numpy.py): ``PlyElement.describe(data, name)``
keeps the array, ``PlyData(elements, byte_order='<').write(path)`` serialises with tests/ply_read_numpy.py's write_ply.

  the reference's   the output dtype (which fields, their order, names and types), which columns are padded with zeros or
                    dropped, the answer of the crop_sh scan, and every byte of every row
  the stand-in's    the header's text, namely the layout plyfile gives -- `ply` / `format binary_little_endian 1.0` /
                    `element <name> <count>` / `property <type> <name>` / `end_header` -- which the project already relies on
                    where it writes a compressed PLY without plyfile (formats/ply_container.py), and the byte swap of a
                    big-endian extra element on its way out

Per case the input table is stored whole (every byte of every row, holes included, plus its dtype's description and the slice
step a test applies), the kwargs, the extra elements; per case and dialect the expected file whole, the expected property list
and -- under crop_sh -- the last_idx the reference's loop found (read back from the f_rest properties it kept).

    python tests/devtools/make_golden_ply_write.py
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ply_read_numpy as pn  # noqa: E402
import ply_write_numpy as pw  # noqa: E402
from oracle import refload  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ply_write_ref.npz")
BOTH = ("3dgs", "cc")
REST = ["f_rest_%d" % i for i in range(45)]


def reference_write(data, path, dialect, kwargs):
    stub = types.ModuleType("plyfile")
    stub.PlyData = pw.StandInPlyData
    stub.PlyElement = pw.StandInElement
    sys.modules["plyfile"] = stub
    refload.load()
    if dialect == "3dgs":
        import gsconverter.formats.ply_3dgs as mod  # type: ignore
        fmt = mod.Ply3DGSFormat()
    else:
        import gsconverter.formats.ply_cc as mod  # type: ignore
        fmt = mod.PlyCCFormat()
    mod.PlyData, mod.PlyElement = pw.StandInPlyData, pw.StandInElement     # (the module may have been imported under another stub)
    import contextlib
    import io
    with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        fmt.write(data, path, **kwargs)
    with open(path, "rb") as f:
        return f.read()


def build(n, fields, rng):
    """fields: [(name, type str)] -> n rows: floats multiples of 1/4 in +-25 and never zero (they compress, and no f_rest column
    is zero by accident), integers random over their range"""
    t = np.zeros(n, [(f, ("<" + ty) if ty[1] != "1" else ty) for f, ty in fields])
    for f, ty in fields:
        if ty[0] == "f":
            v = rng.integers(1, 100, n) * rng.choice([-1, 1], n)
            t[f] = (v / 4.0).astype(ty)
        else:
            info = np.iinfo(ty)
            t[f] = rng.integers(info.min, int(info.max) + 1, n, dtype=np.int64).astype(ty)
    return t


def crop_table(n, rng, last_idx, how):
    """a degree-3 table whose f_rest_j, j > last_idx, hold nothing that counts, and whose f_rest_{last_idx} holds the deciding
    value in the form `how`"""
    t = build(n, pn.canonical_fields(3), rng)
    for j in range(last_idx + 1, 45):
        t[REST[j]] = 0
    if last_idx < 0:
        t["f_rest_0"] = -0.0                                   # -0.0 does not count: nothing is left
        return t
    f = REST[last_idx]
    if how == "row0":                                          # the only value that counts in the whole of f_rest sits in row 0
        for j in range(45):
            t[REST[j]] = 0
        t[f][0] = 1.5
    elif how == "last_row":                                    # ... in the last row of a partial last tile
        t[f] = 0
        t[f][n - 1] = -2.25
    elif how == "nan":
        t[f] = 0
        t[f][n // 2] = np.float32(np.nan)
    elif how == "denormal":
        t[f] = 0
        t[f].view(np.uint32)[n // 3] = 0x00000001
    elif how == "minus_zero_above":                            # f_rest_{last_idx + 1} holds -0.0 and nothing else: it falls through
        t[REST[last_idx + 1]] = -0.0
    else:
        assert how == "plain"
    return t


def cases():
    """-> [(name, table (possibly a view), step, kwargs, extra elements)]"""
    rng = np.random.default_rng(20261019)
    out = []

    def add(name, table, step=1, crop=False, extras=()):
        out.append((name, table, step, {"crop_sh": True} if crop else {}, list(extras)))

    rgb = [(c, "u1") for c in pn.COLOURS]
    add("canonical_deg3", build(300, pn.canonical_fields(3), rng))
    add("canonical_rgb", build(129, pn.canonical_fields(3) + rgb, rng))
    add("rgb_no_normals", build(128, [f for f in pn.canonical_fields(3) if f[0] not in ("nx", "ny", "nz")] + rgb, rng))
    add("rgb_crop_8", _with_rgb(crop_table(65, rng, 8, "plain"), rng), crop=True)
    for deg, n in ((0, 63), (1, 64), (2, 65)):
        add("deg%d" % deg, build(n, pn.canonical_fields(deg), rng))
    for deg, n in ((0, 127), (1, 128), (2, 129)):
        add("deg%d_crop" % deg, build(n, pn.canonical_fields(deg), rng), crop=True)
    add("no_normals", build(65, [f for f in pn.canonical_fields(3) if f[0] not in ("nx", "ny", "nz")], rng))
    wide = build(127, [("pad_a", "u1")] + pn.canonical_fields(1) + [("junk", "f8"), ("label", "i2"), ("pad_b", "u1")], rng)
    add("holes", wide[[f for f, _ in pn.canonical_fields(1)] + ["label"]])
    fields = pn.canonical_fields(2) + rgb + [("conf", "f4")]
    add("shuffled", build(128, [fields[i] for i in rng.permutation(len(fields))], rng))
    add("noncontiguous", build(258, pn.canonical_fields(1) + rgb, rng), step=2)
    types8 = [("e_" + t, t) for t in pn.SOURCE_TYPES]
    add("extras", build(64, [types8[0]] + pn.canonical_fields(0) + types8[1:], rng))
    add("extras_crop", build(63, [types8[0]] + pn.canonical_fields(1) + types8[1:], rng), crop=True)
    add("red_without_green", build(1, pn.canonical_fields(0) + [("red", "u1"), ("blue", "u1")], rng))
    add("green_without_red", build(63, pn.canonical_fields(0) + [("green", "u1")], rng))
    add("no_opacity", build(64, [f for f in pn.canonical_fields(1) if f[0] != "opacity"], rng))
    f8 = [(f, "f8" if f == "f_rest_3" else t) for f, t in pn.canonical_fields(1)]
    add("f8_rest_3", build(63, f8, rng))
    t = build(65, f8, rng)
    for j in range(4, 9):
        t[REST[j]] = 0
    add("f8_rest_3_crop", t, crop=True)
    add("zero_rows", build(0, pn.canonical_fields(2), rng))
    add("zero_rows_crop", build(0, pn.canonical_fields(2), rng), crop=True)
    camera = build(3, [("fx", "f4"), ("fy", "f8"), ("id", "i4"), ("flag", "u1")], rng)
    big = np.empty(3, np.dtype([("fx", ">f4"), ("fy", ">f8"), ("id", ">i4"), ("flag", "u1")]))
    for f in camera.dtype.names:
        big[f] = camera[f]
    empty = build(0, [("a", "u2"), ("b", "f4")], rng)
    add("extra_elements", build(1, pn.canonical_fields(1), rng), extras=[pw.Extra("camera", big), pw.Extra("empty", empty)])
    add("extra_elements_zero_rows", build(0, pn.canonical_fields(0), rng), crop=True, extras=[pw.Extra("camera", camera)])
    for last_idx, n, how in ((-1, 64, "plain"), (0, 129, "row0"), (5, 300, "last_row"), (8, 127, "minus_zero_above"), (9, 65, "nan"),
                             (23, 128, "denormal"), (24, 63, "plain"), (44, 1, "plain")):
        add("crop_last_%s" % ("m1" if last_idx < 0 else last_idx), crop_table(n, rng, last_idx, how), crop=True)
    return out


def _with_rgb(t, rng):
    """the table widened by red green blue (251-byte rows)"""
    out = np.zeros(len(t), t.dtype.descr + [(c, "u1") for c in pn.COLOURS])
    for f in t.dtype.names:
        out[f] = t[f]
    for c in pn.COLOURS:
        out[c] = rng.integers(0, 256, len(t)).astype("u1")
    return out


def found_last_idx(prop_names):
    """the last_idx the reference's loop found, read from the f_rest properties it kept (crop_sh: nothing is padded)"""
    kept = [int(n.rsplit("_", 1)[1]) for n in prop_names if "f_rest_" in n]
    return max(kept) if kept else -1


def main():
    spec, arrays = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, base, step, kwargs, extras in cases():
            table = base[::step] if step != 1 else base
            arrays[name + "__table"] = pw.table_bytes(base)
            rec = {"rows": len(table), "base_rows": len(base), "step": step, "dtype": pw.dtype_descr(base.dtype), "kwargs": kwargs,
                   "extra_elements": [{"name": e.name, "rows": len(e.data), "dtype": pw.dtype_descr(e.data.dtype)} for e in extras], "writers": {}}
            for k, e in enumerate(extras):
                arrays["%s__extra%d" % (name, k)] = pw.table_bytes(e.data)
            assert rec["rows"] <= 300, name
            for dialect in BOTH:
                kw = dict(kwargs, extra_elements=extras) if extras else dict(kwargs)
                blob = reference_write(table, os.path.join(tmp, "%s_%s.ply" % (name, dialect)), dialect, kw)
                dtype, rows, mine, last_idx = pw.write(table, dialect, bool(kwargs.get("crop_sh")), extras)
                assert mine == blob, (name, dialect)
                props = pw.properties(dtype)
                w = {"properties": props, "itemsize": dtype.itemsize, "file_bytes": len(blob)}
                if kwargs.get("crop_sh"):
                    w["last_idx"] = last_idx
                    if any(n.startswith("f_rest_") for n in table.dtype.names):
                        assert found_last_idx([p[1] for p in props]) == last_idx, (name, dialect)     # the reference's own answer
                rec["writers"][dialect] = w
                arrays["%s__%s__file" % (name, dialect)] = np.frombuffer(blob, np.uint8)
            spec[name] = rec
            print(name, rec["rows"], "rows", {d: "%d bytes a row, %d properties%s" % (w["itemsize"], len(w["properties"]),
                                                                                     ", last_idx %d" % w["last_idx"] if "last_idx" in w else "")
                                             for d, w in rec["writers"].items()})
    arrays["spec"] = np.frombuffer(json.dumps(spec, sort_keys=True).encode(), np.uint8)
    blob = pw.npz_bytes(arrays)
    assert len(blob) < 1_000_000
    with open(OUT, "wb") as f:
        f.write(blob)
    print(OUT, len(blob), "bytes")


if __name__ == "__main__":
    main()
