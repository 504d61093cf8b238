"""Build tests/golden/ply_read_ref.npz from the REFERENCE's own PLY readers (build box only: needs the reference).

The reference's ``Ply3DGSFormat.read`` (formats/ply_3dgs.py:8-60) and ``PlyCCFormat.read`` (formats/ply_cc.py:8-62) run unchanged;
only ``plyfile`` (not installed here) is a stub whose ``PlyData.read`` is the numpy parser of tests/ply_read_numpy.py: every
element as a structured array in the file's byte order, which is what plyfile hands the reference.  The input files are stored
whole, the reference's rows whole; per case and reader the spec records names, dtype strings, itemsize and rows, or the
exception's type and message.

    python tests/devtools/make_golden_ply_read.py
"""
import hashlib
import io
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ply_read_numpy as pn  # noqa: E402
from oracle import refload  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ply_read_ref.npz")
BOTH = ("3dgs", "cc")


def reference_read(path, dialect):
    stub = types.ModuleType("plyfile")
    stub.PlyData = pn.PlyData
    stub.PlyElement = object
    sys.modules["plyfile"] = stub
    refload.load()
    if dialect == "3dgs":
        import gsconverter.formats.ply_3dgs as mod  # type: ignore
        fmt = mod.Ply3DGSFormat()
    else:
        import gsconverter.formats.ply_cc as mod  # type: ignore
        fmt = mod.PlyCCFormat()
    try:
        with np.errstate(all="ignore"):
            rows = fmt.read(path)
    except Exception as e:  # noqa: BLE001 -- the reference's own error is the expected result
        return None, None, {"type": type(e).__name__, "message": str(e)}
    return rows, [el.name for el in fmt.extra_elements], None


def cases(tmp):
    """-> [(name, path, readers)]"""
    rng = np.random.default_rng(20261020)
    out = []

    def add(name, elements, readers=BOTH, fmt="binary_little_endian"):
        out.append((name, pn.write_ply(os.path.join(tmp, name + ".ply"), elements, fmt), readers))

    def prefixed(prefix, degree=2, n=20, plain=pn.CC_PLAIN):      # degree 2: padded, so no reader finds its rows in the file as they are
        return pn.build(n, [(f if f in plain else prefix + f, t) for f, t in pn.canonical_fields(degree)], rng)

    add("canonical_deg3", [("vertex", pn.build(60, pn.canonical_fields(3), rng))])
    for deg in (0, 1, 2):
        add("deg%d" % deg, [("vertex", pn.build(33, pn.canonical_fields(deg), rng))], ("3dgs",))
    add("cc_layout", [("vertex", pn.build(40, pn.cc_fields(3), rng))])
    add("prefix_scal", [("vertex", prefixed("scal_"))])
    add("prefix_scalar_scal", [("vertex", prefixed("scalar_scal_"))])
    nested = prefixed("scalar_scal_")
    add("prefix_scalar_scal_nested", [("vertex", pn.build(20, [(f, nested.dtype[f].str[1:]) for f in nested.dtype.names] + [("scalar_f_dc_0", "f4")], rng))])
    both = pn.cc_fields(3, rgb=False, extras=())
    add("opacity_and_scalar_opacity", [("vertex", pn.build(20, both[:7] + [("opacity", "f4")] + both[7:], rng))])
    add("red_without_green", [("vertex", pn.build(20, pn.canonical_fields(3) + [("red", "u1"), ("blue", "u1")], rng))])
    add("missing_rot_3", [("vertex", pn.build(20, pn.canonical_fields(3)[:-1], rng))])
    camera = pn.build(3, [("fx", "f4"), ("fy", "f8"), ("id", "i4"), ("flag", "u1")], rng)
    add("camera_before_vertex", [("camera", camera), ("vertex", pn.build(20, pn.canonical_fields(1), rng))])
    add("no_vertex", [("camera", camera)])
    add("zero_vertices", [("vertex", pn.build(0, pn.cc_fields(3), rng)), ("camera", camera)])
    fields = pn.cc_fields(3)
    add("shuffled", [("vertex", pn.build(20, [fields[i] for i in rng.permutation(len(fields))], rng))])
    mixed = [(f, pn.SOURCE_TYPES[k % 8]) for k, (f, _) in enumerate(pn.canonical_fields(3))]
    add("every_source_type", [("vertex", pn.build(40, mixed, rng))])
    add("big_endian", [("vertex", pn.build(40, mixed + [(c, "u1") for c in pn.COLOURS], rng))], fmt="binary_big_endian")
    add("extras_of_every_type", [("vertex", pn.build(20, pn.cc_fields(0, extras=[("scalar_e_" + t, t) for t in pn.SOURCE_TYPES]), rng))])
    # prefix "": scalar_opacity (f8) and scalar_x are extras whose stripped names are standard fields (define_dtype drops them);
    # the CC reader's third lookup then reads scalar_opacity into `opacity`, and `x` keeps its direct source
    plain = [(f, t) for f, t in pn.canonical_fields(3) if f != "opacity"]
    add("cc_extra_collides", [("vertex", pn.build(20, plain + [("scalar_opacity", "f8"), ("scalar_x", "f4"), ("scalar_keep", "i2")], rng))])
    return out


def main():
    import tempfile
    spec, arrays = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, path, readers in cases(tmp):
            with open(path, "rb") as f:
                data = f.read()
            arrays[name + "__file"] = np.frombuffer(data, np.uint8)
            rec = {"file_bytes": len(data), "file_sha256": hashlib.sha256(data).hexdigest(), "readers": {}}
            for dialect in readers:
                rows, extra_names, err = reference_read(path, dialect)
                if err is not None:
                    rec["readers"][dialect] = {"error": err}
                    continue
                assert len(rows) <= 300, name
                rec["readers"][dialect] = {"names": list(rows.dtype.names), "dtype": [rows.dtype[f].str for f in rows.dtype.names],
                                           "itemsize": rows.dtype.itemsize, "rows": len(rows), "extra_elements": extra_names}
                arrays["%s__%s__rows" % (name, dialect)] = np.ascontiguousarray(rows).view(np.uint8).reshape(-1).copy()
                mine, others = pn.read(path, dialect)
                assert mine.dtype == rows.dtype and mine.tobytes() == rows.tobytes() and [n for n, _ in others] == extra_names, (name, dialect)
            spec[name] = rec
            print(name, {d: r.get("error", {}).get("type") or "%d rows x %d bytes" % (r["rows"], r["itemsize"]) for d, r in rec["readers"].items()})
    arrays["spec"] = np.frombuffer(json.dumps(spec, sort_keys=True).encode(), np.uint8)
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    assert len(buf.getvalue()) < 1_000_000
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print(OUT, len(buf.getvalue()), "bytes")


if __name__ == "__main__":
    main()
