"""Build tests/golden/ply_text_ref.npz from the REFERENCE's own PLY readers on ASCII files (build box only: needs the reference).

The reference's ``Ply3DGSFormat.read`` (formats/ply_3dgs.py:8-60) and ``PlyCCFormat.read`` (formats/ply_cc.py:8-62) run unchanged;
only ``plyfile`` (not installed here) is a stub whose ``PlyData.read`` is the ASCII oracle of tests/ply_text_numpy.py: the contract
of DESIGN.md "ASCII PLY bodies", every element as a structured array in the declared types.  The input files are stored whole,
the reference's rows whole; per case and reader the spec records names, dtype strings, itemsize, rows and the other elements.

    python tests/devtools/make_golden_ply_text.py
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
import ply_text_numpy as pt  # noqa: E402
from oracle import refload  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ply_text_ref.npz")
BOTH = ("3dgs", "cc")


def reference_read(path, dialect):
    stub = types.ModuleType("plyfile")
    stub.PlyData = pt.PlyData
    stub.PlyElement = object
    sys.modules["plyfile"] = stub
    refload.load()
    if dialect == "3dgs":
        import gsconverter.formats.ply_3dgs as mod  # type: ignore
        fmt = mod.Ply3DGSFormat()
    else:
        import gsconverter.formats.ply_cc as mod  # type: ignore
        fmt = mod.PlyCCFormat()
    with np.errstate(all="ignore"):
        rows = fmt.read(path)
    return rows, [el.name for el in fmt.extra_elements]


def cases(tmp):
    """-> [(name, path)]"""
    rng = np.random.default_rng(20261021)
    out = []

    def add(name, elements, formats=None, **kw):
        out.append((name, pt.write_arrays(os.path.join(tmp, name + ".ply"), elements, formats, **kw)))

    def doubles(n, subnormal):   # every standard field a double: Gaussian, log-uniform and random-bit finite values
        t = pn.build(n, pn.canonical_fields(3, "f8"), rng)
        for k, f in enumerate(t.dtype.names):
            if k % 3 == 1:
                t[f] = rng.standard_normal(n) * 10.0 ** rng.integers(-30, 31, n)
            elif k % 3 == 2:
                v = rng.integers(0, 1 << 64, n, dtype=np.uint64).view(np.float64)
                t[f] = np.where(np.isfinite(v) & (subnormal | (np.abs(v) >= 2.2250738585072014e-308) | (v == 0)), v, 1.0)
        return t

    add("digits15", [("vertex", doubles(100, False))], {"f8": "%.15g"})   # (a subnormal result is the host's)
    add("repr", [("vertex", doubles(100, True))], {"f8": lambda v: repr(float(v))})
    add("cc_crlf", [("vertex", pn.build(40, pn.cc_fields(3), rng))], eol="\r\n")
    camera = pn.build(3, [("fx", "f4"), ("fy", "f8"), ("id", "i4"), ("flag", "u1")], rng)
    add("camera_both_sides", [("camera", camera), ("vertex", pn.build(20, pn.canonical_fields(1), rng)), ("camera2", camera[:2])], sep="\t")
    mixed = [(f, pn.SOURCE_TYPES[k % 8]) for k, (f, _) in enumerate(pn.canonical_fields(3))]
    add("every_source_type", [("vertex", pn.build(40, mixed + [(c, "u1") for c in pn.COLOURS], rng))], last_newline=False)
    return out


def main():
    import tempfile
    spec, arrays = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, path in cases(tmp):
            with open(path, "rb") as f:
                data = f.read()
            arrays[name + "__file"] = np.frombuffer(data, np.uint8)
            rec = {"file_bytes": len(data), "file_sha256": hashlib.sha256(data).hexdigest(), "readers": {}}
            for dialect in BOTH:
                rows, extra_names = reference_read(path, dialect)
                assert len(rows) <= 300, name
                rec["readers"][dialect] = {"names": list(rows.dtype.names), "dtype": [rows.dtype[f].str for f in rows.dtype.names],
                                           "itemsize": rows.dtype.itemsize, "rows": len(rows), "extra_elements": extra_names}
                arrays["%s__%s__rows" % (name, dialect)] = np.ascontiguousarray(rows).view(np.uint8).reshape(-1).copy()
                mine, others = pt.read(path, dialect)
                assert mine.dtype == rows.dtype and mine.tobytes() == rows.tobytes() and [n for n, _ in others] == extra_names, (name, dialect)
            spec[name] = rec
            print(name, {d: "%d rows x %d bytes" % (r["rows"], r["itemsize"]) for d, r in rec["readers"].items()})
    arrays["spec"] = np.frombuffer(json.dumps(spec, sort_keys=True).encode(), np.uint8)
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    assert len(buf.getvalue()) < 1_000_000
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print(OUT, len(buf.getvalue()), "bytes")


if __name__ == "__main__":
    main()
