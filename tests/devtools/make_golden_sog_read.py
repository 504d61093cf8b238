"""Build tests/golden/sog_read_ref.npz from the REFERENCE's own SOG reader (build box only: needs the reference).

The reference's ``SogFormat().read`` (formats/sog.py:23-247) runs unchanged on every case.  The input files come from
tests/sog_read_numpy.py's builders (random texels in every channel, every band count, palettes on both sides of the 64-entry
image row, textures larger than needed and of other modes than RGBA, one file laid out as the reference's writer does) and are
stored whole.  Per case the spec records the reference's dtype names / types and its rows (whole for small cases, sha256 of the
row bytes for larger ones), or the exception it raised: type and message.  Every error case has exactly one defect.

Every case's position table is asserted to lie at least 4 float64 ulps from a float32 rounding boundary in every entry (random
mins / maxs are redrawn until it does), so that a host whose numpy takes another float64 exp path still gives the recorded bits.

    python tests/devtools/make_golden_sog_read.py
"""
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sog_read_numpy as srn  # noqa: E402
from oracle import refload  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sog_read_ref.npz")
WHOLE_BELOW = 6000           # row bytes up to this are stored whole
MARGIN_ULPS = 4


def reference_read(path):
    refload.load()
    import gsconverter.formats.sog as mod  # type: ignore
    try:
        with np.errstate(all="ignore"):
            return mod.SogFormat().read(path), None
    except Exception as e:  # noqa: BLE001 -- the reference's own error is the expected result
        return None, [type(e).__module__ + "." + type(e).__name__, str(e)]


def boundary_margin(mins, maxs) -> float:
    """the smallest distance, in float64 ulps, of an entry of the position table from the float32 rounding boundary next to it"""
    worst = np.inf
    qv = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    with np.errstate(all="ignore"):
        for a in range(3):
            v = srn.position_of(qv, mins[a], maxs[a])
            f = v.astype(np.float32)
            other = np.nextafter(f, np.where(v >= f, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
            mid = (f.astype(np.float64) + other.astype(np.float64)) / 2
            ok = np.isfinite(v) & np.isfinite(mid)
            worst = min(worst, float((np.abs(v - mid) / np.spacing(np.abs(v)))[ok].min()))
    return worst


def drawn_range(rng):
    while True:
        mins = [round(float(v), 3) for v in rng.uniform(-6, 0, 3)]
        maxs = [round(float(v), 3) for v in rng.uniform(0.5, 8, 3)]
        if boundary_margin(mins, maxs) >= MARGIN_ULPS:
            return mins, maxs


def bundle(meta, members) -> bytes:
    bio = io.BytesIO()
    srn.write_bundle(bio, meta, members)
    return bio.getvalue()


def cases():
    """-> [(name, file bytes, (mins, maxs) or None)]"""
    rng = np.random.default_rng(20261018)
    out = []

    def add(name, n, bands, palette, texels=None, meta=None, size=None, modes=None, drop=None, **meta_kw):
        meta = meta if meta is not None else srn.meta_for(n, bands, palette, rng, **meta_kw)
        texels = texels if texels is not None else srn.random_texels(n, bands, palette, rng)
        members = srn.encode_textures(texels, n, bands, palette, size, modes)
        for d in drop or ():
            del members[d]
        out.append((name, bundle(meta, members), (meta["means"]["mins"], meta["means"]["maxs"]) if isinstance(meta, dict) and "means" in meta else None))
        return meta, texels

    add("b0", 23, 0, 0)
    add("b1", 31, 1, 7)
    add("b2", 37, 2, 65)
    add("b3", 41, 3, 130)
    add("n0_b0", 0, 0, 0)
    add("n0_b2", 0, 2, 70)
    mins, maxs = drawn_range(rng)
    add("drawn_range", 29, 1, 20, mins=mins, maxs=maxs)
    add("integer_range", 19, 0, 0, mins=[-2, 0, 1], maxs=[3, 5, 1])
    add("reversed_range", 19, 0, 0, mins=[2.5, 0.75, -1.0], maxs=[-3.0, 0.75, -4.5])
    add("double_codebooks", 27, 1, 9, decimals=None)
    add("long_codebooks", 33, 1, 12, sizes=(300, 257, 400))
    for p in (1, 63, 64, 65, 128, 300):
        add("palette_%d" % p, 45, 1, p)
    add("palette_300_b3", 140, 3, 300)
    add("larger_textures", 30, 2, 40, size=(12, 9))
    add("other_width", 100, 1, 5, size=(7, 15))
    add("modes", 50, 1, 30, modes={"means_u": "RGB", "scales": "RGB", "sh0": "RGB", "quats": "RGB", "shN_labels": "RGB", "shN_centroids": "RGB"})
    add("mode_l", 26, 0, 0, modes={"scales": "L", "means_l": "L"})
    t = srn.random_texels(256, 0, 0, rng)
    t["quats"][:, 3] = np.arange(256)
    add("every_quat_alpha", 256, 0, 0, texels=t)
    # the reference's WRITER lays coefficient j of palette entry i down at pixel i * C + j (:584-588); its reader looks elsewhere
    n, bands, palette = 60, 2, 130
    t = srn.random_texels(n, bands, palette, rng)
    w_c, h_c = srn.centroid_dims(bands, palette)
    cen = np.full((w_c * h_c, 4), 255, np.uint8)
    cen[:palette * 8, :3] = rng.integers(0, 256, (palette * 8, 3), dtype=np.uint8)
    t["shN_centroids"] = cen
    add("writer_layout", n, bands, palette, texels=t)
    add("smooth_b0", 5000, 0, 0, texels=srn.smooth_texels(5000, 0, 0))
    add("smooth_b3", 20000, 3, 1000, texels=srn.smooth_texels(20000, 3, 1000))

    # ---- one defect each
    out.append(("err_not_zip", b"not a zip bundle at all" * 9, None))
    meta, t = add("err_no_meta", 21, 1, 7)
    out[-1] = ("err_no_meta", bundle(None, srn.encode_textures(t, 21, 1, 7)), None)
    meta = srn.meta_for(21, 1, 7, rng)
    del meta["quats"]
    add("err_missing_key", 21, 1, 7, meta=meta)
    add("err_missing_texture", 21, 1, 7, drop=["sh0.webp"])
    n, bands, palette = 41, 1, 7                     # 40 = 8 x 5 pixels; the centroid image needs 576: 575 = 25 x 23
    for name in srn.TEXTURES:
        t = srn.random_texels(n, bands, palette, rng)
        meta = srn.meta_for(n, bands, palette, rng)
        members = srn.encode_textures(t, n, bands, palette)
        if name == "shN_centroids":
            members[name + ".webp"] = srn.webp(t[name][:575], 25, 23)
        else:
            members[name + ".webp"] = srn.webp(t[name][:40], 8, 5)
        out.append(("err_small_" + name, bundle(meta, members), (meta["means"]["mins"], meta["means"]["maxs"])))
    for k, name in enumerate(("scales", "sh0", "shN")):
        sizes = [256, 256, 256]
        sizes[k] = 200
        t = srn.random_texels(n, bands, palette, rng)
        tex = t["shN_centroids" if name == "shN" else name]
        tex[:, :3] = np.minimum(tex[:, :3], 199)
        tex[5 if name != "shN" else 64 * 3 * 0 + 4, 1] = 212          # the one index past the codebook
        add("err_short_" + name, n, bands, palette, texels=t, sizes=tuple(sizes))
    return out


def main():
    import tempfile
    spec, arrays = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, data, span in cases():
            if span is not None:
                margin = boundary_margin(*span)
                assert margin >= MARGIN_ULPS, (name, margin)
            path = os.path.join(tmp, name + ".sog")
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
                rec["dtype"] = [rows.dtype[f].str for f in rows.dtype.names]
                rec["itemsize"] = rows.dtype.itemsize
                raw = np.ascontiguousarray(rows).view(np.uint8).reshape(-1)
                if raw.nbytes <= WHOLE_BELOW:
                    arrays[name + "__rows"] = raw.copy()
                else:
                    arrays[name + "__sha256"] = np.frombuffer(srn.sha(rows), np.uint8)
                rec["nan_words"] = int(sum(np.isnan(rows[f]).sum() for f in rows.dtype.names))
            spec[name] = rec
            print(name, len(data), rec.get("error") or ("%d rows, %d NaN words" % (rec["rows"], rec.get("nan_words", 0))))
    arrays["spec"] = np.frombuffer(json.dumps(spec, sort_keys=True).encode(), np.uint8)
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print(OUT, len(buf.getvalue()), "bytes")


if __name__ == "__main__":
    main()
