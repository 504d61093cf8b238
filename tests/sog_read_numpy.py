"""The SOG reader restated in numpy (gsconverter/formats/sog.py:23-247), and builders of .sog files.

``read`` is checked against the reference's recorded rows on every case of tests/golden/sog_read_ref.npz
(tests/test_sog_read_host.py), which licenses it as the checker at sizes the golden file cannot hold.  It keeps the reference's
statements and operand dtypes (float64 positions rounded on assignment, float32 rotation and opacity, uint8 slot arithmetic);
the one change is the palette's Python double loop (:190-202), here one fancy index with the same pixel formula.

The builders save WebP with lossless=True, exact=True: without `exact` the encoder discards the colour of a pixel whose alpha
is 0 (an sh0 texel of opacity byte 0, any means or labels texel with alpha 0).
"""
import hashlib
import io
import json
import zipfile

import numpy as np
from PIL import Image

COEFFS = (0, 9, 24, 45)
BASE_BEFORE = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
BASE_AFTER = ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
TEXTURES = ("means_l", "means_u", "scales", "quats", "sh0", "shN_centroids", "shN_labels")     # the reference's reading order
MINS, MAXS = [-3.1, -0.2, 0.0], [2.5, 4.0, 7.7]


def sha(rows) -> bytes:
    return hashlib.sha256(np.ascontiguousarray(rows).view(np.uint8).tobytes()).digest()


def define_dtype(bands: int) -> np.dtype:
    """structures.py:23-59 with has_scal=False, has_rgb=False"""
    return np.dtype([(f, "f4") for f in BASE_BEFORE] + [("f_rest_%d" % i, "f4") for i in range(3 * ((bands + 1) ** 2 - 1))]
                    + [(f, "f4") for f in BASE_AFTER])


# ---- per-code results (what the device takes from tables)
def position_of(qv, lo, hi):
    """:78-82 -- qv uint16; float64"""
    norm = qv / 65535.0
    log_val = norm * (hi - lo) + lo
    return np.sign(log_val) * (np.exp(np.abs(log_val)) - 1.0)


def opacity_of(b):
    a = np.clip(b.astype(np.float32) / 255.0, 1.0 / 255.0, 0.9999)
    return -np.log((1.0 / a) - 1.0)


def quat_component_of(b):
    return (b.astype(np.float32) / 255.0 - 0.5) * 2.0


def centroid_pixel(i, j, cpb):
    """:192-194 -- the READER's pixel of coefficient j of palette entry i (the writer put it at i * (cpb // 3) + j)"""
    return (i // 64) * (64 * cpb) + (i % 64) * (cpb // 3) + j


def read(path: str) -> np.ndarray:
    if not zipfile.is_zipfile(path):
        raise ValueError("SOG Format: Only ZIP-bundled .sog files are supported.")
    with zipfile.ZipFile(path, "r") as zf:
        with zf.open("meta.json") as f:
            meta = json.load(f)
        count = meta["count"]

        def flat(filename, expected=None):
            expected = count if expected is None else expected
            with zf.open(filename) as f:
                img = Image.open(f)
                width, height = img.size
                if img.mode != "RGBA":
                    img = img.convert("RGBA")
                data = np.array(img).flatten()
                if width * height < expected:
                    raise ValueError(f"Image {filename} too small: {width * height} < {expected}")
                return data[:expected * 4]
        return decode(meta, flat)


def decode(meta, flat) -> np.ndarray:
    """:60-247 -- flat(file name, expected=None) -> the texture's first `expected` (default count) RGBA texels, flat"""
    count = meta["count"]
    with np.errstate(all="ignore"):
        means_l = flat(meta["means"]["files"][0]).reshape(-1, 4)[:count]
        means_u = flat(meta["means"]["files"][1]).reshape(-1, 4)[:count]
        mins, maxs = meta["means"]["mins"], meta["means"]["maxs"]
        xyz = [position_of(means_l[:, a].astype(np.uint16) | (means_u[:, a].astype(np.uint16) << 8), mins[a], maxs[a]) for a in range(3)]
        scales_idx = flat(meta["scales"]["files"][0]).reshape(-1, 4)[:count]
        scale_codebook = np.array(meta["scales"]["codebook"], dtype=np.float32)
        scale = [scale_codebook[scales_idx[:, a]] for a in range(3)]
        quats_u8 = flat(meta["quats"]["files"][0]).reshape(-1, 4)[:count]
        q_rest = quat_component_of(quats_u8[:, :3])
        max_comp_idx = quats_u8[:, 3] - 252                                          # uint8: wraps below 252
        q_missing = np.sqrt(np.maximum(1.0 - np.sum(q_rest ** 2, axis=1), 0.0))
        rot = np.zeros((4, count), np.float32)
        for mc in range(4):
            mask = max_comp_idx == mc
            rest = [k for k in range(4) if k != mc]
            rot[mc][mask] = q_missing[mask]
            for slot, k in enumerate(rest):
                rot[k][mask] = q_rest[mask, slot]
        sh0_raw = flat(meta["sh0"]["files"][0]).reshape(-1, 4)[:count]
        sh0_codebook = np.array(meta["sh0"]["codebook"], dtype=np.float32)
        f_dc = [sh0_codebook[sh0_raw[:, a]] for a in range(3)]
        opacity = opacity_of(sh0_raw[:, 3])
        bands, sh_values = 0, None
        if "shN" in meta:
            bands, palette_size = meta["shN"]["bands"], meta["shN"]["count"]
            cpb = [0, 9, 24, 45][bands]
            cpc = cpb // 3
            raw = flat(meta["shN"]["files"][0], expected=64 * cpb * int(np.ceil(palette_size / 64)))
            i, j = np.arange(palette_size)[:, None], np.arange(cpc)[None, :]
            pix = centroid_pixel(i, j, cpb)                                           # [P, C]
            indices = np.zeros((palette_size, 3, cpc), np.uint8)
            for ch in range(3):
                indices[:, ch, :] = raw[pix * 4 + ch]
            codebook_sh = np.array(meta["shN"]["codebook"], dtype=np.float32)
            palette_flat = codebook_sh[indices].reshape(palette_size, -1)
            labels_raw = flat(meta["shN"]["files"][1]).reshape(-1, 4)[:count]
            labels = labels_raw[:, 0].astype(np.uint16) | (labels_raw[:, 1].astype(np.uint16) << 8)
            sh_values = palette_flat[labels]
        out = np.zeros(count, define_dtype(bands))
        for a, f in enumerate("xyz"):
            out[f] = xyz[a]
        for a in range(3):
            out["scale_%d" % a], out["f_dc_%d" % a] = scale[a], f_dc[a]
        for a in range(4):
            out["rot_%d" % a] = rot[a]
        out["opacity"] = opacity
        if sh_values is not None:
            for k in range(sh_values.shape[1]):
                out["f_rest_%d" % k] = sh_values[:, k]
        return out


# ---- file builders
def dims(n: int):
    """the writer's texture size (:259-260), at least 4 x 4"""
    w = max(4, int(np.ceil(np.sqrt(n) / 4) * 4))
    return w, max(4, int(np.ceil(n / w / 4) * 4))


def webp(pixels, w: int, h: int, mode: str = "RGBA") -> bytes:
    """pixels uint8 [h * w, 4] (mode RGBA; RGB takes the first three channels, L the first)"""
    pixels = np.ascontiguousarray(pixels, np.uint8).reshape(h * w, 4)
    raw = {"RGBA": pixels, "RGB": pixels[:, :3], "L": pixels[:, 0]}[mode]
    bio = io.BytesIO()
    Image.frombytes(mode, (w, h), np.ascontiguousarray(raw).tobytes()).save(bio, format="WEBP", lossless=True, exact=True, quality=100, method=0)
    return bio.getvalue()


def codebook(rng, size=256, spread=2.0, decimals=3):
    """sorted Python floats: short decimals (a small meta.json), or with decimals None float32 values spelled as doubles"""
    v = (rng.standard_normal(size) * spread).astype(np.float32)
    return sorted(float(x) if decimals is None else round(float(x), decimals) for x in v)


def meta_for(n, bands=0, palette=0, rng=None, mins=None, maxs=None, sizes=(256, 256, 256), decimals=3):
    rng = rng or np.random.default_rng(0)
    meta = {"version": 2, "asset": {"generator": "gsconverter-sog"}, "count": n,
            "means": {"mins": list(mins or MINS), "maxs": list(maxs or MAXS), "files": ["means_l.webp", "means_u.webp"]},
            "scales": {"codebook": codebook(rng, sizes[0], 3.0, decimals), "files": ["scales.webp"]},
            "quats": {"files": ["quats.webp"]},
            "sh0": {"codebook": codebook(rng, sizes[1], 1.5, decimals), "files": ["sh0.webp"]}}
    if bands:
        meta["shN"] = {"count": palette, "bands": bands, "codebook": codebook(rng, sizes[2], 0.3, decimals), "files": ["shN_centroids.webp", "shN_labels.webp"]}
    return meta


def centroid_dims(bands, palette):
    return 64 * COEFFS[bands], max(1, (palette + 63) // 64)


def padded(tex, npix, fill=255):
    """texels uint8 [n, 4] -> [npix, 4], the rest `fill`"""
    out = np.full((npix, 4), fill, np.uint8)
    out[:len(tex)] = tex
    return out


def random_texels(n, bands, palette, rng, alpha_any=True):
    """-> {texture: uint8 [n, 4]} (centroids [w_c * h_c, 4]): random bytes in every channel, alpha included; quats alpha mostly
    252 ... 255; labels below `palette`, the last row's label palette - 1"""
    t = {k: rng.integers(0, 256, (n, 4), dtype=np.uint8) for k in ("means_l", "means_u", "scales", "quats", "sh0")}
    if n:
        slot = rng.integers(252, 256, n)
        t["quats"][:, 3] = np.where(rng.random(n) < 0.9, slot, t["quats"][:, 3]) if alpha_any else slot
    if bands:
        w_c, h_c = centroid_dims(bands, palette)
        cen = np.full((h_c, w_c, 4), 255, np.uint8)                # random where the reader looks (:193), 255 elsewhere: a small file
        used = 64 * (COEFFS[bands] // 3)
        cen[:, :used] = rng.integers(0, 256, (h_c, used, 4), dtype=np.uint8)
        t["shN_centroids"] = cen.reshape(-1, 4)
        lab = rng.integers(0, palette, n).astype(np.uint32)
        if n:
            lab[-1] = palette - 1
        t["shN_labels"] = labels_texels(lab, rng)
    return t


def labels_texels(lab, rng=None):
    n = len(lab)
    tex = np.zeros((n, 4), np.uint8) if rng is None else rng.integers(0, 256, (n, 4), dtype=np.uint8)
    tex[:, 0], tex[:, 1] = lab & 0xFF, lab >> 8
    return tex


def smooth_texels(n, bands, palette):
    """texels that compress: slowly varying bytes per channel, yet every byte value and every slot occur"""
    i = np.arange(n, dtype=np.int64)
    def tex(*steps):
        return np.stack([((i // s + 17 * k) & 0xFF) for k, s in enumerate(steps)], axis=1).astype(np.uint8)
    t = {"means_l": tex(1, 2, 3, 97), "means_u": tex(256, 300, 411, 89), "scales": tex(5, 7, 11, 83), "quats": tex(3, 13, 29, 1),
         "sh0": tex(4, 6, 9, 2)}
    t["quats"][:, 3] = 252 + (i // 50) % 4
    t["quats"][::211, 3] = (i[::211] // 211) & 0xFF
    if bands:
        w_c, h_c = centroid_dims(bands, palette)
        p = np.arange(w_c * h_c, dtype=np.int64)
        t["shN_centroids"] = np.stack([(p // 3) & 0xFF, (p // 5 + 80) & 0xFF, (p // 7 + 160) & 0xFF, np.full_like(p, 255)], axis=1).astype(np.uint8)
        lab = ((i // 3) * 7) % palette
        lab[-1:] = palette - 1
        t["shN_labels"] = labels_texels(lab.astype(np.uint32))
        t["shN_labels"][:, 3] = 255
    return t


def write_bundle(path, meta, members: dict):
    """path: a file name or a writable binary file; members: {file name: bytes}; meta None leaves meta.json out"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as zf:
        for name, data in members.items():
            zf.writestr(zipfile.ZipInfo(name, (2020, 1, 1, 0, 0, 0)), data)        # a fixed date: the same bytes on every run
        if meta is not None:
            zf.writestr(zipfile.ZipInfo("meta.json", (2020, 1, 1, 0, 0, 0)), json.dumps(meta))
    return path


def encode_textures(texels: dict, n, bands=0, palette=0, size=None, modes=None) -> dict:
    """{texture: texels} -> {file name: WebP bytes}; size: (w, h) of the per-row textures, by default the writer's"""
    w, h = size or dims(n)
    out = {}
    for name, tex in texels.items():
        if name == "shN_centroids":
            w_c, h_c = centroid_dims(bands, palette)
            if len(tex) != w_c * h_c:            # a caller's own shape: (texels, w, h)
                tex, w_c, h_c = tex
            out[name + ".webp"] = webp(tex, w_c, h_c, (modes or {}).get(name, "RGBA"))
        else:
            out[name + ".webp"] = webp(padded(tex, w * h), w, h, (modes or {}).get(name, "RGBA"))
    return out


def build_file(path, n, bands, palette, rng, meta=None, texels=None, size=None, modes=None, **meta_kw) -> str:
    """a random file (or the given texels / meta)"""
    texels = texels if texels is not None else random_texels(n, bands, palette, rng)
    meta = meta if meta is not None else meta_for(n, bands, palette, rng, **meta_kw)
    return write_bundle(path, meta, encode_textures(texels, n, bands, palette, size, modes))


def edge_triples() -> np.ndarray:
    """byte triples around a float32 sum of squares (c0^2 + c1^2) + c2^2 of 1, found by a search of all 2^24: the two largest
    sums below 1 and the two smallest above 1 (no byte triple sums to exactly 1: asserted) -> uint8 [4, 3]"""
    c = quat_component_of(np.arange(256, dtype=np.uint8))
    sq = c * c
    s = (sq[:, None, None] + sq[None, :, None]) + sq[None, None, :]
    assert s.dtype == np.float32 and not (s == np.float32(1)).any()
    below = np.where(s < 1, s, -1).reshape(-1)
    above = np.where(s > 1, s, 9).reshape(-1)
    picks = [np.argmax(below), np.argmax(np.where(below < below.max(), below, -1)), np.argmin(above), np.argmin(np.where(above > above.min(), above, 9))]
    return np.array([np.unravel_index(k, s.shape) for k in picks], np.uint8)


def pattern_texels(bands, palette=300, n=65536):
    """65 536 rows: every u16 code on every position axis; every byte in every channel of scales, sh0 and quats; every alpha
    byte in quats; rotation triples with a sum of squares above 1, exactly 1 and just below 1 in the first rows"""
    assert n == 65536
    i = np.arange(n, dtype=np.uint32)
    codes = [i, i[::-1], (i * 40503 + 7) & 0xFFFF]
    t = {"means_l": np.stack([c & 0xFF for c in codes] + [i & 0xFF], axis=1).astype(np.uint8),
         "means_u": np.stack([c >> 8 for c in codes] + [(i >> 3) & 0xFF], axis=1).astype(np.uint8)}
    for k, name in enumerate(("scales", "sh0", "quats")):
        t[name] = np.stack([((i * (2 * a + 1) + 37 * a + 11 * k) >> (0 if a < 3 else 8)) & 0xFF for a in range(4)], axis=1).astype(np.uint8)
    t["quats"][:, 3] = (i >> 8) & 0xFF                                                # 256 rows of every alpha byte
    t["quats"][i % 3 == 0, 3] = 252 + (i[i % 3 == 0] // 3) % 4
    edge = np.array([[255, 255, 255], [0, 0, 0], [255, 0, 128], [255, 127, 128], [255, 128, 128], [255, 127, 127], [127, 127, 127], [128, 128, 128],
                     [218, 218, 127], [217, 218, 128], [37, 218, 128], [128, 255, 127], [0, 128, 127], [201, 201, 201], [200, 201, 202]], np.uint8)
    edge[-4:] = edge_triples()
    for s in range(4):
        t["quats"][15 * s:15 * (s + 1), :3] = edge
        t["quats"][15 * s:15 * (s + 1), 3] = 252 + s
    if bands:
        w_c, h_c = centroid_dims(bands, palette)
        p = np.arange(w_c * h_c, dtype=np.uint32)
        t["shN_centroids"] = np.stack([(p * 3 + 1) & 0xFF, (p * 5 + 2) & 0xFF, (p * 7 + 3) & 0xFF, p & 0xFF], axis=1).astype(np.uint8)
        lab = i % palette
        lab[-1] = palette - 1
        t["shN_labels"] = labels_texels(lab)
        t["shN_labels"][:, 2:] = t["scales"][:, 2:]
    return t


def pattern_file(path, bands, palette=300) -> str:
    n = 65536
    return build_file(path, n, bands, palette, np.random.default_rng(5 + bands), texels=pattern_texels(bands, palette))



def staged_rows(host, place, n, bands, palette, mins, maxs, codebooks):
    """`decode` on the staged texels (_lib.sog_texel_layout): the per-row textures as they lie there, the compacted centroid
    pixels put back where the reader looks for them (:193) -> (rows, False), or (None, True) when a label is at or above
    `palette`.  codebooks: the scales, sh0 and shN lists of meta.json"""
    def tex(name):
        off, nb = place[name]
        return host[off:off + nb]

    def flat(name, expected=None):
        if name != "shN_centroids":
            return tex(name)
        cpb = COEFFS[bands]
        image = np.zeros((expected // (64 * cpb), 64 * cpb, 4), np.uint8)
        image[:, :64 * (cpb // 3)] = tex(name).reshape(image.shape[0], 64 * (cpb // 3), 4)
        return image.reshape(-1)
    meta = {"count": n, "means": {"mins": mins, "maxs": maxs, "files": ["means_l", "means_u"]},
            "scales": {"codebook": codebooks[0], "files": ["scales"]}, "quats": {"files": ["quats"]},
            "sh0": {"codebook": codebooks[1], "files": ["sh0"]}}
    if bands:
        meta["shN"] = {"count": palette, "bands": bands, "codebook": codebooks[2], "files": ["shN_centroids", "shN_labels"]}
        lab = tex("shN_labels").reshape(-1, 4).astype(np.uint32)
        if ((lab[:, 0] | (lab[:, 1] << 8)) >= palette).any():
            return None, True
    return decode(meta, flat), False
