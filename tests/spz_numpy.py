"""A numpy restatement of the SPZ v3 payload (header + body) and the deterministic tables the SPZ tests run on.

The restatement is the checker where the reference is absent (the GPU box: tests/test_spz_gpu.py at 1M rows,
tests/devtools/check_spz_large.py at 10M and 50M).  It states the format from its description -- six sections of fixed
width per splat, float32 arithmetic with numpy's rounding and numpy's own casts -- and is itself checked against the
reference's payloads in tests/golden/spz_ref.npz (tests/test_spz_host.py).
"""
from __future__ import annotations

import struct

import numpy as np

F = np.float32
SH_DIM = {0: 0, 1: 3, 2: 8, 3: 15}


# ------------------------------------------------------------------------------------------------------------ payload
def sh_degree(data: np.ndarray) -> int:
    names = data.dtype.names
    if "f_rest_0" not in names:
        return 0
    top = next((t for t in (44, 23, 8) if f"f_rest_{t}" in names), None)
    if top is None:
        return 0
    last = next((i for i in range(top, -1, -1) if f"f_rest_{i}" in names and np.count_nonzero(data[f"f_rest_{i}"])), -1)
    return 3 if last >= 24 else 2 if last >= 9 else 1 if last >= 0 else 0


def _bytes24(v: np.ndarray) -> np.ndarray:
    """(n, 3) float32 -> (n, 9) bytes: round(v * 4096) as int32, the three low bytes of each axis"""
    with np.errstate(all="ignore"):
        q = np.rint(v * F(4096)).astype(np.int32)
    return np.stack([(q >> s) & 0xFF for s in (0, 8, 16)], axis=-1).astype(np.uint8).reshape(len(v), 9)


def _u8(v: np.ndarray, lo, hi) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return np.clip(v, lo, hi).astype(np.uint8)


def _rotations(data: np.ndarray) -> np.ndarray:
    """smallest-three: X Y Z W of the normalised quaternion, the largest |component|'s index in bits 30-31, the other three
    (earliest first from bit 20 down) as sign-relative-to-the-largest + 9-bit magnitude"""
    n = len(data)
    w, x, y, z = (data[f"rot_{i}"] for i in range(4))
    with np.errstate(all="ignore"):
        norm = np.sqrt(w * w + x * x + y * y + z * z + F(1e-9))
        r = np.stack([x / norm, y / norm, z / norm, w / norm], axis=1)
    big = np.argmax(np.abs(r), axis=1)
    word = big.astype(np.uint32) << np.uint32(30)
    neg = r[np.arange(n), big] < 0
    scale = F(511.0 / 0.7071067811865476)
    for j in range(4):
        sel = big != j
        v = r[sel, j]
        with np.errstate(all="ignore"):
            mag = np.clip(np.abs(v) * scale + F(0.5), 0, 511).astype(np.uint32)   # one array per component, as cast there
        sign = ((v < 0) != neg[sel]).astype(np.uint32)
        shift = ((2 - (j - (big[sel] < j))) * 10).astype(np.uint32)
        word[sel] |= ((sign << np.uint32(9)) | mag) << shift
    return word.astype("<u4")


def _sh(data: np.ndarray, d: int) -> np.ndarray:
    names = [[f"f_rest_{i + 15 * c}" for i in range(d)] for c in range(3)]
    chans = [[data[nm] for nm in row] for row in names]          # red coefficients first, then green, then blue
    v = np.stack([chans[c][i] for i in range(d) for c in range(3)], axis=1)
    with np.errstate(all="ignore"):
        q = np.rint(v * F(128) + F(128)).astype(np.int32)
    bs = np.where(np.arange(3 * d) < 9, 8, 16).astype(np.int32)
    return np.clip((q + bs // 2) // bs * bs, 0, 255).astype(np.uint8)


def sections(data: np.ndarray, deg: int):
    """the body's six sections (positions, alpha, colours, scales, rotations, SH) as arrays of whole rows"""
    n = len(data)
    names = data.dtype.names
    xyz = np.stack([data[a] for a in "xyz"], axis=1)
    parts = [_bytes24(xyz)]
    if "opacity" in names:
        with np.errstate(all="ignore"):
            a = F(1) / (F(1) + np.exp(-np.clip(data["opacity"], F(-20), F(20)))) * F(255)
        parts.append(_u8(a, 0, 255))
    else:
        parts.append(np.full(n, 255, np.uint8))
    if "f_dc_0" in names:
        dc = np.stack([data[f"f_dc_{c}"] for c in range(3)], axis=1)
        parts.append(_u8((dc * F(0.15) + F(0.5)) * F(255), 0, 255))
    else:
        parts.append(np.full((n, 3), 128, np.uint8))
    sc = np.stack([data[f"scale_{c}"] for c in range(3)], axis=1)
    parts.append(_u8((sc + F(10)) * F(16), 0, 255))
    parts.append(_rotations(data))
    parts.append(_sh(data, SH_DIM[deg]) if SH_DIM[deg] else np.zeros((n, 0), np.uint8))
    return parts


def header(n: int, deg: int) -> bytes:
    return struct.pack("<IIIBBBB", 0x5053474E, 3, n, deg, 12, 1, 0)


def payload(data: np.ndarray) -> bytes:
    """the uncompressed .spz content (raises numpy's ValueError for a field the format needs and the table lacks)"""
    deg = sh_degree(data)
    return header(len(data), deg) + b"".join(np.ascontiguousarray(p).tobytes() for p in sections(data, deg))


# ------------------------------------------------------------------------------------------------------------ tables
def dtype_3dgs(n_rest=45, opacity=True, dc=True, rgb=False) -> np.dtype:
    """the converter's 3DGS row: x y z nx ny nz | f_dc_0..2 | f_rest_* | opacity | scale_0..2 | rot_0..3 (+ red green blue u1)"""
    fl = ["x", "y", "z", "nx", "ny", "nz"] + (["f_dc_0", "f_dc_1", "f_dc_2"] if dc else [])
    fl += [f"f_rest_{i}" for i in range(n_rest)] + (["opacity"] if opacity else [])
    fl += ["scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    return np.dtype([(f, "<f4") for f in fl] + ([(c, "u1") for c in ("red", "green", "blue")] if rgb else []))


def random_table(n: int, seed: int, n_rest=45, opacity=True, dc=True, rgb=False, sh_scale=0.3, sh_upto=None) -> np.ndarray:
    """a plausible scene: positions up to +-60, log-scales around -4, opacity logits, unnormalised quaternions.
    sh_upto: f_rest fields from this index on are zero"""
    rng = np.random.default_rng(seed)
    t = np.zeros(n, dtype_3dgs(n_rest, opacity, dc, rgb))
    for f in t.dtype.names:
        if f in ("red", "green", "blue"):
            t[f] = rng.integers(0, 256, n)
        elif f in ("x", "y", "z"):
            t[f] = rng.uniform(-60, 60, n)
        elif f.startswith("scale_"):
            t[f] = rng.normal(-4.0, 1.5, n)
        elif f == "opacity":
            t[f] = rng.normal(0.0, 3.0, n)
        elif f.startswith("f_dc_"):
            t[f] = rng.normal(0.0, 1.2, n)
        elif f.startswith("f_rest_"):
            i = int(f[7:])
            t[f] = 0.0 if sh_upto is not None and i >= sh_upto else rng.normal(0.0, sh_scale, n)
        else:
            t[f] = rng.normal(0.0, 1.0, n)
    return t


def _near_byte_opacities() -> np.ndarray:
    """opacities whose alpha (1 / (1 + exp(-o)) * 255) lands within a few ulp of an integer"""
    out = []
    for k in range(1, 255):
        o = np.float32(-np.log(255.0 / k - 1.0))
        b = o.view(np.int32)
        out += [np.int32(b + d).view(np.float32) for d in range(-3, 4)]
    return np.array(out, np.float32)


def _sh_boundary_values() -> np.ndarray:
    """values on every rounding (k + 0.5) and floor-division (multiple of 8 / 16 minus half) boundary of v * 128 + 128"""
    vals = []
    for t in np.arange(-2.0, 260.0, 0.5):
        v = np.float32((t - 128.0) / 128.0)
        b = v.view(np.int32)
        vals += [np.int32(b + d).view(np.float32) for d in (-1, 0, 1)]
    vals += [np.nan, np.inf, -np.inf, 3e38, -3e38, 1.7e7, -1.7e7, 0.0, -0.0]
    return np.array(vals, np.float32)


def edge_table() -> np.ndarray:
    """explicit edge rows (248-byte 3DGS rows, degree 3): every column walks its own list of edge values, the lists cycled
    over the rows"""
    pos = np.array([0, 2047.99, 2048, -2048, -2048.01, 2050.5, -4000.25, 2 ** 19, -2 ** 19, 2 ** 19 + 1, 524287.9, 3e5,
                    -7e5, 1e9, -1e9, np.nan, np.inf, -np.inf, 0.5 / 4096, 1.5 / 4096, 2.5 / 4096, -0.5 / 4096, -0.0, 1e-30], np.float32)
    opa = np.concatenate([np.array([20, -20, 20.5, -20.5, 19.999, np.inf, -np.inf, np.nan, 0, -0.0, 80, -80, 1e30], np.float32),
                          _near_byte_opacities()])
    # colour: (dc * 0.15 + 0.5) * 255 at 0 and 255 and around; scale: (s + 10) * 16 at 0 and 255
    dcv = np.array([-0.5 / 0.15, 0.5 / 0.15, -3.3333, 3.3333, -3.334, 3.334, 0, np.nan, np.inf, -np.inf, 1e-8], np.float32)
    dcv = np.concatenate([dcv, np.nextafter(dcv[:2], np.float32(np.inf)), np.nextafter(dcv[:2], np.float32(-np.inf))])
    scv = np.array([-10, 5.9375, 5.9376, 5.9374, -10.0001, -9.9999, 6, 100, -100, np.nan, np.inf, -np.inf, -3.03125], np.float32)
    quats = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0.5, 0.5, 0.5, 0.5], [0.5, -0.5, 0.5, -0.5], [0, 0, 0, 0],
                      [np.nan, 0, 0, 0], [0, np.nan, 1, 0], [1, 2, np.nan, 3], [-1, 0.2, 0.1, 0.3], [0.1, -0.9, 0.2, 0.3],
                      [0.2, 0.3, -0.95, 0.1], [0.1, 0.2, 0.3, -0.93], [np.inf, 0, 0, 0], [0, np.inf, -np.inf, 0],
                      [np.inf, np.inf, 1, 0], [-0.7071068, 0.7071068, 0, 0], [1e-20, 0, 0, 0], [3e38, 3e38, 0, 0],
                      [0.6, -0.6, 0.3, 0.3], [0, 0, -1, 1]], np.float32)
    shv = _sh_boundary_values()
    n = max(len(opa), len(shv), 256)
    t = np.zeros(n, dtype_3dgs())
    rng = np.random.default_rng(99)
    for a, f in enumerate("xyz"):
        t[f] = np.roll(np.resize(pos, n), 7 * a)
    t["opacity"] = np.resize(opa, n)
    for c in range(3):
        t[f"f_dc_{c}"] = np.roll(np.resize(dcv, n), 3 * c)
        t[f"scale_{c}"] = np.roll(np.resize(scv, n), 5 * c)
    q = np.resize(quats, (n, 4))
    for c in range(4):
        t[f"rot_{c}"] = q[:, c]
    for i in range(45):
        t[f"f_rest_{i}"] = np.roll(np.resize(shv, n), 11 * i)
    t["nx"] = rng.normal(size=n)
    return t


def case_table(spec: dict) -> np.ndarray:
    """the table of one golden case from its recorded recipe"""
    kind = spec["kind"]
    if kind == "edges":
        return edge_table()
    t = random_table(spec["n"], spec["seed"], n_rest=spec.get("n_rest", 45), opacity=spec.get("opacity", True),
                     dc=spec.get("dc", True), rgb=spec.get("rgb", False), sh_scale=spec.get("sh_scale", 0.3), sh_upto=spec.get("sh_upto"))
    return t
