"""A numpy restatement of the .ksplat file (both headers + payload) and the deterministic tables the ksplat tests run on.

The restatement is the checker where the reference is absent (the GPU box: tests/test_ksplat_gpu.py, and
tests/devtools/check_ksplat_large.py at 10M and 50M rows).  It states the format from its description -- a 4096-byte file
header, a 1024-byte section header, [u32 N % bucket_size], [bucket centres], N interleaved rows -- with numpy's float32
arithmetic and numpy's own casts, and is itself checked against the reference's files in tests/golden/ksplat_ref.npz
(tests/test_ksplat_host.py).
"""
from __future__ import annotations

import struct

import numpy as np

from spz_numpy import dtype_3dgs, random_table  # noqa: F401  (the same 3DGS tables)

F = np.float32
SH_C0 = 0.28209479177387814


# ------------------------------------------------------------------------------------------------------------ format
def options(level=0, sh_level=None, bucket_size=None, block_size=None):
    """the writer's keyword conversions -> (level, sh_level, bucket_size, block_size)"""
    return (int(level), None if sh_level is None else int(sh_level), 256 if bucket_size is None else int(bucket_size),
            5.0 if block_size is None else float(block_size))


def sh_degree(data: np.ndarray, sh_level=None) -> int:
    """1 if a present f_rest_0..8 holds a value != 0 (NaN counts, -0.0 does not), 2 if a present f_rest_9..23 does too; then at
    most sh_level"""
    names = data.dtype.names

    def any_nonzero(idx):
        return any(f"f_rest_{j}" in names and np.count_nonzero(data[f"f_rest_{j}"]) for j in idx)
    d = (2 if any_nonzero(range(9, 24)) else 1) if any_nonzero(range(9)) else 0
    return sh_level if sh_level is not None and sh_level < d else d


def n_sh(degree: int) -> int:
    return {1: 9, 2: 24}.get(degree, 0)


def row_dtype(level: int, sh_count: int) -> np.dtype:
    big = level == 0
    item = "<f4" if big else "<f2"
    fields = [("pos", "<f4" if big else "<u2", (3,)), ("scale", item, (3,)), ("rot", item, (4,)), ("color", "u1", (4,))]
    if sh_count:
        fields.append(("sh", "<f4" if big else ("<f2" if level == 1 else "u1"), (sh_count,)))
    return np.dtype(fields)


def heads(n, level, bucket_size, block_size, degree):
    """(file header, section header, leading payload word, bucket count); struct raises as the writer's does"""
    h = bytearray(4096)
    h[1] = 1
    struct.pack_into("<IIIIH", h, 4, 1, 1, n, n, level)
    struct.pack_into("<ff", h, 36, -2.0, 2.0)
    s = bytearray(1024)
    struct.pack_into("<II", s, 0, n, n)
    if level >= 1:
        struct.pack_into("<II", s, 8, bucket_size, -(-n // bucket_size))
        struct.pack_into("<fHxxI", s, 16, block_size, 12, 32767)
    sc = n_sh(degree)
    bps = (12 + 12 + 16 + 4 + 4 * sc) if level == 0 else (6 + 6 + 8 + 4 + (2 if level == 1 else 1) * sc)
    part = int(n % bucket_size != 0)
    nb = n // bucket_size + part
    struct.pack_into("<III", s, 28, 4 * part + (12 * nb if level >= 1 else 0) + n * bps, n // bucket_size, part)
    struct.pack_into("<H", s, 40, degree)
    return bytes(h), bytes(s), struct.pack("<I", n % bucket_size) if part else b"", nb


def centres(data: np.ndarray, bucket_size: int) -> np.ndarray:
    """(n_buckets, 3) float32: (min + max) / 2 of x, y, z over every bucket of bucket_size consecutive rows"""
    starts = np.arange(0, len(data), bucket_size)
    with np.errstate(all="ignore"):
        return np.column_stack([(np.minimum.reduceat(data[a], starts) + np.maximum.reduceat(data[a], starts)) / 2.0
                                for a in "xyz"]).astype(F)


def rows(data: np.ndarray, level: int, sh_count: int, cen=None, bucket_size=1, block_size=5.0, first_row=0) -> np.ndarray:
    """the interleaved rows of `data` (row i of data is row first_row + i of the table; cen: the table's centres)"""
    n = len(data)
    out = np.zeros(n, row_dtype(level, sh_count))
    xyz = np.column_stack([data[a] for a in "xyz"])
    with np.errstate(all="ignore"):
        if level == 0:
            out["pos"] = xyz
        else:
            per_row = cen[(first_row + np.arange(n)) // bucket_size]
            sf = 32767 / (block_size / 2.0)
            out["pos"] = np.clip(np.round((xyz - per_row) * sf) + 32767, 0, 65535).astype(np.uint16)
        dt = out.dtype["scale"].base
        out["scale"] = np.column_stack([np.exp(data[f"scale_{a}"]) for a in range(3)]).astype(dt)
        out["rot"] = np.column_stack([data[f"rot_{a}"] for a in range(4)]).astype(dt)
        col = [np.clip((0.5 + SH_C0 * data[f"f_dc_{a}"]) * 255, 0, 255).astype(np.uint8) for a in range(3)]
        col.append(np.clip((1 / (1 + np.exp(-data["opacity"]))) * 255, 0, 255).astype(np.uint8))
        out["color"] = np.column_stack(col)
        if sh_count:
            sh = np.column_stack([data[f"f_rest_{j}"] for j in range(sh_count)])
            if level == 2:                           # only level 2 quantises; levels >= 3 cast the values themselves
                out["sh"] = np.clip((sh + 2.0) / 4.0 * 255, 0, 255).astype(np.uint8)
            else:
                out["sh"] = sh.astype(out.dtype["sh"].base)
    return out


def file_bytes(data: np.ndarray, level=0, **kw) -> bytes:
    """the whole .ksplat file; raises what the writer raises (struct.error, ZeroDivisionError, numpy's ValueError)"""
    level, sh_level, bs, blk = options(level, **kw)
    n = len(data)
    degree = sh_degree(data, sh_level)
    h, s, word, nb = heads(n, level, bs, blk, degree)
    for a in "xyz":
        data[a]
    cen = None
    if level >= 1:
        cen = centres(data, bs) if n else np.zeros((0, 3), F)
        32767 / (blk / 2.0)                     # ZeroDivisionError for a zero block size
    for f in ["scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3", "f_dc_0", "f_dc_1", "f_dc_2", "opacity"]:
        data[f]
    for j in range(n_sh(degree)):
        data[f"f_rest_{j}"]
    body = rows(data, min(level, 3), n_sh(degree), cen, bs, blk)
    return h + s + word + (cen.tobytes() if level >= 1 else b"") + body.tobytes()


# ------------------------------------------------------------------------------------------------------------ tables
EXP_HARD = np.array([0xC2781E37], np.uint32).view(np.float32)[0]   # a worst case of numpy's exp


def edge_table() -> np.ndarray:
    """explicit edge rows (248-byte 3DGS rows): every column walks its own list of edge values; rows 14-20 (bucket 2 of 7), 21-27
    and 28-34 hold only zeros in x (both signs / only -0 / only +0), rows 256-511 only zeros of both signs in y, row 40's x is
    NaN and rows 41-42 put -inf and +inf into one bucket of 7 (a NaN centre)"""
    f = np.float32
    pos = np.array([0, -0.0, 1.5, -2.25, 1e9, -1e9, 3e38, -3e38, 1e-40, -1e-40, 2.5, 2.4999, 7.0, -7.0, 0.37, 1e5, -1e5, 65535,
                    np.nan, np.inf, -np.inf], f)
    scale = np.array([0, -0.0, 1, -1, 11.089, 11.0904, 12, 20, 88.7228, 88.72284, 89, -9.7, -16.6, -17.3, -24, -87.4, -103.97,
                      -104, np.nan, np.inf, -np.inf, EXP_HARD, 1e-40, -4.5, -6.2], f)
    opa = np.array([0, -0.0, 100, -100, 88.8, -88.8, 104, -104, 1e-40, np.nan, np.inf, -np.inf, EXP_HARD, 5.5, -5.5, 2.0, -2.0,
                    0.0039, 17.3], f)
    dc = np.array([0, -0.0, -1.7724539, 1.7724539, -1.77245, 1.77246, 5, -5, np.nan, np.inf, -np.inf, 1e-40, 0.1, -0.1], f)
    rot = np.array([1, 0, -0.0, 0.5, -0.5, 65504, 65519, 65520, -65520, 1e5, 6.1e-5, 6e-8, 2.9e-8, 3e-8, 1e-40, np.nan, np.inf,
                    -np.inf, 0.33333334, 2049, 2051], f)
    sh = np.array([0, -0.0, -2, 2, -2.0000002, 2.0000002, -1.9921875, 1.9921875, 0.5, -0.5, 6e-8, 65520, -65520, 1e-40, np.nan,
                   np.inf, -np.inf, 0.0157, 1.234567, -0.1], f)
    n = 512
    t = np.zeros(n, dtype_3dgs())
    for a, nm in enumerate("xyz"):
        t[nm] = np.roll(np.resize(pos, n), 5 * a)
    for c in range(3):
        t[f"scale_{c}"] = np.roll(np.resize(scale, n), 3 * c)
        t[f"f_dc_{c}"] = np.roll(np.resize(dc, n), 4 * c)
    for c in range(4):
        t[f"rot_{c}"] = np.roll(np.resize(rot, n), 6 * c)
    t["opacity"] = np.resize(opa, n)
    for i in range(45):
        t[f"f_rest_{i}"] = np.roll(np.resize(sh, n), 7 * i)
    t["x"][14:21] = np.array([0, -0.0, 0, -0.0, -0.0, 0, 0], f)
    t["x"][21:28] = -0.0
    t["x"][28:35] = 0.0
    t["x"][35:42] = 1.0
    t["x"][40] = np.nan
    t["x"][42:49] = np.array([2.0, -np.inf, np.inf, 1.0, 0.0, 3.0, 4.0], f)
    t["y"][256:512] = np.where(np.arange(256) % 3 == 1, f(-0.0), f(0.0))
    t["nx"] = np.random.default_rng(5).normal(size=n)
    return t


def ties_table() -> np.ndarray:
    """positions at exact rint ties for block_size 63.998046875 (sf_inv = 1024): bucket centres 0, x = (k + 0.5) / 1024"""
    t = random_table(256, 41)
    k = np.arange(256) - 128
    for nm in "xyz":
        v = ((k + 0.5) / 1024).astype(np.float32)
        v[0], v[1] = -0.5, 0.5                       # min / max of the one bucket: centre 0
        t[nm] = v
    return t


def case_table(spec: dict) -> np.ndarray:
    """the table of one golden case from its recorded recipe"""
    kind = spec["kind"]
    if kind == "edges":
        return edge_table()
    if kind == "ties":
        return ties_table()
    t = random_table(spec["n"], spec["seed"], n_rest=spec.get("n_rest", 45), rgb=spec.get("rgb", False),
                     sh_scale=spec.get("sh_scale", 0.3), sh_upto=spec.get("sh_upto"))
    if "drop" in spec:                               # a table that lacks one field
        import numpy.lib.recfunctions as rfn
        t = rfn.repack_fields(t[[f for f in t.dtype.names if f != spec["drop"]]])
    return t


def case_kwargs(spec: dict) -> dict:
    return dict(spec.get("kw", {}))
