"""The project's own numpy restatement of the .splat read (what gsx_splat_unpack_dev must return, bit for bit), and the builders
of the files the reader's tests decode.  Not the reference's text: the tests/golden/splat_read_ref.npz fixture ties it to the
reference's own rows (tests/test_splat_read_host.py).

A .splat file is n records of 32 bytes: 3 f32 position | 3 f32 linear scale | 4 u8 colour (r g b alpha) | 4 u8 rotation; bytes
behind the last whole record are ignored.  A row is 17 float32 (x y z nx ny nz f_dc_0..2 opacity scale_0..2 rot_0..3) and the
bytes red green blue, packed: 71 bytes."""
import hashlib

import numpy as np

RECORD = np.dtype([("pos", "<u4", (3,)), ("scale", "<f4", (3,)), ("colour", "u1", (4,)), ("rot", "u1", (4,))])
FLOATS = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2",
          "rot_0", "rot_1", "rot_2", "rot_3"]
BYTES = ["red", "green", "blue"]
F = np.float32


def sha(rows) -> bytes:
    return hashlib.sha256(np.ascontiguousarray(rows).view(np.uint8).reshape(-1).tobytes()).digest()


def define_dtype() -> np.dtype:
    return np.dtype([(f, "<f4") for f in FLOATS] + [(f, "u1") for f in BYTES])


def f_dc_of(b):
    """colour byte -> f_dc, every step float32"""
    return (b.astype(F) / F(255.0) - F(0.5)) / F(0.28209479177387814)


def opacity_of(b):
    """alpha byte -> logit, every step float32: the clip to [1 / 255, 0.9999] keeps the log's argument positive and finite"""
    a = b.astype(F) / F(255.0)
    a = np.minimum(np.maximum(a, F(1.0 / 255.0)), F(0.9999))
    return -np.log(F(1.0) / a - F(1.0))


def log_scale_of(s):
    """float32 linear scale -> np.log of max(s, 1e-6) where a NaN goes through the maximum"""
    s = np.asarray(s, F)
    with np.errstate(all="ignore"):
        clamped = np.where(np.isnan(s), s, np.where(s > F(1e-6), s, F(1e-6)))
        return np.log(clamped)


def rotation_of(b):
    """uint8[n, 4] -> float32[n, 4]: (b - 128) / 128 renormalised (the norm clamped at 1e-6: all four bytes 128)"""
    q = (b.astype(np.int32) - 128).astype(F) * F(0.0078125)
    ss = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]
    norm = np.sqrt(ss)
    assert norm.dtype == F
    norm = np.where(norm > F(1e-6), norm, F(1e-6))
    return q / norm[:, None]


def decode(raw, n: int) -> np.ndarray:
    """the first 32 n bytes of `raw` -> the n rows"""
    recs = np.frombuffer(raw, RECORD, n)
    rows = np.zeros(n, define_dtype())
    for a, f in enumerate("xyz"):
        rows[f].view(np.uint32)[:] = recs["pos"][:, a]                  # the file's bits
    for a in range(3):
        rows["scale_%d" % a] = log_scale_of(recs["scale"][:, a])
        rows["f_dc_%d" % a] = f_dc_of(recs["colour"][:, a])
    rows["opacity"] = opacity_of(recs["colour"][:, 3])
    rot = rotation_of(recs["rot"])
    for a in range(4):
        rows["rot_%d" % a] = rot[:, a]
    return rows


def read(path: str) -> np.ndarray:
    with open(path, "rb") as f:
        raw = f.read()
    return decode(raw, len(raw) // RECORD.itemsize)


# ---- file builders ----

def write_file(path, records: bytes, trailing: int = 0) -> str:
    with open(path, "wb") as f:
        f.write(records)
        f.write(bytes(range(1, trailing + 1)))
    return path


def random_records(n: int, rng) -> bytes:
    """random bytes in every slot: NaN, negative, huge and denormal positions and scales among them"""
    return rng.integers(0, 256, n * RECORD.itemsize, dtype=np.uint8).tobytes()


def realistic_records(n: int, rng) -> bytes:
    """a scene's values: positions of a few units, scales exp(N(-4.5, 1.5)), unit quaternions quantised as the writers do"""
    recs = np.zeros(n, RECORD)
    recs["pos"] = (rng.standard_normal((n, 3)) * 3.0).astype(F).view(np.uint32)
    recs["scale"] = np.exp(rng.normal(-4.5, 1.5, (n, 3))).astype(F)
    recs["colour"] = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    recs["rot"] = np.clip(q * 128 + 128, 0, 255).astype(np.uint8)
    return recs.tobytes()


def build_file(path, n: int, rng, trailing: int = 0) -> str:
    return write_file(path, random_records(n, rng), trailing)


ROT_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def pattern_records() -> bytes:
    """6 x 65 536 records: block p holds every pair of bytes in the rotation slots ROT_PAIRS[p] with the other two slots at 128;
    every colour and alpha slot walks all 256 values; the positions are raw bit patterns (signalling NaNs, denormals)"""
    n = 6 * 65536
    i = np.arange(n, dtype=np.uint32)
    recs = np.zeros(n, RECORD)
    recs["rot"] = 128
    for p, (a, b) in enumerate(ROT_PAIRS):
        blk = slice(65536 * p, 65536 * (p + 1))
        recs["rot"][blk, a] = (i[blk] & 0xFF).astype(np.uint8)
        recs["rot"][blk, b] = ((i[blk] >> 8) & 0xFF).astype(np.uint8)
    recs["colour"][:, 0] = i & 0xFF
    recs["colour"][:, 1] = (i >> 8) & 0xFF
    recs["colour"][:, 2] = (i * 7 + 3) & 0xFF
    recs["colour"][:, 3] = (i * 13 + 5) & 0xFF
    for a in range(3):
        recs["pos"][:, a] = (i + np.uint32(a)) * np.uint32(0x9E3779B1)
    recs["scale"] = np.exp(((i[:, None] * np.uint32(2654435761) + np.arange(3, dtype=np.uint32)) % 2000).astype(np.float64) / 100.0 - 14.0).astype(F)
    return recs.tobytes()


def pattern_file(path) -> str:
    return write_file(path, pattern_records())


def scale_records(vector) -> bytes:
    """every input of `vector` (float32) in each of the three scale slots, at different rows"""
    v = np.ascontiguousarray(vector, F)
    recs = np.zeros(len(v), RECORD)
    recs["rot"] = np.array([128, 200, 90, 17], np.uint8)
    for a, shift in enumerate((0, 1237, 40001)):
        recs["scale"][:, a] = np.roll(v, shift)
    return recs.tobytes()


def scale_file(path, vector) -> str:
    return write_file(path, scale_records(vector))


def edge_scale_records() -> bytes:
    """NaNs of both signs and kinds, +-inf, negative, +-0, denormal and clamp-edge scales, one per slot and row"""
    bits = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0,
                     0x00000001, 0x007FFFFF, 0x00800000, 0x80000001, 0xBF800000, 0xC2F00000, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F800000,
                     0x358637BD, 0x358637BC, 0x358637BE, 0x3F3504F3, 0x3F3504F2, 0x3F3504F4, 0x3FB504F3, 0x3A83126F, 0x41200000],
                    np.uint32).view(F)
    recs = np.zeros(3 * len(bits), RECORD)
    recs["scale"] = F(0.01)
    recs["rot"] = np.array([255, 0, 128, 127], np.uint8)
    for a in range(3):
        recs["scale"][a * len(bits):(a + 1) * len(bits), a] = bits
    recs["colour"][:, 3] = np.arange(len(recs)) * 3
    return recs.tobytes()


def all_128_records(n: int, rng) -> bytes:
    """rotation bytes all 128 (the clamped norm) on every other row, one byte off 128 on the rest"""
    recs = np.frombuffer(bytearray(realistic_records(n, rng)), RECORD)
    recs["rot"] = 128
    recs["rot"][1::2, 0] = 129
    recs["rot"][3::4, 3] = 127
    return recs.tobytes()
