"""The SPZ reader restated in numpy (gsconverter/formats/spz.py:18-47, :175-296), and builders of .spz files.

``read`` is checked against the reference's recorded rows on every case of tests/golden/spz_read_ref.npz
(tests/test_spz_read_host.py), which licenses it as the checker at sizes the golden file cannot hold.  It runs on the host's
numpy alone and keeps the reference's operand dtypes where they decide a bit: float32 throughout, except the scale (float64,
rounded on assignment) and the version-3 rotation (float64 from the sign factor on, rounded on assignment).
"""
import gzip
import hashlib
import struct

import numpy as np

MAGIC = 0x5053474E
HEADER = "<IIIBBBB"
SH_DIM = {0: 0, 1: 3, 2: 8, 3: 15}
POS_BYTES = {1: 6, 2: 9, 3: 9}
ROT_BYTES = {1: 3, 2: 3, 3: 4}
BASE_BEFORE = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
BASE_AFTER = ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]


def sha(rows) -> bytes:
    return hashlib.sha256(np.ascontiguousarray(rows).view(np.uint8).tobytes()).digest()


def n_coeffs(degree: int) -> int:
    return 3 * ((degree + 1) ** 2 - 1)


def define_dtype(degree: int) -> np.dtype:
    """structures.py:23-59 with has_scal=False, has_rgb=True"""
    return np.dtype([(f, "f4") for f in BASE_BEFORE] + [("f_rest_%d" % i, "f4") for i in range(n_coeffs(degree))]
                    + [(f, "f4") for f in BASE_AFTER] + [(f, "u1") for f in ("red", "green", "blue")])


def section_bytes(version: int, degree: int):
    """bytes per row of positions, alpha, colour, scale, rotation, sh"""
    return (POS_BYTES[version], 1, 3, 3, ROT_BYTES[version], 3 * SH_DIM.get(degree, 0))


def body_bytes(version: int, degree: int, n: int) -> int:
    return n * sum(section_bytes(version, degree))


# ---- per-code results (what the device takes from tables)
def opacity_of(b):
    a = np.clip(b.astype(np.float32) / 255.0, 1e-7, 1.0 - 1e-7)
    return np.log(a / (1.0 - a))


def f_dc_of(b):
    return (b.astype(np.float32) / 255.0 - 0.5) / 0.15


def colour_byte_of(f_dc):
    return np.clip((0.5 + 0.28209479177387814 * f_dc) * 255.0, 0, 255).astype(np.uint8)


def scale_of(b):
    return b / 16.0 - 10.0                       # float64


def sh_of(b):
    return (b.astype(np.float32) - 128.0) / 128.0


def legacy_component_of(b):
    return b.astype(np.float32) / 127.5 - 1.0


def v3_component_of(c):
    """float64: the float32 magnitude times a float64 sign (uint32 array times a Python float)"""
    mag, neg = c & 0x1FF, (c >> 9) & 0x1
    return (mag.astype(np.float32) / 511.0) * 0.707106781186547524401 * (1.0 - 2.0 * neg)


def legacy_rotation(raw):
    """raw uint8 [n, 3] -> w, x, y, z (float32)"""
    xyz = legacy_component_of(raw)
    sq = xyz * xyz
    w = np.sqrt(np.maximum(np.float32(0), np.float32(1) - ((sq[:, 0] + sq[:, 1]) + sq[:, 2])))
    return w, xyz[:, 0], xyz[:, 1], xyz[:, 2]


def v3_rotation(packed):
    """packed uint32 [n] -> w, x, y, z (float32)"""
    n = len(packed)
    idx = (packed >> 30) & 3
    v = [v3_component_of((packed >> s) & 0x3FF) for s in (20, 10, 0)]
    largest = np.sqrt(np.maximum(0.0, 1.0 - ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])))
    comps = np.zeros((4, n), np.float32)         # X Y Z W
    for i in range(4):
        m = idx == i
        comps[i][m] = largest[m]
        for slot, j in enumerate(j for j in range(4) if j != i):
            comps[j][m] = v[slot][m]
    return comps[3], comps[0], comps[1], comps[2]


def decode(raw: bytes, version: int, n: int, degree: int, bits: int) -> np.ndarray:
    """spz.py:175-251 on the bytes behind the header"""
    out = np.zeros(n, define_dtype(degree))
    per = section_bytes(version, degree)
    starts = np.concatenate([[0], np.cumsum([n * p for p in per])]).astype(np.int64)
    sec = [np.frombuffer(raw, np.uint8, n * per[k], int(starts[k])) for k in range(6)]
    with np.errstate(all="ignore"):
        if version == 1:
            pos = sec[0].view(np.float16).reshape(n, 3).astype(np.float32)
        else:
            b = sec[0].reshape(n, 3, 3).astype(np.int32)
            i = b[:, :, 0] | (b[:, :, 1] << 8) | (b[:, :, 2] << 16)
            i = np.where(i & 0x800000, i | -16777216, i).astype(np.int32)
            pos = i.astype(np.float32) / (1 << bits)
        for a, f in enumerate("xyz"):
            out[f] = pos[:, a]
        out["opacity"] = opacity_of(sec[1])
        col, sc = sec[2].reshape(n, 3), sec[3].reshape(n, 3)
        for a in range(3):
            dc = f_dc_of(col[:, a])
            out["f_dc_%d" % a] = dc
            out[("red", "green", "blue")[a]] = colour_byte_of(dc)
            out["scale_%d" % a] = scale_of(sc[:, a])
        if version >= 3:
            quat = v3_rotation(sec[4].view(np.uint32))
        else:
            quat = legacy_rotation(sec[4].reshape(n, 3))
        for a in range(4):
            out["rot_%d" % a] = quat[a]
        dim = SH_DIM.get(degree, 0)
        if dim:
            sh = sh_of(sec[5].reshape(n, dim, 3))
            for j in range(dim):
                for ch in range(3):
                    out["f_rest_%d" % (j + ch * dim)] = sh[:, j, ch]
    return out


def read(path: str) -> np.ndarray:
    """spz.py:18-47"""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) > 2 and data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    if len(data) < 16:
        raise ValueError("Decompressed SPZ data too short for header")
    magic, version, n, degree, bits, _, _ = struct.unpack(HEADER, data[:16])
    if magic != MAGIC:
        raise ValueError("Invalid SPZ magic number: %s" % hex(magic))
    if not 1 <= version <= 3:
        raise ValueError("Unsupported SPZ version: %d" % version)
    return decode(data[16:], version, n, degree, bits)


# ---- file builders
def header(version, n, degree, bits=12, flags=0, reserved=0) -> bytes:
    return struct.pack(HEADER, MAGIC, version, n, degree, bits, flags, reserved)


def wrap(payload: bytes, gzip_level=0) -> bytes:
    """gzip_level None: the payload as it is (the reader takes an un-gzipped file too)"""
    return payload if gzip_level is None else gzip.compress(payload, compresslevel=gzip_level, mtime=0)


def write_file(path, version, degree, n, body: bytes, bits=12, gzip_level=0, **head) -> str:
    with open(path, "wb") as f:
        f.write(wrap(header(version, n, degree, bits, **head) + body, gzip_level))
    return path


def random_body(version, degree, n, rng) -> bytes:
    """random bytes in every section; version-1 positions are random float16 patterns, NaNs included"""
    return rng.integers(0, 256, body_bytes(version, degree, n), dtype=np.uint8).tobytes()


def build_file(path, version, degree, n, rng, frac_bits=12, gzip_level=0) -> str:
    return write_file(path, version, degree, n, random_body(version, degree, n, rng), frac_bits, gzip_level)


def pattern_body(version, degree=3, n=65536) -> bytes:
    """65 536 rows that hold every byte value in every byte slot of every section, and: version 1, every float16 pattern in
    each position slot; version >= 2, 24-bit positions at +-1, +-(2^23 - 1) and -2^23; version 3, every 10-bit component in
    each rotation slot with each idx."""
    assert n == 65536
    i = np.arange(n, dtype=np.uint32)
    per = section_bytes(version, degree)
    secs = []
    for k, p in enumerate(per):
        s = np.zeros((n, p), np.uint8)
        for a in range(p):
            s[:, a] = (i * (2 * a + 1) + 37 * a + 11 * k) & 0xFF    # an odd multiplier: every byte value, 256 times, per slot
        secs.append(s)
    if version == 1:
        h = secs[0].view(np.uint16)                                  # [n, 3]
        h[:, 0], h[:, 1], h[:, 2] = i, i[::-1], (i * 40503 + 7) & 0xFFFF
    else:
        edge = np.array([1, -1, (1 << 23) - 1, -(1 << 23) + 1, -(1 << 23), 0], np.int32)
        for a in range(3):
            v = edge[(np.arange(24) + a) % len(edge)].astype(np.uint32)
            for byte in range(3):
                secs[0][:24, 3 * a + byte] = (v >> (8 * byte)) & 0xFF
    if version == 3:
        # block k = i >> 10 of 1024 rows: code i & 0x3FF in slot k % 3 with idx (k // 3) % 4 -- blocks 0..11 hold all twelve pairs
        c, slot, idx = i & 0x3FF, (i >> 10) % 3, (i >> 10) // 3 % 4
        other = ((i * 2654435761) >> 7) & 0x3FF
        other2 = ((i * 40503) >> 3) & 0x3FF
        codes = np.stack([np.where(slot == 0, c, other), np.where(slot == 1, c, other2), np.where(slot == 2, c, other)], axis=1)
        packed = (idx.astype(np.uint32) << 30) | (codes[:, 0].astype(np.uint32) << 20) | (codes[:, 1].astype(np.uint32) << 10) | codes[:, 2]
        secs[4] = packed.astype("<u4").view(np.uint8).reshape(n, 4)
    return b"".join(s.tobytes() for s in secs)


def pattern_file(path, version, degree=3, frac_bits=12, gzip_level=0) -> str:
    return write_file(path, version, degree, 65536, pattern_body(version, degree), frac_bits, gzip_level)
