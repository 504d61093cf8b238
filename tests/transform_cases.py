"""What tests/test_transform_host.py and tests/test_transform_gpu.py share, computed on the CPU: packed splat dtypes at the strides
of the issue, small seeded tables with the edge rows planted in front, and the five kinds of transform."""
import importlib

import numpy as np

tf = importlib.import_module("3dgsconverter_amd.transform")

F4 = np.dtype("<f4")
STRIDES = (56, 68, 71, 104, 107, 167, 248, 251, 300)


def splat_dtype(stride: int) -> np.dtype:
    """A packed dtype of `stride` bytes.  56: degree 0 without normals; 68: with normals; 71: a u1 tag in FRONT of them (every
    float field at an unaligned byte) and two u1 behind; 104 / 107: degree 1 (+ rgb); 167: degree 2 + rgb; 248: the 3DGS row;
    251: + rgb; 300: 248 bytes + 52 bytes of extra fields of other types (rows of more than 256 bytes: tiles of 64 rows)"""
    degree = {56: 0, 68: 0, 71: 0, 104: 1, 107: 1, 167: 2, 248: 3, 251: 3, 300: 3}[stride]
    n_rest = {0: 0, 1: 9, 2: 24, 3: 45}[degree]
    names = ["x", "y", "z"] + ([] if stride == 56 else ["nx", "ny", "nz"]) + ["f_dc_0", "f_dc_1", "f_dc_2"]
    names += ["f_rest_%d" % i for i in range(n_rest)] + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    fields = [(nm, "<f4") for nm in names]
    if stride == 71:
        fields = [("tag", "u1")] + fields + [("b0", "u1"), ("b1", "u1")]
    elif stride in (107, 167, 251):
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    elif stride == 300:
        fields += [("label", "<i8")] + [("extra_%d" % i, "<f4") for i in range(10)] + [("flag_%d" % i, "u1") for i in range(4)]
    dt = np.dtype(fields)
    assert dt.itemsize == stride, (stride, dt.itemsize)
    return dt


def frame_fields(dtype: np.dtype):
    """the fields a transform may write"""
    return [nm for nm in dtype.names if nm in ("x", "y", "z", "nx", "ny", "nz") or nm.startswith(("scale_", "rot_", "f_rest_"))]


def float_fields(dtype: np.dtype):
    return [nm for nm in dtype.names if dtype[nm] == F4]


def edge_rows(dtype: np.dtype) -> np.ndarray:
    """the planted rows: zeros of both signs, float32 denormals, values whose results are denormal (under a scale below 1) and
    whose results overflow (under a scale above 1, or in a sum), then one row with a NaN and one with an infinity in each
    field a transform writes.  Random bytes elsewhere."""
    ff = frame_fields(dtype)
    rng = np.random.default_rng(7)
    t = random_rows(dtype, 5 + 2 * len(ff), rng)
    for nm in ff:
        t[nm][0] = 0.0
        t[nm][1] = -0.0
        t[nm][2] = np.float32(1e-40) if len(nm) % 2 else np.float32(-3e-45)
        t[nm][3] = np.float32(2.5e-38) if len(nm) % 2 else np.float32(-1.3e-38)
        t[nm][4] = np.float32(3.1e38) if len(nm) % 2 else np.float32(-2.9e38)
    nan_payload = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x7fc00000], np.uint32).view(np.float32)
    for k, nm in enumerate(ff):
        t[nm][5 + 2 * k] = nan_payload[k % 4]
        t[nm][6 + 2 * k] = np.inf if k % 2 else -np.inf
    return t


def random_rows(dtype: np.dtype, n: int, rng) -> np.ndarray:
    """n rows: standard normal float fields, random bytes in every other field"""
    t = rng.integers(0, 256, (n, dtype.itemsize), dtype=np.uint8).reshape(-1).view(dtype).copy()
    for nm in float_fields(dtype):
        t[nm] = rng.standard_normal(n).astype(np.float32)
    return t


def table(stride: int, n: int, seed: int = 0) -> np.ndarray:
    """n rows of splat_dtype(stride): the edge rows in front (as many as fit), seeded random rows behind them"""
    dt = splat_dtype(stride)
    t = random_rows(dt, n, np.random.default_rng(1000 * stride + n + seed))
    e = edge_rows(dt)
    k = min(n, len(e))
    t[:k] = e[:k]
    return t


def transforms():
    """{name: (R or None, s or None, t or None)}: the five kinds"""
    R = tf.rotation_from_euler_deg(25.0, -40.0, 70.0)
    return {
        "rotation": (R, None, None),
        "scale_up": (None, 2.5, None),
        "translation": (None, None, (0.5, -1.25, 3.0)),
        "all_three": (tf.rotation_from_euler_deg(-130.0, 15.5, 200.0), 0.37, (-4.0, 0.125, 1e-3)),
        "quarter_turn": (tf.rotation_from_euler_deg(-90.0, 0.0, 0.0), None, None),
    }


def capped_names(dtype: np.dtype, degree: int):
    """cap_sh_degree's columns (data_processor.py:310-313): f_rest_i from 0 / 9 / 24 on"""
    start = {0: 0, 1: 9, 2: 24}[degree]
    return [nm for nm in ("f_rest_%d" % i for i in range(start, 45)) if nm in dtype.names]
