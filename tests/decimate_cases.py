"""What tests/test_decimate_host.py and tests/test_decimate_gpu.py share, computed on the CPU: packed splat dtypes at the strides of
the issue, seeded scenes whose rows fall into voxels of chosen sizes, the rows the merge cannot use, and an independent two-pass
computation of a group's moments."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transform_cases as tc  # noqa: E402

H = 0.25                        # the scenes' voxel size: a power of two, so a multiple of it is a float32 on a cell face
STRIDES = (68, 104, 164, 248, 251, 300)
MIXED_SIZES = (1, 2, 1, 3, 300, 1, 17, 257, 1, 64, 5, 256, 1, 255, 2, 9)


def splat_dtype(stride: int) -> np.dtype:
    """68 / 104 / 248: degrees 0 / 1 / 3 with normals; 164: degree 2 with normals; 251: degree 3 with normals and colours; 300:
    normals and 52 bytes of extra fields of other types (transform_cases.splat_dtype)"""
    if stride != 164:
        return tc.splat_dtype(stride)
    names = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + ["f_rest_%d" % i for i in range(24)]
    names += ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    dt = np.dtype([(nm, "<f4") for nm in names])
    assert dt.itemsize == 164
    return dt


def group_sizes(n: int, shape: str):
    """the sizes of the scene's voxels, in the order of their cells"""
    if shape == "singletons":
        return [1] * n
    if shape == "one_cell":
        return [n] if n else []
    sizes, k = [], 0
    while sum(sizes) < n:
        sizes.append(min(MIXED_SIZES[k % len(MIXED_SIZES)], n - sum(sizes)))
        k += 1
    return sizes


def cell_of(g: int):
    """the g-th cell of a scene: a lattice walk through negative and positive indices, no cell twice"""
    return (g % 11 - 5, (g // 11) % 11 - 5, g // 121 - 3)


def scene(stride: int, n: int, shape: str = "mixed", seed: int = 0, on_faces: bool = False, max_alpha: float = 0.4) -> np.ndarray:
    """n mergeable rows of splat_dtype(stride) in voxels of side H with group_sizes(n, shape) members, the rows shuffled so that
    a voxel's members are interleaved with the others'.  Log-scales in (-7, -4.5), opacities of alpha in (0.05, max_alpha),
    random unit-free quaternions, standard normal SH and normals, random bytes elsewhere.  on_faces: every coordinate is a
    multiple of H (a point on three cell faces), negative ones included."""
    dt = splat_dtype(stride)
    rng = np.random.default_rng(7919 * stride + 31 * n + seed)
    t = tc.random_rows(dt, n, rng)
    sizes = group_sizes(n, shape)
    cells = np.repeat(np.array([cell_of(g) for g in range(len(sizes))], np.float64).reshape(-1, 3), sizes, axis=0)
    u = np.zeros((n, 3)) if on_faces else rng.uniform(0.05, 0.95, (n, 3))
    pos = ((cells + u) * H).astype(np.float32)
    perm = rng.permutation(n)
    for a, nm in enumerate("xyz"):
        t[nm] = pos[perm, a]
    for i in range(3):
        t["scale_%d" % i] = rng.uniform(-7.0, -4.5, n).astype(np.float32)
    alpha = rng.uniform(0.05, max_alpha, n)
    t["opacity"] = np.log(alpha / (1.0 - alpha)).astype(np.float32)
    return t


UNMERGEABLE = ("nan_x", "inf_y", "neg_inf_z", "w_zero", "w_inf", "w_nan", "zero_quat", "nan_quat")


def plant_unmergeable(t: np.ndarray, every: int = 7) -> np.ndarray:
    """a copy with every `every`-th row made a row of one of the UNMERGEABLE kinds, in turn -> (table, the planted rows)"""
    t = t.copy()
    rows = np.arange(3, len(t), every)
    for k, r in enumerate(rows):
        kind = UNMERGEABLE[k % len(UNMERGEABLE)]
        if kind == "nan_x":
            t["x"][r] = np.nan
        elif kind == "inf_y":
            t["y"][r] = np.inf
        elif kind == "neg_inf_z":
            t["z"][r] = -np.inf
        elif kind == "w_zero":
            t["opacity"][r] = -200.0            # E(200) = inf, 1 / (1 + inf) = 0
        elif kind == "w_inf":
            t["scale_0"][r] = t["scale_1"][r] = t["scale_2"][r] = 40.0
        elif kind == "w_nan":
            t["scale_1"][r] = np.nan
        elif kind == "zero_quat":
            for i in range(4):
                t["rot_%d" % i][r] = 0.0 if i % 2 else -0.0
        else:
            t["rot_2"][r] = np.nan
    return t, rows


def plant_nonfinite_sh(t: np.ndarray, every: int = 5) -> np.ndarray:
    """a copy with a NaN, an infinity or a NaN of another payload in an SH field of every `every`-th row (the rows stay mergeable)"""
    t = t.copy()
    names = [nm for nm in t.dtype.names if nm.startswith(("f_dc_", "f_rest_"))]
    vals = np.array([0x7fc00000, 0x7f800000, 0xffc12345, 0xff800000], np.uint32).view(np.float32)
    for k, r in enumerate(range(1, len(t), every)):
        t[names[k % len(names)]][r] = vals[k % 4]
    return t


def two_pass_moments(pos, w, C):
    """independent of the definition's shifted one-pass sums: pos (k, 3), w (k,), C (k, 3, 3) float64 -> (mean, covariance) with
    the mean computed first and the deviations taken from it"""
    W = np.sum(w)
    mu = np.sum(w[:, None] * pos, axis=0) / W
    d = pos - mu
    Sig = np.sum(w[:, None, None] * (C + d[:, :, None] * d[:, None, :]), axis=0) / W
    return mu, Sig


def member_covariances(t: np.ndarray) -> np.ndarray:
    """(k, 3, 3) float64: R diag(exp(scale)^2) R^T with numpy's own float64 exp and matrix products"""
    q = np.stack([t["rot_%d" % i].astype(np.float64) for i in range(4)], axis=1)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.empty((len(t), 3, 3))
    R[:, 0] = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], axis=1)
    R[:, 1] = np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], axis=1)
    R[:, 2] = np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)
    s = np.stack([t["scale_%d" % i] for i in range(3)], axis=1)
    e = np.stack([_lib().np_exp_host(np.ascontiguousarray(s[:, i])).astype(np.float64) for i in range(3)], axis=1)   # (csrc/np_exp.h's float32 exp)
    return np.einsum("kij,kj,klj->kil", R, e * e, R)


def _lib():
    import importlib
    return importlib.import_module("3dgsconverter_amd._lib")


def survivor_list(n0: int, n: int, seed: int = 0) -> np.ndarray:
    """n ascending uint32 rows of [0, n0)"""
    return np.sort(np.random.default_rng(n0 + seed).choice(n0, n, replace=False)).astype(np.uint32)
