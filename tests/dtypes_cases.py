"""The tables of the field-dtype tests (tests/test_field_dtypes_host.py, tests/test_field_dtypes_gpu.py) and of their fixture
generator (tests/devtools/make_golden_dtypes.py -> tests/golden/dtypes_ref.npz).

Every table is a splat table (oracle.datasets.sog_scene: every field the filters and writers read) plus ``orig_index`` (i8: the
reference's filters return the surviving rows, this recovers their mask) and ``extra`` (f8: a field nothing reads, which keeps
its own dtype).  The cases differ only in the dtypes and the layout of the float fields:

  f4le       the little-endian float32 table itself
  f4be       every float32 field big-endian                      (the same numbers)
  f2         every float32 field float16                         (rounded once; the reference then computes in float16)
  f8r        every float32 field float64                         (the same numbers: float32 holds them)
  f8         every float32 field float64, x/y/z off the float32 grid
  mixed_x8   x float64 off the float32 grid, the rest float32
  mixed_x8r  x float64 holding float32 values, the rest float32
  mixed_x2   x float16, the rest float32                         (x, y, z promote to float32)
  strided    every third row of a little-endian float32 table    (a view, not C-contiguous)
  subset     the little-endian float32 table without nx/ny/nz/extra (a view: padding inside the row)

What each entry point must do with each case is stated here (ACCEPT) and checked by the tests; the adversarial tables at the
end are built so that a float32 cast changes the reference's answer.
"""
from __future__ import annotations

import numpy as np

from oracle import datasets

N = 5003                 # ragged: not a multiple of 64, 256 or 1024
N_LARGE = 70001          # >= 65536: DataProcessor's pinned-buffer gather (_xyz_rows)
CASES = ("f4le", "f4be", "f2", "f8r", "f8", "mixed_x8", "mixed_x8r", "mixed_x2", "strided", "subset")
LARGE_CASES = ("f4be", "f8r", "mixed_x2")
XYZ = ("x", "y", "z")

# the cases each entry point takes (gives the reference's answer); every other case raises TypeError
ACCEPT = {
    "sor": {"f4le", "f4be", "f2", "f8r", "mixed_x8r", "mixed_x2", "strided", "subset"},
    "density": {"f4le", "f4be", "mixed_x2", "strided", "subset"},
    "writer": {"f4le", "f4be", "strided", "subset"},          # compressed PLY, SOG
    "writer_le": {"f4le", "strided", "subset"},               # SPZ, .ksplat: little-endian float32 only
}

SOR_K, SOR_SIGMA = 8, 1.0
DENSITY_KW = {"voxel_size": 1.0, "threshold_percentage": 0.1}
ALPHA_MIN = 100
BOX = (-2.5, -3.0, -2.0, 3.0, 2.5, 1.5)


def _base(n: int, seed: int) -> np.ndarray:
    s = datasets.sog_scene(n, seed)
    dt = s.dtype.descr + [("orig_index", "<i8"), ("extra", "<f8")]
    t = np.zeros(n, dt)
    for nm in s.dtype.names:
        t[nm] = s[nm]
    t["orig_index"] = np.arange(n)
    t["extra"] = np.random.default_rng(seed + 7).standard_normal(n)
    return t


def retype(t: np.ndarray, types: dict) -> np.ndarray:
    """a packed copy of `t` with the fields named in `types` converted (numpy's cast) to the given dtypes"""
    dt = [(nm, types.get(nm, t.dtype.fields[nm][0].str)) for nm in t.dtype.names]
    out = np.zeros(len(t), dt)
    for nm in t.dtype.names:
        out[nm] = t[nm]
    return out


def float_fields(t: np.ndarray):
    return [nm for nm in t.dtype.names if t.dtype.fields[nm][0] == np.dtype("<f4")]


def _off_grid(t: np.ndarray, names, seed: int):
    """float64 x/y/z moved off the float32 grid by a relative 1e-9 (every value, so a cast rounds every one of them)"""
    rng = np.random.default_rng(seed + 11)
    for nm in names:
        v = t[nm]
        t[nm] = v + np.abs(v) * 1e-9 * rng.uniform(0.25, 1.0, len(v)) + 1e-12
    return t


def table(case: str, n: int = N, seed: int = 1) -> np.ndarray:
    if case == "strided":
        b = _base(3 * n, seed)
        b["orig_index"] //= 3                 # (row i of the view is row 3i of the table)
        return b[::3]
    b = _base(n, seed)
    ff = float_fields(b)
    if case == "f4le":
        return b
    if case == "f4be":
        return retype(b, {nm: ">f4" for nm in ff})
    if case == "f2":
        return retype(b, {nm: "<f2" for nm in ff})
    if case == "f8r":
        return retype(b, {nm: "<f8" for nm in ff})
    if case == "f8":
        return _off_grid(retype(b, {nm: "<f8" for nm in ff}), XYZ, seed)
    if case == "mixed_x8":
        return _off_grid(retype(b, {"x": "<f8"}), ("x",), seed)
    if case == "mixed_x8r":
        return retype(b, {"x": "<f8"})
    if case == "mixed_x2":
        return retype(b, {"x": "<f2"})
    if case == "subset":
        return b[[nm for nm in b.dtype.names if nm not in ("nx", "ny", "nz", "extra")]]
    raise KeyError(case)


def f4le_equivalent(t: np.ndarray) -> np.ndarray:
    """the little-endian float32 table with the same numbers, where float32 holds them (what a correct float32 path computes on)"""
    return retype(t, {nm: "<f4" for nm in t.dtype.names if t.dtype.fields[nm][0].kind == "f" and nm != "extra"})


def field_bytes(t: np.ndarray) -> bytes:
    """every field's values, field by field, with their dtypes (not the padding between them, which a copy leaves undefined)"""
    return b"".join(nm.encode() + t.dtype.fields[nm][0].str.encode() + np.ascontiguousarray(t[nm]).tobytes() for nm in t.dtype.names)


def masks_from_rows(rows: np.ndarray, n: int) -> np.ndarray:
    m = np.zeros(n, bool)
    m[np.asarray(rows["orig_index"])] = True
    return m


# ------------------------------------------------------------------------------------------------------------ adversarial
ADV_SOR = {"n": 3001, "k": 8, "sigma": 1.0, "seed": 21}
ADV_DENSITY = {"n": 4001, "seed": 22, "voxel_size": 1.0, "threshold_percentage": 0.5}
ADV_DIV = {"n": 2000, "seed": 23, "voxel_size": 0.1}


def adv_sor_table() -> np.ndarray:
    """georeferenced-style coordinates: 1e6 plus a 10-unit scene, in float64.  float32's grid there is 1/16 -- as coarse as the
    neighbour distances -- so a cast moves the mean distances and the mask"""
    rng = np.random.default_rng(ADV_SOR["seed"])
    n = ADV_SOR["n"]
    t = np.zeros(n, [("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("orig_index", "<i8")])
    xyz = 1e6 + rng.uniform(0.0, 10.0, (n, 3))
    t["x"], t["y"], t["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    t["orig_index"] = np.arange(n)
    return t


def adv_density_table() -> np.ndarray:
    """a 3 x 3 x 3-voxel block of float64 points plus five points at x = 3 - 1e-9: in voxel 2 (inside the block, kept) in float64,
    in voxel 3 (five points: not dense, dropped) once cast to float32, where 3 - 1e-9 rounds to 3"""
    rng = np.random.default_rng(ADV_DENSITY["seed"])
    n = ADV_DENSITY["n"]
    t = np.zeros(n, [("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("orig_index", "<i8")])
    xyz = rng.uniform(0.0, 3.0, (n, 3))
    xyz[:5, 0] = 3.0 - 1e-9
    t["x"], t["y"], t["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    t["orig_index"] = np.arange(n)
    return t


def adv_div_table() -> np.ndarray:
    """float64 coordinates that float32 holds exactly (a cast is exact) but whose float64 division by 0.1 lands in another voxel
    than the float32 division: the density filter cannot take float64 tables even when their values are float32's.  The
    values come from a scan over float32 multiples of the voxel size for the ones the two divisions disagree on."""
    rng = np.random.default_rng(ADV_DIV["seed"])
    v = ADV_DIV["voxel_size"]
    cand = (np.arange(1, 200001, dtype=np.float64) * v).astype(np.float32)
    cand = np.concatenate([cand, np.nextafter(cand, np.float32(np.inf)), np.nextafter(cand, np.float32(0))])
    k64 = np.floor(cand.astype(np.float64) / v)
    k32 = np.floor(cand / v)
    hard = cand[k64 != k32]
    n = ADV_DIV["n"]
    t = np.zeros(n, [("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("orig_index", "<i8")])
    xyz = rng.uniform(0.0, 2.0, (n, 3)).astype(np.float32).astype(np.float64)
    xyz[:min(len(hard), 16), 0] = hard[:16]
    t["x"], t["y"], t["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    t["orig_index"] = np.arange(n)
    return t


def cast_f32(t: np.ndarray) -> np.ndarray:
    """what a silent cast hands the device: x/y/z as float32"""
    return retype(t, {nm: "<f4" for nm in XYZ})
