"""The definition of a scene transform p' = s R p + t on a splat table, in numpy: what csrc/transform.hip (kernel and host twin)
reproduce bit for bit.  Original to this project.

Every product and sum is float64, rounded once per operation, sums left to right; the result is cast to float32 (round to
nearest even).  The log-scales take one float32 add.  The fields come from the dtype alone, independently of
transform.plan_transform; the numbers R -> q_R, D1..D3 are transform.py's (held to their identities in float64 by
test_transform_host.py).

  position   M = s R (nine float64 products);  x' = f32(((M00 X + M01 Y) + M02 Z) + t0), t is always added
  normals    the same with R, no translation             (only under a rotation, when nx ny nz are all there)
  log-scales scale_i' = scale_i + f32(log(f64(s)))       (only when s != 1)
  quaternion rot' = q_R (x) rot, Hamilton product, the norm kept       (only under a rotation)
  SH         per complete band l and channel c: out_j = f32((...((D[j,0] v_0 + D[j,1] v_1) + D[j,2] v_2) + ...))
  capped     the columns of `zero_names` are 0x00000000 in the result: the fill is applied after the transform
Everything else is a bit copy.
"""
import importlib

import numpy as np

tf = importlib.import_module("3dgsconverter_amd.transform")


def f64(col):
    return np.asarray(col).astype(np.float64)


def transform_table(table: np.ndarray, R=None, s=None, t=None, zero_names=()) -> np.ndarray:
    out = table.copy()
    names = table.dtype.names
    R = np.eye(3) if R is None else np.array(R, dtype=np.float64)
    s = 1.0 if s is None else float(s)
    t = np.zeros(3) if t is None else np.array(t, dtype=np.float64)
    rotates = not np.array_equal(R, np.eye(3))
    with np.errstate(all="ignore"):
        M = np.float64(s) * R
        X, Y, Z = f64(table["x"]), f64(table["y"]), f64(table["z"])
        for i, nm in enumerate("xyz"):
            out[nm] = ((((M[i, 0] * X + M[i, 1] * Y) + M[i, 2] * Z) + t[i])).astype(np.float32)
        if s != 1.0 and all(f"scale_{i}" in names for i in range(3)):
            ls = np.float32(np.log(np.float64(s)))
            for i in range(3):
                out[f"scale_{i}"] = table[f"scale_{i}"] + ls
        if rotates:
            if all(nm in names for nm in ("nx", "ny", "nz")):
                X, Y, Z = f64(table["nx"]), f64(table["ny"]), f64(table["nz"])
                for i, nm in enumerate(("nx", "ny", "nz")):
                    out[nm] = ((R[i, 0] * X + R[i, 1] * Y) + R[i, 2] * Z).astype(np.float32)
            if all(f"rot_{i}" in names for i in range(4)):
                w, x, y, z = (np.float64(v) for v in tf.quat_from_rotation(R))
                a, b, c, d = (f64(table[f"rot_{i}"]) for i in range(4))
                out["rot_0"] = (((w * a - x * b) - y * c) - z * d).astype(np.float32)
                out["rot_1"] = (((w * b + x * a) + y * d) - z * c).astype(np.float32)
                out["rot_2"] = (((w * c - x * d) + y * a) + z * b).astype(np.float32)
                out["rot_3"] = (((w * d + x * c) - y * b) + z * a).astype(np.float32)
            n_rest = sum(1 for nm in names if nm.startswith("f_rest_"))
            m = n_rest // 3
            D = tf.sh_rotation(R)
            for band in (1, 2, 3):
                if m < band * band + 2 * band:
                    continue
                Db, nb, k0 = D[band - 1], 2 * band + 1, band * band - 1
                for c in range(3):
                    v = [f64(table[f"f_rest_{c * m + k0 + k}"]) for k in range(nb)]
                    for j in range(nb):
                        acc = Db[j, 0] * v[0]
                        for k in range(1, nb):
                            acc = acc + Db[j, k] * v[k]
                        out[f"f_rest_{c * m + k0 + j}"] = acc.astype(np.float32)
    for nm in zero_names:
        if nm in names:
            out[nm] = 0
    return out


def same_by_class(got: np.ndarray, want: np.ndarray, float_names) -> "str | None":
    """The comparison rule: the tables' bytes are equal, except that where the definition has a NaN in a float32 field the other
    table may hold a NaN of any payload.  -> None, or a description of the first difference"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return "dtype or shape differ: %s %s / %s %s" % (got.dtype, got.shape, want.dtype, want.shape)
    g = got.copy()
    for nm in float_names:
        wn = np.isnan(want[nm])
        gn = np.isnan(got[nm])
        if not np.array_equal(wn, gn):
            i = int(np.nonzero(wn != gn)[0][0])
            return "field %s row %d: NaN in one table only (%r / %r)" % (nm, i, got[nm][i], want[nm][i])
        col = g[nm]
        col[wn] = want[nm][wn]
        g[nm] = col
    gb = g.view(np.uint8).reshape(len(g), -1) if len(g) else np.zeros((0, 1), np.uint8)
    wb = want.view(np.uint8).reshape(len(want), -1) if len(want) else np.zeros((0, 1), np.uint8)
    if np.array_equal(gb, wb):
        return None
    r, b = (int(v[0]) for v in np.nonzero(gb != wb))
    nm = next((n for n in want.dtype.names if want.dtype.fields[n][1] <= b < want.dtype.fields[n][1] + want.dtype[n].itemsize), "?")
    return "row %d byte %d (field %s): %r / %r" % (r, b, nm, got[nm][r] if nm != "?" else None, want[nm][r] if nm != "?" else None)
