"""The definition of voxel decimation on a splat table, in numpy: what csrc/decimate.hip reproduces bit for bit.  Original to
this project (the reference has no counterpart); DESIGN.md 6r states it in words.

Every operation is float64, rounded once, in the order written here, except where float32 is stated.  The float32 exp and
log are csrc/np_exp.h and csrc/np_log.h through their host twins (_lib.np_exp_host, _lib.np_log_host), not the running
numpy's.  Clamps are two comparisons each (a NaN stays a NaN); no operation looks at the sign or the payload of a NaN.

  mergeable   x y z finite;  w = E((s0 + s1) + s2) * (1 / (1 + E(-opacity))) in float32 finite and > 0;
              qq = ((q0 q0 + q1 q1) + q2 q2) + q3 q3 in float64 finite and > 0.  Every other row is a group of its own.
  cell        per axis f = floorf(v / (float)H) in float32; f outside [-2^20, 2^20) on a mergeable row: ValueError.
  groups      the mergeable rows of one cell, members in row order, groups in the order of their first member's row.
              A group of one row is a bit copy.
  sums        members in row order in blocks of 256; a block sum runs from +0.0 member by member, the group sum from +0.0
              block by block.
  terms       c = (cell + 0.5) * H,  d = p - c,  n = sqrt(qq),  (a, b, cq, dq) = q / n,  R the standard matrix,
              v_i = e_i e_i with e_i = f64(E(scale_i)),  C_jk = ((R_j0 v_0) R_k0 + (R_j1 v_1) R_k1) + (R_j2 v_2) R_k2;
              W += w,  S1_j += w d_j,  S2_jk += w (C_jk + d_j d_k),  channel += w f64(value)
  moments     m = S1 / W,  mu = c + m,  Sigma_jk = S2_jk / W - m_j m_k
  eigen       6 cyclic Jacobi sweeps over (0,1), (0,2), (1,2) (jacobi3); eigenvalues unsorted, V from the identity
  outputs     lambda clamped to [2^-126, FLT_MAX];  scale_j = 0.5f * L(f32(lambda_j));  rot = Shepperd(V), normalised,
              rot_0 >= 0;  position f32(mu);  alpha' = W / sqrt((l0 l1) l2) clamped to [2^-24, 1 - 2^-10],
              opacity = L(f32(alpha' / (1 - alpha')));  f_dc_*, f_rest_*, nx ny nz = f32(S / W);
              red green blue (u1) = rint(S / W) clamped to 0 ... 255 (a NaN gives 0);  every other field the first member's
  zero_names  those fields are 0x00000000 in every output row
"""
import importlib

import numpy as np

lib = importlib.import_module("3dgsconverter_amd._lib")

F32, F64 = np.float32, np.float64
BLOCK = 256
CELL_LIMIT = 1 << 20
GEOMETRY = ("x", "y", "z", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3", "opacity")
RGB = ("red", "green", "blue")
S2_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
LAMBDA_MIN, LAMBDA_MAX = F64(2.0 ** -126), F64(np.finfo(np.float32).max)
ALPHA_MIN, ALPHA_MAX = F64(2.0 ** -24), F64(1.0 - 2.0 ** -10)


def mean_names(dtype):
    """the '<f4' fields that become the weighted mean of a group's members, in the dtype's field order"""
    import re
    return tuple(nm for nm in np.dtype(dtype).names
                 if re.fullmatch(r"f_dc_\d+|f_rest_\d+|nx|ny|nz", nm))


def u8_names(dtype):
    names = np.dtype(dtype).names
    return RGB if all(nm in names and np.dtype(dtype)[nm] == np.dtype("u1") for nm in RGB) else ()


def weight(table):
    """the visibility weight in float32: csrc/splat_metric.h's expression before the negation"""
    s0, s1, s2, o = (np.ascontiguousarray(table[nm], dtype=F32) for nm in ("scale_0", "scale_1", "scale_2", "opacity"))
    with np.errstate(all="ignore"):
        return lib.np_exp_host((s0 + s1) + s2) * (F32(1) / (F32(1) + lib.np_exp_host(-o)))


def quat_norm2(table):
    q = [table[f"rot_{i}"].astype(F64) for i in range(4)]
    with np.errstate(all="ignore"):
        return ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]


def mergeable(table):
    w = weight(table)
    qq = quat_norm2(table)
    ok = np.isfinite(table["x"]) & np.isfinite(table["y"]) & np.isfinite(table["z"])
    with np.errstate(all="ignore"):
        return ok & np.isfinite(w) & (w > 0) & np.isfinite(qq) & (qq > 0)


def cells_f32(table, H):
    """(n, 3) float32: floorf(v / (float)H), density.hip's voxel_key before the cast"""
    h = F32(H)
    with np.errstate(all="ignore"):
        return np.stack([np.floor(np.ascontiguousarray(table[nm], dtype=F32) / h) for nm in ("x", "y", "z")], axis=1)


def groups_of(table, H):
    """-> (list of int64 row arrays, one per group, in output order; the (n, 3) int64 cells, valid for mergeable rows).
    ValueError when a mergeable row's cell leaves [-2^20, 2^20)"""
    n = len(table)
    ok = mergeable(table)
    f = cells_f32(table, H)
    with np.errstate(all="ignore"):
        inside = np.all((f >= F32(-CELL_LIMIT)) & (f < F32(CELL_LIMIT)), axis=1)
    if np.any(ok & ~inside):
        raise ValueError("decimate: the voxel size %r is too small for the scene's coordinates (a cell index leaves +-2^20)" % (H,))
    cell = np.zeros((n, 3), np.int64)
    cell[ok] = f[ok].astype(np.int64)
    b = cell + CELL_LIMIT
    key = (b[:, 2].astype(np.uint64) << np.uint64(42)) | (b[:, 1].astype(np.uint64) << np.uint64(21)) | b[:, 0].astype(np.uint64)
    key[~ok] = (np.uint64(1) << np.uint64(63)) | np.arange(n, dtype=np.uint64)[~ok]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    heads = np.nonzero(np.concatenate(([True], ks[1:] != ks[:-1])))[0] if n else np.zeros(0, np.int64)
    ends = np.concatenate((heads[1:], [n])) if n else heads
    runs = [order[a:b_] for a, b_ in zip(heads, ends)]
    runs.sort(key=lambda r: int(r[0]))          # (a run's first entry is its lowest row: the order is stable)
    return runs, cell


def blocked_sum(terms):
    """terms (k, C) float64 in member order -> (C,): blocks of 256 summed member by member from +0.0, the block sums summed in
    block order from +0.0"""
    zero = np.zeros((1, terms.shape[1]), F64)
    with np.errstate(all="ignore"):
        blocks = [np.add.accumulate(np.concatenate((zero, terms[a:a + BLOCK])), axis=0)[-1] for a in range(0, len(terms), BLOCK)]
        return np.add.accumulate(np.concatenate((zero, np.array(blocks, F64).reshape(len(blocks), -1))), axis=0)[-1]


def rotation_matrix(q0, q1, q2, q3):
    """-> R[j][k] (arrays) of the quaternion normalised in float64"""
    qq = ((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3
    n = np.sqrt(qq)
    w, x, y, z = q0 / n, q1 / n, q2 / n, q3 / n
    xx, yy, zz = x * x, y * y, z * z
    xy, xz, yz = x * y, x * z, y * z
    wx, wy, wz = w * x, w * y, w * z
    return [[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
            [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
            [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]]


def member_terms(table, rows, cell, H, means, u8s):
    """the (k, 10 + len(means) + len(u8s)) float64 terms of the rows `rows`, all of cell `cell` (3 ints): W | S1 | S2 | channels"""
    t = table[rows]
    with np.errstate(all="ignore"):
        w = weight(t).astype(F64)
        c = [(F64(int(cell[a])) + 0.5) * F64(H) for a in range(3)]
        d = [t[nm].astype(F64) - c[a] for a, nm in enumerate(("x", "y", "z"))]
        R = rotation_matrix(*[t[f"rot_{i}"].astype(F64) for i in range(4)])
        e = [lib.np_exp_host(np.ascontiguousarray(t[f"scale_{i}"], dtype=F32)).astype(F64) for i in range(3)]
        v = [e[i] * e[i] for i in range(3)]
        cols = [w] + [w * d[a] for a in range(3)]
        for j, k in S2_PAIRS:
            C = ((R[j][0] * v[0]) * R[k][0] + (R[j][1] * v[1]) * R[k][1]) + (R[j][2] * v[2]) * R[k][2]
            cols.append(w * (C + d[j] * d[k]))
        cols += [w * t[nm].astype(F64) for nm in means]
        cols += [w * t[nm].astype(F64) for nm in u8s]
    return np.stack(cols, axis=1)


def moments(S, cell, H):
    """group sums S (10+,) -> (W, mu (3,), Sigma 3x3 nested list)"""
    with np.errstate(all="ignore"):
        W = S[0]
        m = [S[1 + a] / W for a in range(3)]
        mu = [(F64(int(cell[a])) + 0.5) * F64(H) + m[a] for a in range(3)]
        Sig = [[None] * 3 for _ in range(3)]
        for i, (j, k) in enumerate(S2_PAIRS):
            Sig[j][k] = Sig[k][j] = S[4 + i] / W - m[j] * m[k]
    return W, mu, Sig


def jacobi3(A):
    """A: symmetric 3x3 (nested lists of float64 scalars or arrays) -> (lambda [3], V[k][j]: column j the eigenvector of lambda_j).
    Exactly 6 sweeps over (0,1), (0,2), (1,2); a rotation whose off-diagonal is exactly 0 is skipped"""
    A = [[np.asarray(A[j][k], F64) for k in range(3)] for j in range(3)]
    one, zero = np.ones_like(A[0][0]), np.zeros_like(A[0][0])
    V = [[one if j == k else zero for k in range(3)] for j in range(3)]
    with np.errstate(all="ignore"):
        for _ in range(6):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                r = 3 - p - q
                apq = A[p][q]
                skip = apq == 0
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                sgn = np.where(theta >= 0, 1.0, -1.0)
                t = np.where(np.isinf(theta), 0.0, sgn / (np.abs(theta) + np.sqrt(theta * theta + 1.0)))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                app, aqq = A[p][p] - t * apq, A[q][q] + t * apq
                arp, arq = c * A[r][p] - s * A[r][q], s * A[r][p] + c * A[r][q]
                A[p][p], A[q][q] = np.where(skip, A[p][p], app), np.where(skip, A[q][q], aqq)
                A[p][q] = A[q][p] = np.where(skip, apq, 0.0)
                new_rp, new_rq = np.where(skip, A[r][p], arp), np.where(skip, A[r][q], arq)
                A[r][p] = A[p][r] = new_rp
                A[r][q] = A[q][r] = new_rq
                for k in range(3):
                    vkp, vkq = c * V[k][p] - s * V[k][q], s * V[k][p] + c * V[k][q]
                    V[k][p], V[k][q] = np.where(skip, V[k][p], vkp), np.where(skip, V[k][q], vkq)
    return [A[0][0], A[1][1], A[2][2]], V


def shepperd(V):
    """rotation matrix V[j][k] -> (w, x, y, z) normalised in float64, w >= 0: branch on the trace, then on the largest diagonal"""
    V = [[np.asarray(V[j][k], F64) for k in range(3)] for j in range(3)]
    with np.errstate(all="ignore"):
        tr = (V[0][0] + V[1][1]) + V[2][2]
        S0 = np.sqrt(tr + 1.0) * 2.0
        S1 = np.sqrt(((1.0 + V[0][0]) - V[1][1]) - V[2][2]) * 2.0
        S2 = np.sqrt(((1.0 + V[1][1]) - V[0][0]) - V[2][2]) * 2.0
        S3 = np.sqrt(((1.0 + V[2][2]) - V[0][0]) - V[1][1]) * 2.0
        b0 = tr > 0
        b1 = ~b0 & (V[0][0] > V[1][1]) & (V[0][0] > V[2][2])
        b2 = ~b0 & ~b1 & (V[1][1] > V[2][2])
        cand = [(0.25 * S0, (V[2][1] - V[1][2]) / S0, (V[0][2] - V[2][0]) / S0, (V[1][0] - V[0][1]) / S0),
                ((V[2][1] - V[1][2]) / S1, 0.25 * S1, (V[0][1] + V[1][0]) / S1, (V[0][2] + V[2][0]) / S1),
                ((V[0][2] - V[2][0]) / S2, (V[0][1] + V[1][0]) / S2, 0.25 * S2, (V[1][2] + V[2][1]) / S2),
                ((V[1][0] - V[0][1]) / S3, (V[0][2] + V[2][0]) / S3, (V[1][2] + V[2][1]) / S3, 0.25 * S3)]
        q = [np.where(b0, cand[0][i], np.where(b1, cand[1][i], np.where(b2, cand[2][i], cand[3][i]))) for i in range(4)]
        n = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
        q = [v / n for v in q]
        flip = q[0] < 0
        return [np.where(flip, -v, v) for v in q]


def clamp(v, lo, hi):
    v = np.asarray(v, F64)
    v = np.where(v < lo, lo, v)
    return np.where(v > hi, hi, v)


def merged_fields(S, cell, H, n_mean, n_u8):
    """group sums -> dict: position (3 f32), scale (3 f32), rot (4 f32), opacity (f32), mean (n_mean f32), u8 (n_u8 uint8),
    and the float64 intermediates W, mu, Sigma, lam (clamped), V, alpha (before the clamp), alpha_clamped"""
    W, mu, Sig = moments(S, cell, H)
    lam, V = jacobi3(Sig)
    with np.errstate(all="ignore"):
        lam = [clamp(v, LAMBDA_MIN, LAMBDA_MAX) for v in lam]
        scale = [F32(0.5) * lib.np_log_host(np.array([v], F64).astype(F32))[0] for v in lam]
        rot = [np.array(v, F64).astype(F32) for v in shepperd(V)]
        alpha = W / np.sqrt((lam[0] * lam[1]) * lam[2])
        ac = clamp(alpha, ALPHA_MIN, ALPHA_MAX)
        opacity = lib.np_log_host(np.array([ac / (1.0 - ac)], F64).astype(F32))[0]
        mean = (S[10:10 + n_mean] / W).astype(F32)
        c = np.rint(S[10 + n_mean:10 + n_mean + n_u8] / W)
        c = np.where(c < 0, 0.0, c)
        c = np.where(c > 255, 255.0, c)
        u8 = np.where(np.isnan(c), 0.0, c).astype(np.uint8)
    return {"position": [np.array(v, F64).astype(F32) for v in mu], "scale": scale, "rot": rot, "opacity": opacity, "mean": mean, "u8": u8,
            "W": W, "mu": mu, "Sigma": Sig, "lam": lam, "V": V, "alpha": alpha, "alpha_clamped": ac}


def decimate_table(table, H, zero_names=(), want_details=False):
    """-> (the decimated table, {"groups", "merged_groups", "passed_through"}) [, details: one merged_fields dict per merged
    group with its member rows under "rows"]"""
    H = float(H)
    if not np.isfinite(H) or H <= 0:
        raise ValueError("decimate: the voxel size must be a finite number greater than 0, got %r" % (H,))
    means, u8s = mean_names(table.dtype), u8_names(table.dtype)
    runs, cell = groups_of(table, H)
    out = np.empty(len(runs), table.dtype)
    merged = 0
    details = []
    for g, rows in enumerate(runs):
        out[g] = table[rows[0]]
        if len(rows) < 2:
            continue
        merged += 1
        cg = cell[rows[0]]
        S = blocked_sum(member_terms(table, rows, cg, H, means, u8s))
        f = merged_fields(S, cg, H, len(means), len(u8s))
        for a, nm in enumerate(("x", "y", "z")):
            out[nm][g] = f["position"][a]
        for i in range(3):
            out[f"scale_{i}"][g] = f["scale"][i]
        for i in range(4):
            out[f"rot_{i}"][g] = f["rot"][i]
        out["opacity"][g] = f["opacity"]
        for i, nm in enumerate(means):
            out[nm][g] = f["mean"][i]
        for i, nm in enumerate(u8s):
            out[nm][g] = f["u8"][i]
        if want_details:
            f["rows"] = rows
            details.append(f)
    for nm in zero_names:
        if nm in (table.dtype.names or ()):
            out[nm] = 0
    info = {"groups": len(runs), "merged_groups": merged, "passed_through": len(runs) - merged}
    return (out, info, details) if want_details else (out, info)


def float_names(dtype):
    """the float32 fields of a table: same_by_class's NaN rule applies to them"""
    dtype = np.dtype(dtype)
    return tuple(nm for nm in dtype.names if dtype[nm] == np.dtype("<f4"))
