"""The definition of the preview image of a splat table, in numpy: what csrc/render.hip reproduces bit for bit.  Original to
this project (the reference renders nothing); DESIGN.md 6s states it in words.  Two stages: ``records`` (one per splat) and
``image`` (the blend of the records).

records -- every operation float64 on the float32 fields, rounded once, in the order written here; the stored values are
rounded to float32.  E is the float32 exp of csrc/np_exp.h through its host twin (_lib.np_exp_host), never the running numpy's.

  camera      p_cam_r = ((V_r0 x + V_r1 y) + V_r2 z) + V_r3;  depth = f32(p_cam_z)
  invisible   a non-finite geometry field (x y z, scale_0..2, rot_0..3, opacity);  qq = ((q0 q0 + q1 q1) + q2 q2) + q3 q3 not > 0;
              p_cam_z <= near;  det not in (0, inf);  the clipped rectangle empty.  An invisible row's record is all zero bits.
  covariance  e_i = f64(E(scale_i)), v_i = e_i e_i, R the matrix of q / sqrt(qq),
              S_jk = ((R_j0 v_0) R_k0 + (R_j1 v_1) R_k1) + (R_j2 v_2) R_k2
  jacobian    t_x = clamp(x_cam / z_cam, +-1.3 tan_fovx) z_cam (t_y alike);  J = [[fx / z, 0, -(fx t_x) / (z z)], [0, fy / z, -(fy t_y) / (z z)]]
              T = J W (W = V's 3x3, each entry one product pair and one sum),  M = T S,  S' = M T^t + 0.3 I
  conic       det = sxx syy - sxy sxy;  a = syy / det, b = -sxy / det, c = sxx / det
  radius      mid = 0.5 (sxx + syy);  r = ceil(3 sqrt(mid + sqrt(max(0.1, mid mid - det))))
  centre      u = fx (x_cam / z_cam) + cx,  v = fy (y_cam / z_cam) + cy
  rectangle   x0 = max(ceil(u - r), 0), x1 = min(floor(u + r), width - 1), y alike, from the float64 u, v
  opacity     1 / (1 + E(-opacity)) in float32 (csrc/splat_metric.h's expression)
  colour      d = (p - eye) / |p - eye|;  per channel sum_k Y_k(d) sh_k from k = 0 upward, + 0.5, values not > 0 become 0;
              or, for a table without f_dc, byte / 255

image -- per pixel (px, py), float32, one operation at a time, over the visible records whose rectangle holds the pixel in
ascending (depth, row):  dx = u - px, dy = v - py;  power = -0.5 (a dx dx + c dy dy) - (b dx) dy;  skipped unless power <= 0;
alpha = min(0.99, opac E(power));  skipped if alpha < 1/255;  T' = T (1 - alpha);  T' < 1e-4 finishes the pixel with nothing
added;  else C += col (alpha T), T = T'.  The pixel is C + T background, and its byte floor(clip(., 0, 1) 255 + 0.5).
"""
import importlib

import numpy as np

lib = importlib.import_module("3dgsconverter_amd._lib")

F32, F64 = np.float32, np.float64
GEOMETRY = ("x", "y", "z", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3", "opacity")
C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)
RECORD = np.dtype([("u", "<f4"), ("v", "<f4"), ("a", "<f4"), ("b", "<f4"), ("c", "<f4"), ("opac", "<f4"), ("r", "<f4"), ("g", "<f4"),
                   ("bl", "<f4"), ("depth", "<f4"), ("x0", "<i4"), ("x1", "<i4"), ("y0", "<i4"), ("y1", "<i4"), ("visible", "<u4"),
                   ("pad", "<u4")])
ALPHA_MAX, ALPHA_MIN, T_MIN = F32(0.99), F32(1.0) / F32(255.0), F32(1e-4)


def rotation_matrix(q0, q1, q2, q3):
    """-> R[j][k] (arrays) of the quaternion (w, x, y, z) normalised in float64"""
    qq = ((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3
    n = np.sqrt(qq)
    w, x, y, z = q0 / n, q1 / n, q2 / n, q3 / n
    xx, yy, zz = x * x, y * y, z * z
    xy, xz, yz = x * y, x * z, y * z
    wx, wy, wz = w * x, w * y, w * z
    return [[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
            [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
            [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]], qq


def sh_basis(x, y, z, degree):
    """Y_0 ... Y_((degree + 1)^2 - 1) of the 3DGS rasteriser's real basis on unit directions, each in the written order"""
    b = [C0]
    if degree >= 1:
        b += [(-C1) * y, C1 * z, (-C1) * x]
    if degree >= 2:
        xx, yy, zz = x * x, y * y, z * z
        b += [(C2[0] * x) * y, (C2[1] * y) * z, C2[2] * ((2.0 * zz - xx) - yy), (C2[3] * x) * z, C2[4] * (xx - yy)]
    if degree >= 3:
        b += [(C3[0] * y) * (3.0 * xx - yy), ((C3[1] * x) * y) * z, (C3[2] * y) * ((4.0 * zz - xx) - yy),
              (C3[3] * z) * ((2.0 * zz - 3.0 * xx) - 3.0 * yy), (C3[4] * x) * ((4.0 * zz - xx) - yy), (C3[5] * z) * (xx - yy),
              (C3[6] * x) * (xx - 3.0 * yy)]
    return b


def colours(table, plan):
    """-> three float64 arrays: the colour of every row before its rounding to float32"""
    if plan.dc[0] < 0:
        return [table[nm].astype(F64) / 255.0 for nm in ("red", "green", "blue")]
    eye = plan.camera.eye
    dx, dy, dz = (table[nm].astype(F64) - F64(eye[k]) for k, nm in enumerate("xyz"))
    n = np.sqrt((dx * dx + dy * dy) + dz * dz)
    basis = sh_basis(dx / n, dy / n, dz / n, plan.degree)
    out = []
    for ch in range(3):
        res = C0 * table["f_dc_%d" % ch].astype(F64)
        for k in range(1, len(basis)):
            res = res + basis[k] * table["f_rest_%d" % (ch * plan.m + k - 1)].astype(F64)
        res = res + 0.5
        out.append(np.where(res > 0, res, 0.0))
    return out


def records(table, plan) -> np.ndarray:
    """stage one: the RECORD of every row of `table` (a structured table of plan.dtype) under plan.camera"""
    cam = plan.camera
    V = cam.view
    n = len(table)
    rec = np.zeros(n, RECORD)
    if n == 0:
        return rec
    with np.errstate(all="ignore"):
        g = {nm: table[nm].astype(F64) for nm in GEOMETRY}
        finite = np.ones(n, bool)
        for nm in GEOMETRY:
            finite &= np.isfinite(g[nm])
        x, y, z = g["x"], g["y"], g["z"]
        pc = [((V[r, 0] * x + V[r, 1] * y) + V[r, 2] * z) + V[r, 3] for r in range(3)]
        zc = pc[2]
        R, qq = rotation_matrix(g["rot_0"], g["rot_1"], g["rot_2"], g["rot_3"])
        e = [lib.np_exp_host(np.ascontiguousarray(table["scale_%d" % i], dtype=F32)).astype(F64) for i in range(3)]
        v = [e[i] * e[i] for i in range(3)]
        S = [[((R[j][0] * v[0]) * R[k][0] + (R[j][1] * v[1]) * R[k][1]) + (R[j][2] * v[2]) * R[k][2] for k in range(3)] for j in range(3)]
        limx, limy = 1.3 * cam.tan_fovx, 1.3 * cam.tan_fovy
        xz, yz = pc[0] / zc, pc[1] / zc
        tx = np.minimum(limx, np.maximum(-limx, xz)) * zc
        ty = np.minimum(limy, np.maximum(-limy, yz)) * zc
        zz = zc * zc
        j00, j02 = cam.fx / zc, -(cam.fx * tx) / zz
        j11, j12 = cam.fy / zc, -(cam.fy * ty) / zz
        T = [[j00 * V[0, k] + j02 * V[2, k] for k in range(3)], [j11 * V[1, k] + j12 * V[2, k] for k in range(3)]]
        M = [[(T[r][0] * S[0][k] + T[r][1] * S[1][k]) + T[r][2] * S[2][k] for k in range(3)] for r in range(2)]
        sxx = ((M[0][0] * T[0][0] + M[0][1] * T[0][1]) + M[0][2] * T[0][2]) + 0.3
        sxy = (M[0][0] * T[1][0] + M[0][1] * T[1][1]) + M[0][2] * T[1][2]
        syy = ((M[1][0] * T[1][0] + M[1][1] * T[1][1]) + M[1][2] * T[1][2]) + 0.3
        det = sxx * syy - sxy * sxy
        a, b, c = syy / det, -sxy / det, sxx / det
        mid = 0.5 * (sxx + syy)
        disc = mid * mid - det
        r = np.ceil(3.0 * np.sqrt(mid + np.sqrt(np.where(disc > 0.1, disc, 0.1))))
        u, vv = cam.fx * xz + cam.cx, cam.fy * yz + cam.cy
        x0, x1 = np.maximum(np.ceil(u - r), 0.0), np.minimum(np.floor(u + r), cam.width - 1.0)
        y0, y1 = np.maximum(np.ceil(vv - r), 0.0), np.minimum(np.floor(vv + r), cam.height - 1.0)
        vis = finite & (qq > 0) & (zc > cam.near) & (det > 0) & (det < np.inf) & (x0 <= x1) & (y0 <= y1)
        o = np.ascontiguousarray(table["opacity"], dtype=F32)
        opac = F32(1) / (F32(1) + lib.np_exp_host(-o))
        col = colours(table, plan)
        for nm, val in (("u", u), ("v", vv), ("a", a), ("b", b), ("c", c), ("opac", opac), ("r", col[0]), ("g", col[1]), ("bl", col[2]),
                        ("depth", zc)):
            rec[nm][vis] = val[vis].astype(F32)
        for nm, val in (("x0", x0), ("x1", x1), ("y0", y0), ("y1", y1)):
            rec[nm][vis] = val[vis].astype(np.int32)
    rec["visible"] = vis
    return rec


def draw_order(rec) -> np.ndarray:
    """the visible rows in ascending (float32 depth, row)"""
    rows = np.nonzero(rec["visible"])[0]
    return rows[np.argsort(rec["depth"][rows], kind="stable")]


def image(rec, plan, details=None) -> np.ndarray:
    """stage two: the (height, width, 3) uint8 image of the records.  details (a dict): receives ``stop_rank``, per pixel the
    place in the draw order of the splat that finished it, or -1"""
    w, h = plan.camera.width, plan.camera.height
    PX, PY = np.meshgrid(np.arange(w, dtype=F32), np.arange(h, dtype=F32))
    T = np.ones((h, w), F32)
    C = np.zeros((h, w, 3), F32)
    done = np.zeros((h, w), bool)
    stop_rank = np.full((h, w), -1, np.int64)
    if details is not None:
        details["stop_rank"] = stop_rank
    with np.errstate(all="ignore"):
        for rank, i in enumerate(draw_order(rec)):
            s = rec[i]
            sl = (slice(int(s["y0"]), int(s["y1"]) + 1), slice(int(s["x0"]), int(s["x1"]) + 1))
            dx, dy = s["u"] - PX[sl], s["v"] - PY[sl]
            power = F32(-0.5) * (s["a"] * (dx * dx) + s["c"] * (dy * dy)) - (s["b"] * dx) * dy
            act = ~done[sl] & (power <= 0)
            alpha = np.minimum(ALPHA_MAX, s["opac"] * lib.np_exp_host(power))
            act &= ~(alpha < ALPHA_MIN)
            Tn = T[sl] * (F32(1) - alpha)
            stop = act & (Tn < T_MIN)
            add = act & ~stop
            done[sl] |= stop
            stop_rank[sl] = np.where(stop, rank, stop_rank[sl])
            wgt = alpha * T[sl]
            for ch, nm in enumerate(("r", "g", "bl")):
                C[sl + (ch,)] = np.where(add, C[sl + (ch,)] + s[nm] * wgt, C[sl + (ch,)])
            T[sl] = np.where(add, Tn, T[sl])
        out = C + T[:, :, None] * np.array(plan.background, F32)
        out = np.where(out < 0, F32(0), np.where(out > 1, F32(1), out))
        return np.floor(out * F32(255) + F32(0.5)).astype(np.uint8)


def render(table, plan) -> np.ndarray:
    return image(records(table, plan), plan)
