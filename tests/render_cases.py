"""What tests/test_render_host.py and tests/test_render_gpu.py share, computed on the CPU: a camera whose view matrix is the
identity (a row's z is its depth, exactly), seeded scenes with the planted rows the issue lists, and the stacks of splats over
one tile that exercise the blend's batch loop."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transform_cases as tc  # noqa: E402

rd = importlib.import_module("3dgsconverter_amd.render")

F32 = np.float32
NEAR = 0.5
SIZES = ((1, 1), (16, 16), (17, 33), (37, 21), (48, 40))
STRIDES = (68, 71, 248, 251)
DEGREE_STRIDES = {0: 68, 1: 104, 2: 167, 3: 248}
GEOMETRY = ("x", "y", "z", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3", "opacity")
RGB_ONLY = np.dtype([(nm, "<f4") for nm in GEOMETRY] + [("red", "u1"), ("green", "u1"), ("blue", "u1")])
BACKGROUND = (0.2, 0.5, 1.0)


def focal(w: int, h: int) -> float:
    return 0.75 * max(w, h)


def axis_camera(w: int, h: int, near: float = NEAR):
    """the camera at the origin that looks along +z with x right and y down: V = (I | 0), so z_cam is the row's z bit for bit"""
    f = focal(w, h)
    return rd.Camera(w, h, np.eye(3, 4), (0.0, 0.0, 0.0), f, f, (w - 1) / 2.0, (h - 1) / 2.0, w / (2.0 * f), h / (2.0 * f), near)


def plan_for(table, w: int, h: int, **kw):
    return rd.plan_render(table.dtype, axis_camera(w, h), **dict({"background": BACKGROUND}, **kw))


def logit(alpha):
    return np.log(alpha / (1.0 - alpha))


def place(t, rows, w, h, px, py, z, sigma_px, alpha, quat=None):
    """rows of `t` at pixel (px, py) and depth z, with a footprint of about sigma_px pixels per axis and opacity alpha"""
    f, cx, cy = focal(w, h), (w - 1) / 2.0, (h - 1) / 2.0
    z = np.broadcast_to(np.asarray(z, np.float64), (len(rows),))
    t["x"][rows] = ((np.asarray(px) - cx) / f * z).astype(F32)
    t["y"][rows] = ((np.asarray(py) - cy) / f * z).astype(F32)
    t["z"][rows] = z.astype(F32)
    sig = np.broadcast_to(np.asarray(sigma_px, np.float64).reshape(len(rows) if np.ndim(sigma_px) else 1, -1), (len(rows), 3))
    for i in range(3):
        t["scale_%d" % i][rows] = np.log(sig[:, i] * z / f).astype(F32)
    t["opacity"][rows] = logit(np.broadcast_to(np.asarray(alpha, np.float64), (len(rows),))).astype(F32)
    if quat is not None:
        for i in range(4):
            t["rot_%d" % i][rows] = F32(quat[i])


def scene(dtype, n: int, w: int, h: int, seed: int = 0) -> np.ndarray:
    """n rows of `dtype` (at least 64) in front of axis_camera(w, h): random splats of 0.5 ... 4 pixels across the image and a
    little beyond its edges, random orientations, colours and opacities, runs of equal float32 depth, and in front the planted
    rows: 0 covers the whole image; 1 straddles the corner of the first four tiles; 2-5 lie off-screen on each side; 6 behind the
    camera; 7 at z_cam == near; 8-18 a non-finite value in each geometry field; 19 a zero quaternion; 20 an opacity deep in the
    0.99 clamp; 21 and 22 an alpha just above and just below 1/255 at their centre pixel."""
    assert n >= 64
    rng = np.random.default_rng(104729 * dtype.itemsize + 31 * n + 7 * w + h + seed)
    t = tc.random_rows(dtype, n, rng)
    rows = np.arange(n)
    z = rng.uniform(1.0, 6.0, n)
    z[40:52] = 2.5                                  # runs of equal float32 depth, their footprints overlapping
    z[52:60] = 3.25
    px, py = rng.uniform(-4.0, w + 3.0, n), rng.uniform(-4.0, h + 3.0, n)
    px[40:60], py[40:60] = rng.uniform(0, w, 20), rng.uniform(0, h, 20)
    place(t, rows, w, h, px, py, z, rng.uniform(0.5, 4.0, (n, 3)), rng.uniform(0.05, 0.9, n))
    place(t, [0], w, h, [w / 2.0], [h / 2.0], 3.0, 4.0 * max(w, h), 0.2, quat=(1, 0, 0, 0))
    place(t, [1], w, h, [15.5], [15.5], 2.0, 1.5, 0.6)
    far = 40.0 * max(w, h)
    place(t, [2, 3, 4, 5], w, h, [-far, w + far, w / 2.0, w / 2.0], [h / 2.0, h / 2.0, -far, h + far], 2.0, 1.0, 0.5)
    t["z"][6] = F32(-2.0)
    t["z"][7] = F32(NEAR)
    bad = np.array([np.nan, np.inf, -np.inf], F32)
    for k, nm in enumerate(GEOMETRY):
        t[nm][8 + k] = bad[k % 3]
    for i in range(4):
        t["rot_%d" % i][19] = F32(0.0)
    place(t, [20], w, h, [w / 3.0], [h / 3.0], 1.5, 1.0, 0.5)
    t["opacity"][20] = F32(20.0)
    place(t, [21, 22], w, h, [min(5, w - 1), min(9, w - 1)], [min(3, h - 1), min(3, h - 1)], 0.9, 2.0, 0.5, quat=(1, 0, 0, 0))
    t["opacity"][21], t["opacity"][22] = F32(-5.5), F32(-5.6)      # sigmoid: 0.00407 and 0.00368 around 1/255 = 0.00392
    return t


def stack(dtype, n: int, alpha: float, sigma_px: float, seed: int = 0) -> np.ndarray:
    """n splats over the one tile of a 16 x 16 image, all centred near its middle, depths ascending with the row in a shuffled
    order.  alpha 0.03 and sigma 3: the middle pixels finish after about 300 splats -- in the second LDS batch -- and the outer
    ones never do.  alpha 0.5 and sigma 40: every pixel finishes inside the first batch and the workgroup leaves the loop."""
    rng = np.random.default_rng(8191 * dtype.itemsize + n + seed)
    t = tc.random_rows(dtype, n, rng)
    z = 2.0 + 0.001 * rng.permutation(n)
    place(t, np.arange(n), 16, 16, 7.5 + rng.uniform(-0.5, 0.5, n), 7.5 + rng.uniform(-0.5, 0.5, n), z, sigma_px, alpha)
    return t


def distinct_depths(dtype, n: int, w: int, h: int) -> np.ndarray:
    """a scene without the planted rows whose float32 depths are all different"""
    rng = np.random.default_rng(n + w)
    t = tc.random_rows(dtype, n, rng)
    z = 1.0 + 0.004 * rng.permutation(n)
    place(t, np.arange(n), w, h, rng.uniform(0, w, n), rng.uniform(0, h, n), z, rng.uniform(0.5, 4.0, (n, 3)), rng.uniform(0.05, 0.9, n))
    assert len(np.unique(t["z"])) == n
    return t
