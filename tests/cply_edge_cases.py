"""Shared by tests/test_cply_edges_host.py and tests/test_cply_edges_gpu.py: the edge fixture of the compressed-PLY writer
(tests/golden/cply_edges_ref.npz, oracle/make_golden_cply_edges.py) and numpy restatements of what the device decides about
the alpha byte (csrc/cply.hip: cply_alpha_code)."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(__file__), "golden", "cply_edges_ref.npz")
SOG_ULPS_EXP = 4          # csrc/sog_math.h
F = np.float32

_gold = None


def gold():
    """the fixture, loaded once and left unchanged (arrays of an NpzFile are fresh copies on every access)"""
    global _gold
    if _gold is None:
        _gold = np.load(GOLD)
    return _gold


def ulp_step(a, steps):
    """csrc/sog_math.h ulp_step: the float32 `steps` ulps above / below, crossing zero correctly"""
    b = np.ascontiguousarray(a, dtype=F).view(np.int32).astype(np.int64)
    b = np.where(b < 0, -(2 ** 31) - b, b) + steps
    b = np.where(b < 0, -(2 ** 31) - b, b)
    return b.astype(np.int32).view(F)


def numpy_alpha_byte(x):
    """the reference's own expression (compressed_ply.py:200-203 and :312) on a float32 column"""
    x = np.ascontiguousarray(x, dtype=F)
    with np.errstate(over="ignore"):
        a = 1.0 / (1.0 + np.exp(-x))
        return np.clip(np.floor(a * 255 + 0.5), 0, 255).astype(np.uint32)


def alpha_code(x):
    """cply_alpha_code in numpy -> (byte, certain): exp in float64, the bracket of +-SOG_ULPS_EXP float32 ulps around it, both ends
    through numpy's float32 sequence; certain where both ends give the same byte and |x| < 80"""
    x = np.ascontiguousarray(x, dtype=F)
    ok = (x == x) & (np.abs(x) < F(80))
    with np.errstate(over="ignore"):
        et = np.exp(-x.astype(np.float64))
    a = np.where(ok, et, 1.0).astype(F)
    q = []
    for s in (-SOG_ULPS_EXP, SOG_ULPS_EXP):
        r = F(1) / (F(1) + ulp_step(a, s))
        q.append(np.clip(np.floor(r * F(255) + F(0.5)), 0, 255).astype(np.uint32))
    return q[0], ok & (q[0] == q[1])


def random_opacities(n=100_000, seed=21):
    return (np.random.default_rng(seed).standard_normal(n) * 4.0).astype(F)


def numpy_sh_bytes(v):
    """compressed_ply.py:245-246"""
    with np.errstate(over="ignore"):
        return np.clip((np.asarray(v, dtype=F) / 8.0 + 0.5) * 256, 0, 255).astype(np.uint8)
