"""The definition of the fidelity sums: what gsx_image_compare_dev and gsx_image_compare_host must return, word
for word, for two (h, w, 3) uint8 images A and B.

  sse[c]   the sum over all pixels of (A - B)^2 in channel c
  windows  (h - 7) (w - 7) when both sides are at least 8, else 0: every 8 x 8 box at stride 1
  ssim[c]  the sum over the windows of q = floor(r1 r2 2^32), with the window's integer sums Sa Sb Saa Sbb Sab over N = 64 pixels:
           r1 = f64(2 Sa Sb + c1) / f64(Sa^2 + Sb^2 + c1)
           r2 = f64(2 (N Sab - Sa Sb) + c2) / f64((N Saa - Sa^2) + (N Sbb - Sb^2) + c2)

All four operands are integers below 2^31 (the largest is 532 711 434), so their float64 values are exact; the two divisions and
the product are numpy's correctly rounded float64 operations on arrays (no fused multiply-add exists in them); the scaling by
2^32 is exact.  Everything else is Python-int or int64 arithmetic.
"""
import math
from fractions import Fraction

import numpy as np

WIN = 8
N = WIN * WIN
C1 = 26634        # round(N^2 (0.01 * 255)^2)
C2 = 239708       # round(N^2 (0.03 * 255)^2)
ONE = 1 << 32

assert C1 == round(N * N * (0.01 * 255) ** 2) and C2 == round(N * N * (0.03 * 255) ** 2)


def window_sums(img_or_product: np.ndarray) -> np.ndarray:
    """(h, w, 3) int64 -> (h - 7, w - 7, 3) int64: the sum over every 8 x 8 box"""
    v = np.lib.stride_tricks.sliding_window_view(img_or_product, (WIN, WIN), axis=(0, 1))
    return v.sum(axis=(-1, -2), dtype=np.int64)


def operands(a: np.ndarray, b: np.ndarray):
    """-> the four integer arrays (n1, d1, n2, d2), each (h - 7, w - 7, 3) int64"""
    a, b = a.astype(np.int64), b.astype(np.int64)
    sa, sb, saa, sbb, sab = (window_sums(v) for v in (a, b, a * a, b * b, a * b))
    n1 = 2 * sa * sb + C1
    d1 = sa * sa + sb * sb + C1
    n2 = 2 * (N * sab - sa * sb) + C2
    d2 = (N * saa - sa * sa) + (N * sbb - sb * sb) + C2
    return n1, d1, n2, d2


def window_q(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """-> q of every window and channel, (h - 7, w - 7, 3) int64"""
    n1, d1, n2, d2 = operands(a, b)
    assert max(int(np.abs(v).max()) for v in (n1, d1, n2, d2)) < 1 << 31
    r1 = n1.astype(np.float64) / d1.astype(np.float64)
    r2 = n2.astype(np.float64) / d2.astype(np.float64)
    return np.floor((r1 * r2) * float(ONE)).astype(np.int64)


def window_q_exact(a: np.ndarray, b: np.ndarray) -> list:
    """floor(exact * 2^32) of every window and channel in rational arithmetic, as a flat list of Python ints (window_q's order)"""
    n1, d1, n2, d2 = (v.ravel().tolist() for v in operands(a, b))
    return [math.floor(Fraction(p * r * ONE, q * s)) for p, q, r, s in zip(n1, d1, n2, d2)]


def compare(a: np.ndarray, b: np.ndarray) -> dict:
    """-> dict(sse: three ints, windows: int, ssim: three ints)"""
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape and a.ndim == 3 and a.shape[2] == 3
    h, w = a.shape[:2]
    d = a.astype(np.int64) - b.astype(np.int64)
    sse = tuple(int(v) for v in (d * d).sum(axis=(0, 1)))
    if h < WIN or w < WIN:
        return {"sse": sse, "windows": 0, "ssim": (0, 0, 0)}
    q = window_q(a, b)
    return {"sse": sse, "windows": (h - 7) * (w - 7), "ssim": tuple(int(v) for v in q.sum(axis=(0, 1), dtype=np.int64))}


def psnr(sse_total: int, h: int, w: int) -> float:
    """10 log10(255^2 * 3 h w / sse) over the three channels; inf for identical images"""
    return math.inf if sse_total == 0 else 10.0 * math.log10(255.0 ** 2 * (3 * h * w) / sse_total)


def ssim(ssim_total: int, windows: int):
    """the mean over windows and channels as a float; None without windows"""
    return None if windows == 0 else ssim_total / (3 * windows * ONE)
