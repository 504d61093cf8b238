"""Shared inputs of the fidelity tests: the image sizes and pairs at which the compare kernel can go wrong.

T is the kernel's tile edge (GSX_FIDELITY_TILE, mirrored by fidelity.TILE): a workgroup owns T x T pixels and window origins and
stages T + 7 pixels per side, so T + 6, T + 7 and T + 8 per side are the last size with one tile of windows, the size whose
windows exactly fill one tile's staging, and the first whose windows need a second tile.
"""
import importlib

import numpy as np

T = importlib.import_module("3dgsconverter_amd.fidelity").TILE

# (height, width)
SIZES = [(7, 7), (5, 40), (8, 8), (8, 9), (9, 8), (T + 6, T + 6), (T + 7, T + 7), (T + 8, T + 8), (T + 6, T + 8), (71, 40)]

PAIRS = ["random", "identical", "black_white", "complement", "one_pixel_corner", "one_pixel_seam", "ramp_shift"]


def pair(kind: str, h: int, w: int):
    """-> (A, B), two (h, w, 3) uint8 images"""
    rng = np.random.default_rng(1000 * h + w)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "random":
        return a, rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "identical":
        return a, a.copy()
    if kind == "black_white":
        return np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)
    if kind == "complement":
        return a, (255 - a).astype(np.uint8)
    if kind == "one_pixel_corner":
        b = a.copy()
        b[h - 1, w - 1, 1] ^= 0x80
        return a, b
    if kind == "one_pixel_seam":        # the first pixel of the second tile (the last pixel of a smaller image)
        b = a.copy()
        b[min(T, h - 1), min(T, w - 1), 2] ^= 0x41
        return a, b
    if kind == "ramp_shift":
        ramp = (np.arange(w + 1) * 255 // max(w, 1)).astype(np.uint8)
        a = np.broadcast_to(ramp[:w, None], (h, w, 3)).copy()
        b = np.broadcast_to(ramp[1:, None], (h, w, 3)).copy()
        return a, b
    raise KeyError(kind)


CASES = [(kind, h, w) for (h, w) in SIZES for kind in PAIRS]
IDS = ["%s-%dx%d" % c for c in CASES]
