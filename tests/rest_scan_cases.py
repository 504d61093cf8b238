"""The f_rest scan's edge values, shared by test_spz_gpu.py (gsx_spz_rest_nonzero_dev) and test_ply_write_gpu.py
(gsx_ply_rest_nonzero_dev): both entry points answer `np.any(table[f] != 0)` per asked field -- NaN and denormals count, -0.0
does not.  A table's f_rest columns hold 0.0 where they are asked for and 1.0 where they are not; one value is planted in the
last row of one asked column."""
import numpy as np

BASE = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
REST = ["f_rest_%d" % i for i in range(45)]
TAIL = ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
SHAPES = {   # row bytes -> (dtype, rows per tile, the n around one tile)
    248: (np.dtype([(nm, "<f4") for nm in BASE + REST + TAIL]), 128, (1, 128, 129)),
    261: (np.dtype([("tag", "u1")] + [(nm, "<f4") for nm in BASE + REST + TAIL + ["e0", "e1", "e2"]]), 64, (1, 64, 65)),   # odd offsets
}
CASES = [(rb, n) for rb, (_, _, ns) in SHAPES.items() for n in ns]
ASKED = [i for i in range(45) if i % 3 != 1]                    # the others hold 1.0 and must not show
PLANTED = [(0x80000000, False), (0x00000001, True), (0x80000001, True), (0x7FC00001, True), (0x3F800000, True)]   # bits -> counts?
FIELDS = (0, 23, 44)                                            # where the value is planted: both ends and the middle of ASKED


def table(row_bytes, n):
    dt = SHAPES[row_bytes][0]
    assert dt.itemsize == row_bytes and all(i in ASKED for i in FIELDS)
    t = np.zeros(n, dt)
    for nm in dt.names:
        if nm not in REST or REST.index(nm) not in ASKED:
            t[nm] = 1
    return t


def plantings(t):
    """yields (field index, the asked mask, numpy's word) with one value planted in `t` itself; `t` is restored between two"""
    want = sum(1 << i for i in ASKED)
    for bits, counts in PLANTED:
        for i in FIELDS:
            col = t[REST[i]].view(np.uint32)
            col[-1] = bits
            with np.errstate(invalid="ignore"):
                word = sum(1 << k for k in ASKED if np.any(t[REST[k]] != 0))
            assert word == ((1 << i) if counts else 0)        # numpy's own answer: no bit for -0.0, exactly the field's bit otherwise
            yield i, want, word
            col[-1] = 0
