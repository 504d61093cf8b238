"""What tests/test_merge_host.py and tests/test_merge_gpu.py share, computed on the CPU: the source layouts of the issue, tables
of random bit patterns for them (NaN payloads, -0.0 and denormals in every float field), aligned guard buffers and the remap
refusals."""
import numpy as np

import merge_numpy as mn

GUARD = 0xA5
SPZ_STRIDES = {0: 71, 1: 107, 2: 167, 3: 251}


def spz_dtype(degree: int) -> np.dtype:
    """the .spz and .splat readers' rows: the standard order at the file's degree, then red green blue"""
    rest = ["f_rest_%d" % i for i in range(3 * ((degree + 1) ** 2 - 1))]
    dt = np.dtype([(nm, "<f4") for nm in mn.BEFORE + rest + mn.AFTER] + [(nm, "u1") for nm in mn.COLOURS])
    assert dt.itemsize == SPZ_STRIDES[degree]
    return dt


def standard_dtype() -> np.dtype:
    """the 248-byte 3DGS row"""
    return np.dtype([(nm, "<f4") for nm in mn.BEFORE + ["f_rest_%d" % i for i in range(45)] + mn.AFTER])


def cc_dtype() -> np.dtype:
    """a 300-byte CloudCompare-style row: the colours as bytes in the MIDDLE (every later float field at an odd byte), extras of
    other types at both ends"""
    fields = [("scalar_label", "<i8")] + [(nm, "<f4") for nm in mn.BEFORE] + [(nm, "u1") for nm in mn.COLOURS]
    fields += [("f_rest_%d" % i, "<f4") for i in range(45)] + [(nm, "<f4") for nm in mn.AFTER]
    fields += [("scalar_extra_%d" % i, "<f4") for i in range(9)] + [("flag_%d" % i, "u1") for i in range(5)]
    dt = np.dtype(fields)
    assert dt.itemsize == 300
    return dt


def no_normals_dtype() -> np.dtype:
    """degree 2 without normals and without colours: 56 + 96 bytes"""
    names = [nm for nm in mn.BEFORE if not nm.startswith("n")] + ["f_rest_%d" % i for i in range(24)] + mn.AFTER
    return np.dtype([(nm, "<f4") for nm in names])


LAYOUTS = {"spz0": spz_dtype(0), "spz1": spz_dtype(1), "spz2": spz_dtype(2), "spz3": spz_dtype(3), "std": standard_dtype(), "cc": cc_dtype(),
           "bare2": no_normals_dtype()}
DESTINATIONS = {248: standard_dtype(), 251: spz_dtype(3)}

PLANTED = np.array([0x80000000, 0x00000001, 0x807fffff, 0x7f800001, 0xffc12345, 0x7fc00000, 0x7f800000, 0x00000000], np.uint32)


def table(dtype, n: int, seed: int = 0) -> np.ndarray:
    """n rows of random bytes: every 32-bit pattern may stand in a float field; -0.0, denormals, signalling and quiet NaNs with
    payloads and an infinity are planted in every float field of the first rows"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(7919 * dtype.itemsize + 31 * n + seed)
    t = rng.integers(0, 256, n * dtype.itemsize, dtype=np.uint8).view(dtype).copy()
    for j, nm in enumerate(nm for nm in dtype.names if dtype[nm] == np.dtype("<f4")):
        k = min(n, len(PLANTED))
        t[nm][:k] = np.roll(PLANTED, j)[:k].view(np.float32)
    return t


def aligned_bytes(nbytes: int, first_byte: int = 0, fill: int = GUARD) -> np.ndarray:
    """a uint8 view of `nbytes` bytes that starts at byte `first_byte` of a 16-byte aligned address, filled"""
    raw = np.full(nbytes + 32, fill, np.uint8)
    at = (-raw.ctypes.data) % 16 + first_byte
    return raw[at:at + nbytes]


def runs_cover_once(runs, src_stride: int, dst_stride: int) -> bool:
    """sorted by destination, inside both rows, every destination byte exactly once, no two joinable neighbours"""
    at = 0
    for k, (s, d, nb) in enumerate(runs):
        if d != at or nb < 1 or s < -1 or (s >= 0 and s + nb > src_stride):
            return False
        if k and ((s < 0 and runs[k - 1][0] < 0) or (s >= 0 and runs[k - 1][0] >= 0 and runs[k - 1][0] + runs[k - 1][2] == s)):
            return False
        at += nb
    return at == dst_stride


def bad_remap_arguments(src: int, dst: int, runs, n: int = 10, rows: int = 20, si: int = 107, so: int = 251):
    """[(what, (src, src_first, src_stride, n, runs, n_runs, dst, dst_first, dst_stride, dst_row0, dst_rows))]: every refusal of
    gsx_rows_remap_*; `src`, `dst`: 16-byte aligned addresses, `runs`: a valid int32 array of (si -> so) runs"""
    import ctypes as C
    good = [src, 0, si, n, runs, len(runs) // 3, dst, 0, so, 3, rows]

    def but(**kw):
        a = list(good)
        for k, v in kw.items():
            a[("src", "src_first", "si", "n", "runs", "n_runs", "dst", "dst_first", "so", "row0", "rows").index(k)] = v
        return tuple(a)

    def arr(*triples):
        flat = [v for t in triples for v in t]
        return (C.c_int32 * len(flat))(*flat)

    whole = [(-1, 0, so)]
    return [
        ("null source", but(src=None)), ("null destination", but(dst=None)), ("null runs", but(runs=None)),
        ("n < 0", but(n=-1)), ("n = 2^32", but(n=1 << 32, rows=1 << 33)), ("dst_rows < 0", but(rows=-1)), ("dst_rows = 2^32", but(rows=1 << 32)),
        ("row0 + n > rows", but(row0=11)), ("row0 < 0", but(row0=-1)),
        ("source stride 0", but(si=0)), ("source stride 513", but(si=513)), ("destination stride 0", but(so=0)),
        ("destination stride 513", but(so=513)),
        ("source first byte 16", but(src_first=16)), ("source first byte -1", but(src_first=-1)),
        ("destination first byte 16", but(dst_first=16)), ("destination first byte -1", but(dst_first=-1)),
        ("misaligned source", but(src=src + 4)), ("misaligned destination", but(dst=dst + 8)),
        ("no runs", but(n_runs=0)), ("129 runs", but(runs=arr(*[(-1, i, 1) for i in range(129)]), n_runs=129)),
        ("a run past the source row", but(runs=arr((si - 3, 0, 4), (-1, 4, so - 4)), n_runs=2)),
        ("a run past the destination row", but(runs=arr((-1, 0, so + 1)), n_runs=1)),
        ("a run before the destination row", but(runs=arr((-1, -1, so + 1)), n_runs=1)),
        ("a source offset of -2", but(runs=arr((-2, 0, so)), n_runs=1)),
        ("an empty run", but(runs=arr((0, 0, 0), *whole), n_runs=2)),
        ("a byte covered twice", but(runs=arr((0, 0, 8), (-1, 7, so - 7)), n_runs=2)),
        ("a byte not covered", but(runs=arr((0, 0, 8), (-1, 9, so - 9)), n_runs=2)),
    ]
