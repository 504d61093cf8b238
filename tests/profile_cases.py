"""Shared inputs of the two table-profile tests (test_table_profile_host.py, test_table_profile_gpu.py): tables at every tile
shape the kernel has (rows of up to 256 bytes: 128 per tile, wider ones: 64), row counts around the wave and the tile, fields
at aligned and odd byte offsets, the deciding value in the first row only and in the last row of a partial tile only, the values
on which the bit test and `!= 0` could part (denormal, NaN, -0.0), infinite and NaN coordinates, absent axes, and the two layouts
both entry points refuse.  numpy's answer comes from the reference's own expressions on the strided columns."""
import numpy as np

NS = (1, 63, 64, 65, 127, 128, 129, 1000)
ROW_BYTES = (68, 71, 104, 164, 248, 251, 512)
FIRST_BYTES = (0, 7)
DENORMAL = np.array([1], np.uint32).view(np.float32)[0]
NAN_PAYLOAD = np.array([0xffc12345], np.uint32).view(np.float32)[0]
AXES = ("x", "y", "z")


def table_dtype(row_bytes: int, n_rest: int, axes=AXES, shift: int = 0) -> np.dtype:
    """`axes`, then n_rest f_rest fields, packed from byte `shift`, in rows of row_bytes (the tail is padding).  An odd `shift`
    or row size puts fields at every byte alignment."""
    names = list(axes) + ["f_rest_%d" % i for i in range(n_rest)]
    assert shift + 4 * len(names) <= row_bytes
    return np.dtype({"names": names, "formats": ["<f4"] * len(names), "offsets": [shift + 4 * k for k in range(len(names))],
                     "itemsize": row_bytes})


def n_rest_for(row_bytes: int) -> int:
    """the widest of 9 / 24 / 45 f_rest fields that fits behind x y z and three bytes of shift"""
    return max(k for k in (0, 9, 24, 45) if 3 + 12 + 4 * k <= row_bytes)


def blank(n: int, dtype: np.dtype, seed: int) -> np.ndarray:
    """n rows: random bytes in the padding (nothing outside the fields may count), finite coordinates, every f_rest zero"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, n * dtype.itemsize, dtype=np.uint8)
    t = raw.view(dtype)
    for a in AXES:
        if a in dtype.fields:
            t[a] = rng.normal(0.0, 10.0, n).astype(np.float32)
    for nm in dtype.names:
        if nm.startswith("f_rest_"):
            t[nm] = 0.0
    return t


class Case:
    def __init__(self, name: str, table: np.ndarray):
        self.name, self.table = name, table

    def __repr__(self):
        return self.name


def expected(table: np.ndarray) -> dict:
    """numpy's answer: np.any(col != 0) per f_rest field (converter.py:121-146), np.min / np.max per axis (main.py:109-114)"""
    fields = table.dtype.fields
    word, lo, hi, nan_axes = 0, [], [], 0
    with np.errstate(all="ignore"):
        for i in range(45):
            nm = "f_rest_%d" % i
            if nm in fields and bool(np.any(table[nm] != 0)):
                assert bool(np.any(table[nm]))          # the CloudCompare writer's form of the same test
                word |= 1 << i
        for a, nm in enumerate(AXES):
            if nm not in fields:
                lo.append(float("inf"))
                hi.append(float("-inf"))
                continue
            mn, mx = float(np.min(table[nm])), float(np.max(table[nm]))
            if mn != mn or mx != mx:
                nan_axes |= 1 << a
            lo.append(mn)
            hi.append(mx)
    return {"rest_nonzero": word, "lo": tuple(lo), "hi": tuple(hi), "nan_axes": nan_axes, "n": len(table)}


def same(got: dict, want: dict) -> bool:
    """the issue's rule: the word, the NaN bits and n are equal; the bounds are `==` by value on the axes without a NaN (the
    sign of a zero is free) and nan on the others"""
    if (got["rest_nonzero"], got["nan_axes"], got["n"]) != (want["rest_nonzero"], want["nan_axes"], want["n"]):
        return False
    for a in range(3):
        if (want["nan_axes"] >> a) & 1:
            if got["lo"][a] == got["lo"][a] or got["hi"][a] == got["hi"][a]:
                return False
        elif got["lo"][a] != want["lo"][a] or got["hi"][a] != want["hi"][a]:
            return False
    return True


def cases():
    out, seed = [], 0
    # every row count at every row size: a random handful of non-zero f_rest values
    for rb in ROW_BYTES:
        for n in NS:
            seed += 1
            k = n_rest_for(rb)
            dt = table_dtype(rb, k, shift=(rb % 4))            # 71 and 251: fields at odd byte offsets
            t = blank(n, dt, seed)
            rng = np.random.default_rng(1000 + seed)
            for i in rng.choice(k, size=min(k, 3), replace=False) if k else ():
                t["f_rest_%d" % i][rng.integers(0, n)] = rng.normal()
            out.append(Case("rb%d_n%d" % (rb, n), t))
    # the single deciding non-zero: row 0 only; the last row of a partial tile only (both tile shapes, more than one block)
    for rb, n in ((248, 129), (248, 1000), (512, 65), (512, 1000), (71, 300)):
        k = n_rest_for(rb)
        for where, row in (("first", 0), ("last", n - 1)):
            seed += 1
            t = blank(n, table_dtype(rb, k, shift=rb % 4), seed)
            t["f_rest_%d" % (k - 1)][row] = 0.5
            t["f_rest_0"][row] = -2.0
            out.append(Case("single_%s_rb%d_n%d" % (where, rb, n), t))
    # denormal, NaN and -0.0 entries: a column of each alone
    seed += 1
    t = blank(300, table_dtype(248, 45), seed)
    t["f_rest_3"][299] = DENORMAL
    t["f_rest_17"][128] = NAN_PAYLOAD
    t["f_rest_44"][:] = -0.0
    t["f_rest_30"][5] = -DENORMAL
    out.append(Case("denormal_nan_negzero", t))
    # +-inf and NaN coordinates on one axis each; a zero extreme of either sign
    seed += 1
    t = blank(300, table_dtype(104, 9), seed)
    t["x"][7] = np.inf
    t["x"][290] = -np.inf
    t["y"][299] = NAN_PAYLOAD
    out.append(Case("inf_x_nan_y", t))
    seed += 1
    t = blank(200, table_dtype(68, 9), seed)
    t["x"] = -np.abs(t["x"])
    t["x"][199] = 0.0
    t["y"] = np.abs(t["y"])
    t["y"][0] = -0.0
    t["z"][:] = np.nan
    out.append(Case("zero_extremes_all_nan_z", t))
    # absent axes, 9 / 24 / 45 f_rest fields
    for axes, k in ((("x", "z"), 9), (("y",), 24), ((), 45), (AXES, 0)):
        seed += 1
        t = blank(257, table_dtype(248, k, axes=axes), seed)
        if k:
            t["f_rest_%d" % (k // 2)][256] = 1.0
        out.append(Case("axes_%s_rest%d" % ("".join(axes) or "none", k), t))
    return out


def refused_layouts(lib):
    """(name, ProfileLayout) that both entry points refuse with a message: a 513-byte row, an offset that leaves the row"""
    wide, _ = lib.profile_layout(table_dtype(512, 45))
    wide.row_bytes = 513
    out_of_row, _ = lib.profile_layout(table_dtype(248, 45))
    out_of_row.rest_offset[44] = 245
    return [("row_513", wide), ("offset_out_of_row", out_of_row)]
